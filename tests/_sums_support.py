"""What the tests of the batched sums share, one copy each: planted scalars and bases, the oracle's byte-table fold over fixed
bases (Fold), device copies and resident calls on a side stream (Side), the gate and the stream control of the two-stream
cases (Gate, pick_independent_stream), and the build-and-run of a C++ mirror program."""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from _oracle import _p  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 2111115437357092606062206234695386632838870926408408195193685246394721360383
THREADS = 16


def scalar_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def planted_scalars(rng, n, m):
    """n x m random scalars, term-major, with 0, 1, r - 1, r and 2^256 - 1 planted and every term of the first sum 2^256 - 1."""
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    for t, v in enumerate([0, 1, R - 1, R, (1 << 256) - 1]):
        k[(7 * t + 3) % (n * m)] = scalar_bytes(v)
    k[:m] = scalar_bytes((1 << 256) - 1)
    return k


def random_bases(oracle, rng, m):
    """m random Elligator outputs, GENERATOR among them from m = 3 on."""
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (m, 32), dtype=np.uint8))
    if m >= 3:
        pts[1] = oracle.generator_xyzt()
    return np.ascontiguousarray(pts, dtype=np.uint64)


def host_scalars(rng, n, m):
    """The host simulations' scalars: n x m, term-major within a sum, random 32-byte strings with 0, 1, r - 1, r and
    2^256 - 1 spread over them."""
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    for t, v in enumerate([0, 1, R - 1, R, (1 << 256) - 1]):
        for j in range(m):
            k[(t * m + j * (t + 1)) % (n * m)] = scalar_bytes(v)
    k[:m] = scalar_bytes(R - 1)                                   # the first sum: every term r - 1
    return k


def host_bases(oracle, rng, m):
    """The host simulations' bases: random Elligator outputs, the identity, GENERATOR, a representative with Z != 1 and one
    that differs from its point by the 2-torsion point (0, -1)."""
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (m + 2, 32), dtype=np.uint8))
    out = [pts[0]]
    kinds = ["identity", "generator", "scaled", "torsion"]
    for j in range(1, m):
        kind = kinds[(j - 1) % len(kinds)]
        if kind == "identity":
            out.append(oracle.identity_xyzt())
        elif kind == "generator":
            out.append(oracle.generator_xyzt())
        elif kind == "scaled":                                      # (lX, lY, lZ, lT): the same point, Z != 1
            p = pts[j].reshape(4, 4)
            lam = np.tile(oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0][:4], (4, 1))
            out.append(oracle.fq_op(2, p, lam)[0].reshape(16))
        else:                                                      # (-X, -Y, Z, T) = P + (0, -1)
            p = pts[j].reshape(4, 4).copy()
            p[:2] = oracle.fq_op(4, p[:2])[0]
            out.append(p.reshape(16))
    return np.ascontiguousarray(np.stack(out), dtype=np.uint64)


def indexed_fold_by_scalar_mul(oracle, bases, idx, k):
    """The oracle's sums: sum_j k[i t + j] * B_{idx[i, j]} by scalar multiplications and additions; an absent term is
    0 * identity -> (encodings, records)."""
    n, t = idx.shape
    flat = idx.reshape(-1)
    pts = np.where((flat >= 0)[:, None], bases[np.maximum(flat, 0)], oracle.identity_xyzt()[None, :])
    kk = np.where((flat >= 0)[:, None], k, 0).astype(np.uint8)
    terms = oracle.scalar_mul_xyzt(np.ascontiguousarray(pts, dtype=np.uint64), np.ascontiguousarray(kk)).reshape(n, t, 16)
    acc = np.ascontiguousarray(terms[:, 0])
    for j in range(1, t):
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(terms[:, j]))
    return oracle.compress(acc), acc


def threaded(f, n):
    """f(lo, hi) on THREADS slices of 0 .. n, concatenated (the oracle's calls release the interpreter lock)."""
    bounds = np.linspace(0, n, THREADS + 1).astype(int)
    with ThreadPoolExecutor(THREADS) as ex:
        return np.concatenate(list(ex.map(lambda q: f(bounds[q], bounds[q + 1]), range(THREADS))))


class Fold:
    """The oracle's sums over fixed bases the way a comb does them, with the oracle's own group law: k B = sum_w (byte w of
    k mod r) 256^w B, the 32 x 256 multiples of each base made once by oracle additions and doublings and every term folded
    by oracle additions on THREADS threads -- the same values as scalar_mul_xyzt, 10x cheaper, and the encodings are
    canonical, so they compare byte for byte.  Term j of a sum picks the table of base idx[i, j]; an absent term (-1) adds
    entry 0, the identity."""

    def __init__(self, oracle, bases):
        self.o = oracle
        self.m = bases.shape[0]
        ident = oracle.identity_xyzt()
        tabs = np.zeros((self.m, 32, 256, 16), np.uint64)
        p = np.ascontiguousarray(bases, dtype=np.uint64)
        for w in range(32):
            acc = np.tile(ident, (self.m, 1))
            for b in range(256):
                tabs[:, w, b] = acc
                acc = oracle.add_xyzt(acc, p)
            for _ in range(8):
                p = oracle.double_xyzt(p)
        self.tabs = tabs

    def _part(self, idx, kb, lo, hi):
        acc = np.tile(self.o.identity_xyzt(), (hi - lo, 1))
        for j in range(idx.shape[1]):
            comb = idx[lo:hi, j]
            for w in range(32):
                acc = self.o.add_xyzt(acc, self.tabs[comb, w, kb[lo:hi, j, w]])
        return acc

    def records(self, idx, k):
        """[n, 16]: the sums of the [n, t] index rows `idx` with the scalars k [n * t, 32]."""
        n, t = idx.shape
        kb = self.o.fr_from_bytes_mod_order(k).reshape(n, t, 32).copy()
        kb[idx < 0] = 0                                          # an absent term: entry 0 of comb 0, the identity
        comb = np.maximum(idx, 0)
        return threaded(lambda lo, hi: self._part(comb, kb, lo, hi), n)

    def __call__(self, idx, k):
        """-> (encodings, records) of the indexed sums."""
        acc = self.records(idx, k)
        return self.o.compress(acc), acc

    def dense(self, k):
        """-> (encodings, records) of the sums over every base in order: the indexed fold with idx[i, j] = j."""
        n = k.shape[0] // self.m
        return self(np.tile(np.arange(self.m), (n, 1)), k)


# the planted sums of mixed_case, within the first 63 (sum 0: see mixed_case)
ZROW, ABSENT, VZERO, DOUBLE, CANCEL = 10, 11, 12, 13, 14


def var_terms(oracle, pts, vk, n, v):
    """[n, v, 16]: the oracle's k P of every variable term; a record with Z = 0 counts as the identity."""
    q = pts.copy()
    q[~q[:, 8:12].any(1)] = oracle.identity_xyzt()
    return threaded(lambda lo, hi: oracle.scalar_mul_xyzt(np.ascontiguousarray(q[lo:hi]), np.ascontiguousarray(vk[lo:hi])),
                     n * v).reshape(n, v, 16)


def join(oracle, fixed, terms, live=None):
    """fixed sums + the variable terms (those with live[i, p] false left out) -> (encodings, records)."""
    acc = np.ascontiguousarray(fixed)
    ident = oracle.identity_xyzt()
    for p in range(terms.shape[1]):
        tp = np.ascontiguousarray(terms[:, p])
        if live is not None:
            tp = np.where(live[:, p, None], tp, ident[None, :])
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(tp, dtype=np.uint64))
    return oracle.compress(acc), acc


def mixed_case(oracle, v, t, m, n, seed=0):
    """Bases, index rows, scalars and points of n mixed sums with the planted rows of tests/test_msm_mixed_host.py.  Sum 0 (all that
    n = 1 sees) has the largest scalars on both sides and its last fixed term absent when t > 1."""
    rng = np.random.default_rng(1000 * v + 10 * t + m + seed)
    bases = random_bases(oracle, rng, m)
    fk, vk = planted_scalars(rng, n, t), planted_scalars(rng, n, v)
    idx = rng.integers(0, m, (n, t)).astype(np.int32)
    idx[rng.random((n, t)) < 0.1] = -1
    idx[0] = m - 1
    if t > 1:
        idx[0, t - 1] = -1
    idx[2] = 1 % m                                               # one index repeated
    pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (n * v, 32), dtype=np.uint8)), dtype=np.uint64)
    if n > CANCEL:
        pts[5 * v] = oracle.identity_xyzt()
        pts[ZROW * v, 8:12] = 0                                  # a record with Z = 0
        idx[ABSENT] = -1                                         # no fixed term: the variable sum alone
        vk[VZERO * v:(VZERO + 1) * v] = 0                        # every variable scalar 0: the fixed sum alone
        kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
        for row, other in ((DOUBLE, kv), (CANCEL, R - kv)):      # P_0 = B_0 meets the fixed term on base 0: doubling, cancelling
            idx[row] = -1
            idx[row, t - 1] = 0
            fk[row * t + t - 1] = scalar_bytes(kv)
            vk[row * v:(row + 1) * v] = 0
            vk[row * v] = scalar_bytes(other)
            pts[row * v] = bases[0]
    return bases, np.ascontiguousarray(idx), fk, pts, vk


class Side:
    """Device copies of host arrays and the resident calls on ONE side stream; host() synchronises that stream alone.
    stream2: an optional second stream for the two-stream cases (pick_independent_stream); nothing here uses it unasked."""

    def __init__(self, torch, ctx, stream2=None):
        self.torch, self.ctx, self.lib = torch, ctx, ctx._lib
        self.stream = torch.cuda.Stream(device="cuda:0")
        self.stream2 = stream2

    def dev(self, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
        self.torch.cuda.current_stream().synchronize()           # the copy is done before the side stream reads it
        return t

    def empty(self, shape, kind="u8", fill=None):
        dt = {"u8": self.torch.uint8, "u64": self.torch.int64}[kind]
        t = self.torch.empty(shape, dtype=dt, device="cuda:0") if fill is None else self.torch.full(shape, fill, dtype=dt, device="cuda:0")
        self.torch.cuda.current_stream().synchronize()
        return t

    def call(self, name, *args, stream=None):
        """rc of the resident call `name`: (ctx, dev 0, the side stream, *args), tensors passed as their device pointers."""
        conv = [ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a for a in args]
        s = self.stream.cuda_stream if stream is None else stream
        return getattr(self.lib, name)(self.ctx._h, 0, ctypes.c_void_p(s), *conv)

    def ok(self, name, *args, stream=None):
        rc = self.call(name, *args, stream=stream)
        assert rc == 0, (name, rc, self.lib.d377_last_error().decode())

    def host(self, t):
        self.stream.synchronize()
        a = t.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a


class Gate:
    """A stretch of plain torch kernels (y = x @ w, the two buffers swapping) that keeps a stream busy for at least min_ms:
    whatever is enqueued behind it on that stream cannot start before it ends, however fast the host is.  The loop count is
    sized once: a short probe gives the time per kernel, the sized loop is then timed once with torch events (`measured_ms`,
    at least min_ms or the constructor fails).  start() makes no call of the library under test and no tensor."""

    def __init__(self, torch, min_ms=200.0, size=4096, aim=1.5):
        self.torch, self.min_ms = torch, min_ms
        self.stream = torch.cuda.Stream(device="cuda:0")         # the sizing runs here, not on the streams of the cases
        g = torch.Generator(device="cuda:0").manual_seed(1)
        self.x = torch.randn((size, size), device="cuda:0", generator=g)
        self.y = torch.empty_like(self.x)
        self.w = torch.randn((size, size), device="cuda:0", generator=g) / size ** 0.5   # (keeps the products' size steady)
        torch.cuda.synchronize()
        self.count = 2
        self._timed()                                            # warm-up: the BLAS library's own set-up
        probe = 16
        self.count = probe
        per = self._timed() / probe
        self.count = max(probe, int(aim * min_ms / per) + 1)
        self.measured_ms = self._timed()                         # the one timing of the sized loop
        assert self.measured_ms >= min_ms, "the gate takes %.1f ms at %d kernels, under %.0f" % (self.measured_ms, self.count, min_ms)

    def _timed(self):
        t0, t1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        t0.record(self.stream)
        end = self.start(self.stream)
        t1.record(self.stream)
        end.synchronize()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def start(self, stream):
        """Enqueues the gate on `stream` -> the event recorded behind its last kernel (query() is false while it runs)."""
        torch = self.torch
        a, b = self.x, self.y
        with torch.cuda.stream(stream):
            for _ in range(self.count):
                torch.mm(a, self.w, out=b)
                a, b = b, a
        end = torch.cuda.Event()
        end.record(stream)
        return end


def runs_beside(torch, gate, s1, work):
    """Does `work()` -- which enqueues something and waits for it on the host -- come back while a gate is still running on
    s1?  True: what it ran on shares no queue with s1.  (False costs the whole gate: the wait ended with it.)"""
    end = gate.start(s1)
    work()
    beside = not end.query()
    s1.synchronize()
    return beside


def pick_independent_stream(torch, gate, s1, candidates=8):
    """The control of the two-stream cases: HIP maps streams onto a few hardware queues, and two streams on one queue run in
    order with or without a guard.  Tries up to `candidates` fresh streams: with a gate running on s1, one trivial torch op on
    the candidate and a synchronize() of it; the candidate is independent of s1 if the gate is still running afterwards.
    -> (stream or None, the candidate's number or None)."""
    probe = torch.zeros(64, device="cuda:0")
    torch.cuda.synchronize()
    for c in range(candidates):
        s = torch.cuda.Stream(device="cuda:0")

        def work():
            with torch.cuda.stream(s):
                probe.add_(1)
            s.synchronize()

        if runs_beside(torch, gate, s1, work):
            return s, c
    return None, None


def build_and_run_cpp(name, marker, hip_headers=False):
    """Compiles tests/cpp/`name`.cpp against the library (with the HIP headers for a program that makes streams of its own)
    and runs it: it must exit 0 and print `marker`."""
    from decaf377_amd import _native
    libdir = os.path.dirname(_native.LIB_PATH)
    exe = os.path.join(ROOT, "tests", "cpp", name)
    hip = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] if hip_headers else []
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + hip + ["-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L" + libdir, "-ldecaf377_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
