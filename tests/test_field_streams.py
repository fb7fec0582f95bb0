"""The eight field multiplier streams of decaf377_amd/csrc/fe_asm.inc on the GPU, limb for limb.

fq29.hpp reaches D377_ASM_MUL, MUL_STRICT, SQR, SQR_STRICT and SQR2X, fqs29.hpp the signed SMUL, SSQR and SSQR2X, all behind
__HIP_DEVICE_COMPILE__: the CPU suite runs their statements (fe_mul_ref, fe_sqr_ref, fes_mul_ref), never the streams.
tests/cpp/field_streams.hip runs both on the device, one lane per row, on the operand rows the CPU suite proves legal
(test_limb_bounds_adversarial, test_signed_products) plus rows with a single extreme limb, and every row is held against
three things: the statement as hipcc translates it, a model on Python integers, and the representation contract itself.
The same products run under a lane predicate (partial exec mask, a lane mask live across the stream), in partial waves and
inside a loop with other products live; the device-compiled linear operations around them (fe_sub, fe_sub_nc, fe_carry,
fe_canon; fe_sub, fe_carry, fe_unsigned on fes) are checked at the rows of their host-simulation tests.

Everything is integer arithmetic and every comparison is exact.  The CPU tests pin the Python model of the unsigned streams
against the host simulation and prove every row (and every step of the chains) inside the contract."""
import ctypes
import functools
import os
import pickle
import re
import select
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_host_sim import (CARRIED, LAZY, TOP, WIDE, _adversarial_cases, _adversarial_linear_rows, _squarer_rows,
                           sim)  # noqa: F401  (sim: the host simulation fixture)
from test_signed_field import (MASK, NL, Q, QL, R_INV, RB, _linear_rows as _signed_linear_rows, _operands, _product_rows,
                               _stream, _value, ssim)  # noqa: F401  (ssim: the signed host simulation fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
R = 1 << 261
M32 = 0xFFFFFFFF
SENTINEL = 0xA5A5A5A5
STOP = 1 << 21                               # a signed top limb's extreme (test_signed_field._operands)
SWIDE = (1 << 30) + (1 << 29) + 16           # signed widths of test_signed_products, per kind
SWIDTH = {"mul": SWIDE, "sqr": (1 << 30) - (1 << 27), "sqr2x": CARRIED}

# harness op -> (name in messages, shape, strict digit, signed limbs); sim_raw_mul's modes are ops 0..4
OPS = [("fe_mul", "mul", False, False), ("fe_mul_strict", "mul", True, False), ("fe_sqr", "sqr", False, False),
       ("fe_sqr_strict", "sqr", True, False), ("fe_sqr2x", "sqr2x", False, False),
       ("fes fe_mul", "mul", False, True), ("fes fe_sqr", "sqr", False, True), ("fes fe_sqr2x", "sqr2x", False, True)]
OP_IDS = [o[0].replace(" ", "_") for o in OPS]


# ---- the model: fe_mul_ref / fe_sqr_ref column by column on Python integers ---------------------------------------------
def _ustream(a, b, kind, strict):
    """(result limbs, largest column accumulator): the 32-bit (strict: 29-bit) Montgomery digit, the SCALE2 form of 2 a^2."""
    a2 = [(x << 1) & M32 for x in a]
    acc, worst, m, r = 0, 0, [0] * NL, [0] * NL
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - (NL - 1)), min(k, NL - 1)
        if kind == "mul":
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        elif kind == "sqr":
            acc += sum(a2[i] * a[k - i] for i in range(lo, hi + 1) if 2 * i < k) + (a[k // 2] * a[k // 2] if k % 2 == 0 else 0)
        else:
            acc += sum(a2[i] * a2[k - i] for i in range(lo, hi + 1) if 2 * i < k) + (a2[k // 2] * a[k // 2] if k % 2 == 0 else 0)
        acc += sum(m[i] * QL[k - i] for i in range(lo, min(k, NL)))
        if k < NL:
            m[k] = -acc & (MASK if strict else M32)      # -q^-1 = -1 for either width
            acc += m[k]                                  # m_k * q_0: the low 29 (32) bits become zero
        else:
            r[k - NL] = acc & MASK
        worst = max(worst, acc)
        acc >>= RB
    r[NL - 1] = acc & M32
    return r, worst


def _model(op, x, y):
    """Result limbs of harness op `op`, asserting that no column leaves its accumulator (the operands are legal)."""
    _, kind, strict, signed = OPS[op]
    if signed:
        assert all(-(1 << 31) <= v < (1 << 31) for v in x + y) and (kind == "mul" or all(abs(v) < (1 << 30) for v in x))
        r, worst = _stream(x, y, kind)
        assert worst < 1 << 63, (OPS[op][0], x, y)
    else:
        assert all(0 <= v < (1 << 32) for v in x + y) and (kind == "mul" or all(v < (1 << 31) for v in x))
        r, worst = _ustream(x, y, kind, strict)
        assert worst < 1 << 64, (OPS[op][0], x, y)
    return r


def _contract(op, x, y, z):
    """None, or what the result z of op(x, y) breaks: the congruence, the value bound or the limb range."""
    _, kind, strict, signed = OPS[op]
    scale = 2 if kind == "sqr2x" else 1
    t, v = scale * _value(x) * _value(y if kind == "mul" else x), _value(z)
    if (v - t * R_INV) % Q != 0:
        return "value is not congruent to %d a b / 2^261 (mod q)" % scale
    if not all(0 <= l <= MASK for l in z[:8]):
        return "limb %d = %#x is outside [0, 2^29)" % next((i, l) for i, l in enumerate(z[:8]) if not 0 <= l <= MASK)
    if signed:
        if not t - Q * R < v * R <= t:
            return "value is outside (s a b / R - q, s a b / R]"
    elif not v < t // R + (1 if strict else 8) * Q + 1:
        return "value is not below a b / R + %d q" % (1 if strict else 8)
    return None


# ---- operand rows -------------------------------------------------------------------------------------------------------
def _unit(i, ext, top):
    return [(top if i == NL - 1 else ext) if j == i else 0 for j in range(NL)]


def _single_limb_rows(kind, signed):
    """Rows with one limb at its extreme and zeros elsewhere, one for each limb index (and sign): a product of two such rows
    is a single MAC of a single column.  Squarers also take two extreme limbs (the doubled cross terms)."""
    if signed:
        ea, eb, top, signs = SWIDTH[kind], CARRIED, STOP, (1, -1)
    else:
        ea, eb, top, signs = (CARRIED if kind == "sqr2x" else LAZY), LAZY, TOP, (1,)
    a_rows, b_rows, tags = [], [], []
    if kind == "mul":
        for i in range(NL):
            for j in range(NL):
                for sa in signs:
                    for sb in signs:
                        a_rows.append([sa * v for v in _unit(i, ea, top)])
                        b_rows.append([sb * v for v in _unit(j, eb, top)])
                        tags.append("single limb %sa[%d] x %sb[%d]" % ("-" if sa < 0 else "", i, "-" if sb < 0 else "", j))
    else:
        for i in range(NL):
            for sa in signs:
                a_rows.append([sa * v for v in _unit(i, ea, top)])
                tags.append("single limb %sa[%d]" % ("-" if sa < 0 else "", i))
            for j in range(i + 1, NL):
                for sa in signs:
                    for sb in signs:
                        a_rows.append([sa * p + sb * q for p, q in zip(_unit(i, ea, top), _unit(j, ea, top))])
                        tags.append("two limbs %sa[%d], %sa[%d]" % ("-" if sa < 0 else "", i, "-" if sb < 0 else "", j))
        b_rows = [list(r) for r in a_rows]
    return a_rows, b_rows, tags


class _Rows:
    """The operand rows of one op, their model results, and where the rows the issue counts lie."""
    def __init__(self, op):
        name, kind, strict, signed = OPS[op]
        if signed:
            a_rows, b_rows = _product_rows(kind)
            b_rows = b_rows[:len(a_rows)] if kind == "mul" else a_rows      # (test_signed_products zips the two lists)
            self.n_listed, self.extreme = len(a_rows), list(range(600, len(a_rows)))
            tags = ["test_signed_products[%s] row %d" % (kind, i) for i in range(len(a_rows))]
        else:
            a, b = _adversarial_cases()
            sel = list(range(len(a))) if kind == "mul" else _squarer_rows(a, 2 if kind == "sqr2x" else 1)
            a_rows = [[int(v) for v in a[i]] for i in sel]
            b_rows = [[int(v) for v in b[i]] for i in sel] if kind == "mul" else a_rows
            self.n_listed = len(sel)
            self.extreme = [k for k, i in enumerate(sel) if i % 202 < 2]       # each pairing's two all-extreme rows
            tags = ["test_limb_bounds_adversarial row %d" % i for i in sel]
        sa, sb, st = _single_limb_rows(kind, signed)
        self.a, self.b, self.tags = list(a_rows) + sa, list(b_rows) + sb, tags + st
        self.n_single = len(sa)
        self.want = [_model(op, x, y) for x, y in zip(self.a, self.b)]


@functools.lru_cache(maxsize=None)
def _rows(op):
    return _Rows(op)


# what the issue counts: listed rows per op (the squarers keep test_limb_bounds_adversarial's selection), all-extreme rows
# among them, single-limb rows
EXPECTED_COUNTS = {0: (1010, 10, 81), 1: (1010, 10, 81), 2: (808, 8, 45), 3: (808, 8, 45), 4: (404, 4, 45),
                   5: (649, 49, 324), 6: (649, 49, 162), 7: (649, 49, 162)}


def _check_counts(op):
    rows = _rows(op)
    assert (rows.n_listed, len(rows.extreme), rows.n_single) == EXPECTED_COUNTS[op], OPS[op][0]
    assert len(rows.a) == len(rows.b) == len(rows.want) == len(rows.tags) == rows.n_listed + rows.n_single
    _, kind, _, signed = OPS[op]
    for k in rows.extreme:                   # the all-extreme rows are what they are said to be
        if signed:
            assert set(rows.a[k][:8]) <= {-SWIDTH[kind], SWIDTH[kind], 0, -1, MASK, -4, MASK + 8} and abs(rows.a[k][8]) in (0, STOP)
        else:
            assert len(set(rows.a[k][:8])) == 1 and rows.a[k][0] in (LAZY, CARRIED, WIDE) and rows.a[k][8] in (0, TOP)
    return rows


def _u32(rows):
    return np.array([[v & M32 for v in r] for r in rows], np.uint32).reshape(len(rows), NL)


def _ints(arr, signed):
    return (arr.view(np.int32) if signed else arr).tolist()


# ---- CPU: the model against the host simulation, every row inside the contract -----------------------------------------
@pytest.mark.parametrize("op", range(5), ids=OP_IDS[:5])
def test_unsigned_model_matches_host_simulation(sim, op):  # noqa: F811
    """The Python model of the unsigned streams gives sim_raw_mul's limbs (the statements as g++ translates them) on every
    row the GPU test runs, no column reaches 2^64, and the model's results keep the contract."""
    rows = _check_counts(op)
    a, b = _u32(rows.a), _u32(rows.b)
    out = np.zeros_like(a)
    sim.sim_raw_mul(op, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(a)),
                    out.ctypes.data_as(ctypes.c_void_p))
    for x, y, z, w, tag in zip(rows.a, rows.b, out.tolist(), rows.want, rows.tags):
        assert z == w, (OPS[op][0], tag)
        assert _contract(op, x, y, w) is None, (OPS[op][0], tag)


@pytest.mark.parametrize("op", range(5, 8), ids=OP_IDS[5:])
def test_signed_rows_match_host_simulation(ssim, op):  # noqa: F811
    """The signed rows (test_signed_products' and the single-limb ones): every partial column sum inside +-2^63, the model
    (test_signed_field._stream) equal to the statement fes_mul_ref, its results inside the contract."""
    rows = _check_counts(op)
    a, b = _u32(rows.a), _u32(rows.b)
    out = np.zeros_like(a)
    ssim.sims_field_op(op - 5, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(a)),
                       out.ctypes.data_as(ctypes.c_void_p))
    for x, y, z, w, tag in zip(rows.a, rows.b, _ints(out, True), rows.want, rows.tags):
        assert z == w, (OPS[op][0], tag)
        assert _contract(op, x, y, w) is None, (OPS[op][0], tag)


# ---- the chains of tests/cpp/field_streams.hip (chain<OP>) on the model -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sub32q():
    text = open(os.path.join(CSRC, "fq29.hpp")).read()
    limbs = [int(v, 16) for v in re.findall(r"0x[0-9a-f]+", re.search(r"SUB32Q\[NL\] = \{([^}]*)\}", text).group(1))]
    assert len(limbs) == NL and _value(limbs) == 32 * Q
    return limbs


def _fe_carry(t):
    return [t[0] & MASK] + [(t[i] & MASK) + (t[i - 1] >> RB) for i in range(1, NL - 1)] + [t[NL - 1] + (t[NL - 2] >> RB)]


def _fe_sub(a, b):
    off = _sub32q()
    assert all(y <= o for y, o in zip(b, off)) and _value(b) < 31 * Q          # fe_sub's precondition
    t = [x + o - y for x, o, y in zip(a, off, b)]
    assert all(v < (1 << 32) for v in t)
    return _fe_carry(t)


def _add(a, b):
    return [x + y for x, y in zip(a, b)]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _chain_model(op, a, b, iters):
    """chain<OP> of the harness; _model asserts every product's operands and columns inside the contract."""
    signed = OPS[op][3]
    mul = lambda p, q: _model(5 if signed else 0, p, q)
    sqr = lambda p: _model(6 if signed else 2, p, p)
    x, y, u, v = sqr(a), b, mul(a, b), sqr(b)
    for _ in range(iters):
        x = _model(op, x if op == 4 else _sub(x, u) if signed else _add(x, u), y)
        u = mul(u, x)
        v = sqr(_sub(v, x) if signed else _add(v, x))
    r = _sub(_add(x, u), v) if signed else _fe_sub(_add(x, u), v)
    assert all(-(1 << 31) <= l < (1 << 31) for l in r)
    return r


CHAIN_ROWS, CHAIN_ITERS = 64, 64


@functools.lru_cache(maxsize=None)
def _chain_rows(op):
    """64 operand rows inside a chain's contract and the model's results.  fe: carried x carried rows of
    test_limb_bounds_adversarial (both all-extreme rows first); fes: rows of carried width and either sign, the 49 extreme
    mixes among them."""
    if OPS[op][3]:
        rng = np.random.default_rng(20 + op)
        a_rows = _operands(rng, CHAIN_ROWS - 49, CARRIED)
        b_rows = _operands(rng, CHAIN_ROWS - 49, CARRIED)
        b_rows = b_rows[::-1]
    else:
        a, b = _adversarial_cases()
        a_rows = [[int(v) for v in r] for r in a[4 * 202:4 * 202 + CHAIN_ROWS]]
        b_rows = [[int(v) for v in r] for r in b[4 * 202:4 * 202 + CHAIN_ROWS]]
        assert a_rows[0] == [CARRIED] * 8 + [TOP] and b_rows[1] == [CARRIED] * 8 + [0]
    assert len(a_rows) == len(b_rows) == CHAIN_ROWS
    return a_rows, b_rows, [_chain_model(op, x, y, CHAIN_ITERS) for x, y in zip(a_rows, b_rows)]


@pytest.mark.parametrize("op", range(8), ids=OP_IDS)
def test_chain_model_stays_inside_the_contract(op):
    """Every product of every step of the chain the GPU test runs takes legal operands (asserted inside the model): the
    device chain can then be held to exact equality."""
    a_rows, b_rows, want = _chain_rows(op)
    assert len(want) == CHAIN_ROWS and len({tuple(w) for w in want}) == CHAIN_ROWS      # not a degenerate chain


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class _Device:
    """build/field_streams.so in a child process (tests/field_streams_worker.py): the harness's HIP runtime stays out of this
    process, where torch brings its own.  The first launch that reports a HIP error, ends the worker or does not answer fails
    its test and every later call: no further launches."""
    REPLY_SECONDS = 120

    def __init__(self, so):
        self.error = None
        self.proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "field_streams_worker.py"), so],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, bufsize=0)

    def _read(self, n):
        buf = b""
        while len(buf) < n:
            if not select.select([self.proc.stdout], [], [], self.REPLY_SECONDS)[0]:
                self.proc.kill()
                return None
            chunk = self.proc.stdout.read(n - len(buf))
            if not chunk:
                return None
            buf += chunk
        return buf

    def call(self, name, *args):
        if self.error is not None:
            pytest.fail("no further launches: %s" % self.error)
        what = "%s%r" % (name, tuple(a for a in args if not isinstance(a, np.ndarray)))
        try:
            payload = pickle.dumps((name, args))
            self.proc.stdin.write(struct.pack("<Q", len(payload)) + payload)
            head = self._read(8)
            body = self._read(struct.unpack("<Q", head)[0]) if head else None
        except OSError:
            body = None
        if body is None:
            self.error = "%s: the worker ended or did not answer (exit status %s)" % (what, self.close())
            pytest.fail(self.error)
        rc, arrays = pickle.loads(body)
        if rc != 0:
            self.error = "%s returned %d (a HIP error code; -1: rejected arguments)" % (what, rc)
            pytest.fail(self.error)
        for mine, theirs in zip([a for a in args if isinstance(a, np.ndarray)], arrays):
            mine[...] = theirs

    def close(self):
        for f in (self.proc.stdin, self.proc.stdout):
            try:
                f.close()
            except OSError:
                pass
        try:
            return self.proc.wait(timeout=30)
        except subprocess.TimeoutExpired:
            self.proc.kill()
            return self.proc.wait()


@pytest.fixture(scope="module")
def dev():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "field_streams.so")
    deps = [os.path.join(ROOT, "tests", "cpp", "field_streams.hip")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(so) or any(os.path.getmtime(d_) > os.path.getmtime(so) for d_ in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC",
                               "-shared", deps[0], "-o", so], timeout=900)
    d = _Device(so)
    yield d
    d.close()


def _require_equal(op, tags, what, got, want):
    """got, want: lists of limb rows.  Fails naming the op, the row and the first differing limb."""
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            i = next(i for i in range(NL) if g[i] != w[i])
            n_bad = sum(1 for g_, w_ in zip(got, want) if g_ != w_)
            pytest.fail("%s, %s (row %d of %d, %d rows differ): the stream differs from %s first at limb %d: got %#x, want %#x\n"
                        "  got  %s\n  want %s" % (OPS[op][0], tags[k], k, len(got), n_bad, what, i, g[i] & M32, w[i] & M32, g, w))


@pytest.mark.gpu
@pytest.mark.parametrize("op", range(8), ids=OP_IDS)
def test_products_on_the_gpu(dev, op):
    """Every contract-edge row through the stream: equal to the statement compiled for the same device, equal to the model on
    Python integers, and inside the contract (congruence, value bound, limb range), in that order of reporting."""
    rows = _check_counts(op)
    signed = OPS[op][3]
    a, b = _u32(rows.a), _u32(rows.b)
    n = len(a)
    assert n % 64 != 0                       # the last wave is partial
    got, want = np.full((n, NL), SENTINEL, np.uint32), np.full((n, NL), SENTINEL, np.uint32)
    dev.call("streams_product", op, a, b, n, got, want)
    got, want = _ints(got, signed), _ints(want, signed)
    _require_equal(op, rows.tags, "its statement on the device", got, want)
    _require_equal(op, rows.tags, "the model", got, rows.want)
    for x, y, z, tag in zip(rows.a, rows.b, got, rows.tags):
        broken = _contract(op, x, y, z)
        assert broken is None, "%s, %s: %s (a %s, b %s, got %s)" % (OPS[op][0], tag, broken, x, y, z)


@pytest.mark.gpu
@pytest.mark.parametrize("op", range(8), ids=OP_IDS)
def test_predicated_products_on_the_gpu(dev, op):
    """The product under a lane predicate (odd rows; a test on the row's data) at sizes around the wave: active lanes give the
    model's limbs and the flag of a comparison made before the stream, inactive lanes keep the sentinel."""
    rows = _rows(op)
    signed = OPS[op][3]
    for mode in (1, 2):
        for n in (1, 63, 64, 65, 257):
            # the listed rows' extremes first (the unsigned list opens with them, the signed one ends in them)
            idx = list(range(rows.n_listed - n, rows.n_listed)) if signed else list(range(n))
            xa, xb = [rows.a[i] for i in idx], [rows.b[i] for i in idx]
            a, b = _u32(xa), _u32(xb)
            got, want = np.full((n, NL), SENTINEL, np.uint32), np.full((n, NL), SENTINEL, np.uint32)
            flag = np.full(n, SENTINEL, np.uint32)
            dev.call("streams_predicated", op, mode, a, b, n, got, want, flag)
            active = [(i & 1) == 1 if mode == 1 else ((int(a[i, 0]) ^ i) & 3) == 1 for i in range(n)]
            assert n == 1 or any(active) and not all(active)
            sent = [SENTINEL - (1 << 32) if signed else SENTINEL] * NL
            tags = ["mode %d, n %d, %s lane %d: %s" % (mode, n, "active" if active[i] else "inactive", i, rows.tags[idx[i]]) for i in range(n)]
            expect = [rows.want[idx[i]] if active[i] else sent for i in range(n)]
            _require_equal(op, tags, "the model (inactive lanes: the sentinel)", _ints(got, signed), expect)
            _require_equal(op, tags, "its statement on the device", _ints(got, signed), _ints(want, signed))
            want_flag = [(1 if int(a[i, 1]) < int(b[i, 2]) else 2) if active[i] else SENTINEL for i in range(n)]
            assert flag.tolist() == want_flag, "%s, mode %d, n %d: the lane mask held across the stream changed" % (OPS[op][0], mode, n)


@pytest.mark.gpu
@pytest.mark.parametrize("op", range(8), ids=OP_IDS)
def test_chains_on_the_gpu(dev, op):
    """x = op(x (+|-) u, y) 64 times in a loop that is not unrolled, two more products live in it and folded into the result:
    the chain on the streams equals the chain on the statements and the chain on the model, on 64 rows."""
    a_rows, b_rows, model = _chain_rows(op)
    signed = OPS[op][3]
    a, b = _u32(a_rows), _u32(b_rows)
    got, want = np.zeros((CHAIN_ROWS, NL), np.uint32), np.zeros((CHAIN_ROWS, NL), np.uint32)
    dev.call("streams_chain", op, a, b, CHAIN_ROWS, CHAIN_ITERS, got, want)
    tags = ["chain of %d, row %d" % (CHAIN_ITERS, i) for i in range(CHAIN_ROWS)]
    _require_equal(op, tags, "the chain on its statements on the device", _ints(got, signed), _ints(want, signed))
    _require_equal(op, tags, "the chain on the model", _ints(got, signed), model)


@pytest.mark.gpu
def test_unsigned_linear_operations_on_the_gpu(dev):
    """fe_sub, fe_sub_nc, fe_carry and fe_canon as compiled for the device, at the rows and with the assertions of
    test_limb_bounds_adversarial (fe_carry: that test's product operands, lazy and wide limbs)."""
    (sub_a, sub_b), (nc_a, nc_b), reps = _adversarial_linear_rows()
    out = np.zeros((8, NL), np.uint32)
    dev.call("streams_linear", 0, sub_a, sub_b, 8, out)
    for i in range(8):
        assert _value(sub_b[i]) < 31 * Q
        assert _value(out[i]) == _value(sub_a[i]) - _value(sub_b[i]) + 32 * Q, ("fe_sub", i)
        assert all(int(x) < (1 << 29) + 8 for x in out[i][:8]), ("fe_sub", i)
        assert out[i].tolist() == _fe_sub(sub_a[i].tolist(), sub_b[i].tolist()), ("fe_sub", i)
    out = np.zeros((4, NL), np.uint32)
    dev.call("streams_linear", 1, nc_a, nc_b, 4, out)
    for i in range(4):
        assert _value(out[i]) == _value(nc_a[i]) - _value(nc_b[i]) + 16 * Q, ("fe_sub_nc", i)
        assert all(int(x) < int(y) + (1 << 30) + 8 for x, y in zip(out[i][:8], nc_a[i][:8])), ("fe_sub_nc", i)
    a, b = _adversarial_cases()
    n = len(a)
    assert n == 1010
    out = np.zeros((n, NL), np.uint32)
    dev.call("streams_linear", 2, a, b, n, out)
    for i in range(n):
        assert out[i].tolist() == _fe_carry(a[i].tolist()), ("fe_carry", i)
        assert _value(out[i]) == _value(a[i]) and all(int(x) < (1 << 29) + 8 for x in out[i][:8]), ("fe_carry", i)
    # canonicalisation of the representatives of zero and of small multiples of q (relaxed products reach 8q+)
    out = np.full((12, NL), SENTINEL, np.uint32)
    dev.call("streams_linear", 3, reps, reps, 12, out)
    assert not out.any(), "fe_canon of k q"
    # and of the adversarial rows: the plain value a / 2^261 mod q itself
    out = np.zeros((n, NL), np.uint32)
    dev.call("streams_linear", 3, a, b, n, out)
    for i in range(n):
        assert _value(out[i]) == _value(a[i]) * R_INV % Q and all(int(x) <= MASK for x in out[i][:8]), ("fe_canon", i)


@pytest.mark.gpu
def test_signed_linear_operations_on_the_gpu(dev):
    """fe_sub, fe_carry and fe_unsigned on fes as compiled for the device, at the rows and with the assertions of
    test_signed_linear_and_conversion."""
    a, b, p = _signed_linear_rows()
    n = len(a)
    assert n == 400 and n % 64 != 0
    ua, ub, up = a.view(np.uint32), b.view(np.uint32), p.view(np.uint32)
    r = np.zeros((n, NL), np.uint32)
    dev.call("streams_linear", 5, ua, ub, n, r)
    assert (r.view(np.int32).astype(np.int64) == a.astype(np.int64) - b).all(), "fes fe_sub"
    dev.call("streams_linear", 4, ua, ub, n, r)
    for x, z in zip(a.tolist(), r.view(np.int32).tolist()):
        assert _value(z) == _value(x) and all(-2 <= l < (1 << 29) + 2 for l in z[:8]), ("fes fe_carry", x, z)
    dev.call("streams_linear", 6, up, ub, n, r)
    for x, z in zip(p.tolist(), r.tolist()):
        assert _value(z) == _value(x) + 2 * Q and all(l < (1 << 29) + 8 for l in z[:8]), ("fe_unsigned", x, z)
