"""CPU check of k_scalar_mul_var's lane: the decompression's square root on signed limbs and the window table that keeps
no entry 0 of its own.

tests/host_sim/vb_signed_sqrt_sim.cpp (sim.cpp plus the signed square root and a table that refuses store(0)) is compiled
for the host with g++.  The chain on fes must give the root and the flag of the chain on fe, limb for limb after
canonicalisation, and both must be the Python model's (oracle/d377_model.py); the -DD377_BOUNDS build walks the same inputs
with every precondition asserted (each column of each signed product inside +-2^63, each s_lookup key one of x, x + q);
and the scalar multiplication through the shared-identity table must be the oracle's, byte for byte."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383
N_SQRT = 1 << 10


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def n_(n):
    return ctypes.c_size_t(n)


def _build(name, flags):
    lib = os.path.join(SIM_DIR, name)
    srcs = [os.path.join(SIM_DIR, f) for f in ("vb_signed_sqrt_sim.cpp", "sim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC] + flags +
                              [os.path.join(SIM_DIR, "vb_signed_sqrt_sim.cpp"), "-o", lib])
    return lib


@pytest.fixture(scope="module")
def vss():
    L = ctypes.CDLL(_build("libd377_vb_signed_sqrt_sim.so", ["-O2", "-DD377_FB_BITS=12"]))
    L.sim_init.restype = ctypes.c_int
    L.vss_scalar_mul_var.restype = ctypes.c_ulong
    L.vss_scalar_mul_var_el.restype = ctypes.c_ulong
    assert L.sim_init() == 0
    return L


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("d377_model", os.path.join(ROOT, "oracle", "d377_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _sqrt_inputs(kats):
    """(num, den) rows as 32-byte strings: the reference's sqrt edge cases, den = 0 and num = 0 in several forms, then seeded
    pairs up to 2^10 rows -- random 256-bit strings (reduced on the way in), ratios that are squares by construction, the
    same ratios times a fixed non-residue, and small values."""
    rng = np.random.default_rng(2377)
    rows = [(c["num"], c["den"]) for c in kats["sqrt_edge_cases"]["cases"]]
    rows += [(1, 0), (0, 0), (5, Q), (Q, 7), (Q - 1, 0), (1, 1), (1, Q - 1), (Q - 1, Q - 1), (2, 1), (1, 2), (1 << 248, 1 << 248),
             ((1 << 256) - 1, (1 << 256) - 1), (1, (1 << 256) - 1)]
    nonres = None
    for c in range(2, 50):
        if pow(c, (Q - 1) // 2, Q) == Q - 1:
            nonres = c
            break
    while len(rows) < N_SQRT:
        kind = len(rows) % 4
        a = int.from_bytes(rng.bytes(32), "little")
        b = int.from_bytes(rng.bytes(32), "little")
        if kind == 0:
            rows.append((a, b))
        elif kind == 1:                       # num / den = a^2: a square
            rows.append((a * a % Q * (b % Q) % Q, b % Q))
        elif kind == 2:                       # the same times a non-residue: not a square (unless a or b is 0 mod q)
            rows.append((a * a % Q * (b % Q) % Q * nonres % Q, b % Q))
        else:
            rows.append((int(rng.integers(0, 1 << 20)), int(rng.integers(1, 1 << 20))))
    num = np.stack([_le(a) for a, _ in rows])
    den = np.stack([_le(b) for _, b in rows])
    return rows, np.ascontiguousarray(num), np.ascontiguousarray(den)


def _run_sqrt(L, signed, with_inv, num, den):
    n = len(num)
    canon = np.zeros((n, 9), np.uint32)
    root = np.zeros((n, 32), np.uint8)
    ws = np.zeros(n, np.uint8)
    L.vss_sqrt(signed, with_inv, _p(num), _p(den), n_(n), _p(canon), _p(root), _p(ws))
    return canon, root, ws


def test_signed_sqrt_equals_unsigned_and_model(vss, model, kats):
    """Root and flag of the fes instantiation equal the fe instantiation's, limb for limb in canonical form, in the form
    with the batched inverse (k_scalar_mul_var's) and in the inversion-free one; both are the Python model's."""
    rows, num, den = _sqrt_inputs(kats)
    assert len(rows) == N_SQRT
    want = [model.sqrt_ratio_zeta(a, b) for a, b in rows]
    want_ws = np.array([1 if w else 0 for w, _ in want], np.uint8)
    want_root = np.stack([_le(r) for _, r in want])
    assert 300 < int(want_ws.sum()) < 800                     # squares and non-squares, plenty of both
    for with_inv in (1, 0):
        cu, ru, wu = _run_sqrt(vss, 0, with_inv, num, den)
        cs, rs, wss = _run_sqrt(vss, 1, with_inv, num, den)
        assert (cs == cu).all() and (wss == wu).all() and (rs == ru).all()
        assert (wss == want_ws).all() and (rs == want_root).all()
    # den = 0: (false, 0) whatever num is, unless num = 0 too (true, 0): the reference's early-outs
    for i, (a, b) in enumerate(rows[:15]):
        if b % Q == 0 or a % Q == 0:
            assert not rs[i].any() and wss[i] == (1 if a % Q == 0 else 0)


def _encodings(oracle, rng, n):
    enc = oracle.encode_to_curve(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    enc[0] = 0                                           # the identity
    enc[1] = 0xFF                                        # not a field element
    enc[2, 0] |= 1                                       # a negative s
    enc[3] = enc[4]
    enc[3, 5] ^= 0x40                                    # (almost surely) not on the curve
    return enc


def test_signed_decompression_equals_unsigned(vss, oracle):
    """ge_decompress<fes> (k_scalar_mul_var) gives the records and statuses of ge_decompress<fe> (every other kernel)."""
    enc = _encodings(oracle, np.random.default_rng(5), 64)
    res = []
    for signed in (0, 1):
        xyzt, st = np.zeros((64, 16), np.uint64), np.zeros(64, np.uint8)
        vss.vss_decompress(signed, _p(enc), n_(64), _p(xyzt), _p(st))
        res.append((xyzt, st))
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert res[1][1][0] == 0 and res[1][1][1] != 0 and res[1][1][2] != 0 and res[1][1][3] != 0


def _special_scalars():
    h8 = 16 ** 62 - 8 * (16 ** 62 - 1) // 15              # window digits: 1, then -8 sixty-two times
    return [0, 1, R_ORDER - 1, R_ORDER, (1 << 256) - 1,
            2 * R_ORDER,                                   # k / 2 mod r = 0 again: every window of the recoding zero
            (2 * h8) % R_ORDER, h8,                        # all -8: for the chain that halves (k = 2h) and the one that does not
            (2 * (7 * (16 ** 62 - 1) // 15)) % R_ORDER,    # all 7
            2, R_ORDER - 2, R_ORDER + 1, (R_ORDER + 1) // 2, (R_ORDER - 1) // 2, 16 ** 62, 2 * 16 ** 62 % R_ORDER]


def test_scalar_mul_through_shared_identity_table(vss, oracle):
    """256 (encoding, scalar) pairs through the signed square root and a table that is never handed entry 0: the oracle's
    bytes and statuses, and not one store(0)."""
    rng = np.random.default_rng(377)
    n = 256
    enc = _encodings(oracle, rng, n)
    k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sp = _special_scalars()
    for j, v in enumerate(sp):
        k[8 + j] = _le(v)                                  # on valid random points
        k[n - 1 - j] = _le(v)
    k[0] = _le(sp[6])                                      # the identity times the all -8 scalar
    enc[n - 1] = 0                                         # and the identity times 0
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert vss.vss_scalar_mul_var(_p(enc), _p(k), n_(n), _p(out), _p(st)) == 0
    oo, so = oracle.scalar_mul_var(enc, k)
    assert (out == oo).all() and (st == so).all()
    assert st[1] != 0 and st[0] == 0 and not out[8].any()           # [0]P: the identity's all-zero encoding
    out2, st2 = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert vss.vss_scalar_mul_var_el(_p(enc), _p(k), n_(n), _p(out2), _p(st2)) == 0
    assert (out2 == oo).all() and (st2 == so).all()


def test_signed_sqrt_bounds(kats, tmp_path):
    """The -DD377_BOUNDS build runs the fes square root over the same 2^10 inputs (edge vectors, den = 0, squares and
    non-squares), both forms, then decompression and the scalar multiplication through the shared-identity table (the table
    entries' y + x left uncarried): a violated precondition aborts."""
    lib = _build("libd377_vb_signed_sqrt_sim_bounds.so", ["-O1", "-g", "-DD377_BOUNDS", "-DD377_FB_BITS=8"])
    _, num, den = _sqrt_inputs(kats)
    work = str(tmp_path / "sqrt_inputs.npz")
    np.savez(work, num=num, den=den)
    code = r"""
import ctypes, sys, numpy as np
L = ctypes.CDLL(sys.argv[1]); L.sim_init.restype = ctypes.c_int; assert L.sim_init() == 0
L.vss_scalar_mul_var.restype = ctypes.c_ulong
p = lambda a: a.ctypes.data_as(ctypes.c_void_p); n_ = ctypes.c_size_t
z = np.load(sys.argv[2]); num = np.ascontiguousarray(z["num"]); den = np.ascontiguousarray(z["den"]); n = len(num)
canon = np.zeros((n, 9), np.uint32); root = np.zeros((n, 32), np.uint8); ws = np.zeros(n, np.uint8)
L.vss_sqrt(1, 1, p(num), p(den), n_(n), p(canon), p(root), p(ws)); print(int(ws.sum()))
L.vss_sqrt(1, 0, p(num), p(den), n_(256), p(canon), p(root), p(ws))
rng = np.random.default_rng(1); m = 24
r0 = rng.integers(0, 256, (m, 32), dtype=np.uint8); k = rng.integers(0, 256, (m, 32), dtype=np.uint8)
enc = np.zeros((m, 32), np.uint8); out = np.zeros((m, 32), np.uint8); st = np.zeros(m, np.uint8); xyzt = np.zeros((m, 16), np.uint64)
L.sim_encode_to_curve(p(r0), n_(m), p(enc), None)
enc[0] = 0; enc[1] = 0xFF; k[2] = 0; k[3] = 0xFF
L.vss_decompress(1, p(enc), n_(m), p(xyzt), p(st))
assert L.vss_scalar_mul_var(p(enc), p(k), n_(m), p(out), p(st)) == 0
L.vss_scalar_mul_var_el(p(enc), p(k), n_(4), p(out), p(st))
"""
    res = subprocess.run([sys.executable, "-c", code, lib, work], capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, res.stderr[-3000:]
    assert 300 < int(res.stdout.split()[0]) < 800
