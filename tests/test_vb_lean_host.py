"""CPU check of the chain k_scalar_mul_var / k_scalar_mul_var_el run: ge_scalar_mul_w4_lean (curve.hpp) -- 62 windows from
a start value [d62]P lifted from table entry d62, and doublings that take 2XY from a squaring (ge_double_neg_sq).

tests/host_sim/vb_lean_sim.cpp is compiled for the host with g++.  The lean chain, the reference statement
ge_scalar_mul_w4<fes> and the oracle must agree byte for byte over both compressors, three host tables (limbs with an own
entry 0, limbs with the shared identity, packed 256-bit slots), want_t true and false, and Elements with Z != 1; the
-DD377_BOUNDS build walks the lean chain with every precondition asserted (each column of each signed product inside
+-2^63, digit 63 zero and digit 62 in 0..5) and counts its field products; tests/cpp/vb_lean_chain.cpp runs it under
AddressSanitizer and UndefinedBehaviorSanitizer as an ordinary program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from _vb_lean_cases import le as _le, special_points, special_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
PROG = os.path.join(ROOT, "tests", "cpp", "vb_lean_chain.cpp")
N = 1 << 10
TABLES = (0, 1, 2)                                        # limbs + own entry 0, limbs + shared identity, packed slots
# field products per element of k_scalar_mul_var's lane with the lean chain; the reference
# statement's are bench.py's KERNEL_OPS: 1668.5 M + 1009 S
LEAN_OPS = (1396.5, 1245.0)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def n_(n):
    return ctypes.c_size_t(n)


def _sources():
    return [os.path.join(SIM_DIR, f) for f in ("vb_lean_sim.cpp", "vb_signed_sqrt_sim.cpp", "sim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC)]


def _stale(target, srcs):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def _build(name, flags):
    lib = os.path.join(SIM_DIR, name)
    if _stale(lib, _sources()):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC] + flags +
                              [os.path.join(SIM_DIR, "vb_lean_sim.cpp"), "-o", lib])
    return lib


@pytest.fixture(scope="module")
def vbl():
    L = ctypes.CDLL(_build("libd377_vb_lean_sim.so", ["-O2", "-DD377_FB_BITS=12"]))
    L.sim_init.restype = ctypes.c_int
    for f in ("vbl_scalar_mul_var", "vbl_scalar_mul_var_sqrt", "vbl_scalar_mul_var_el"):
        getattr(L, f).restype = ctypes.c_ulong
    assert L.sim_init() == 0
    return L


@pytest.fixture(scope="module")
def case(oracle):
    """2^10 seeded (encoding, scalar) pairs with the special scalars and points, and the oracle's answers, computed once"""
    rng = np.random.default_rng(62377)
    valid = oracle.encode_to_curve(rng.integers(0, 256, (N, 32), dtype=np.uint8))
    enc = valid.copy()
    k = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    sp = special_scalars()
    pts = special_points(oracle, valid)
    for j, v in enumerate(sp):
        k[8 + j] = _le(v)                                  # on valid random points
        k[N - 1 - j] = _le(v)
        enc[N - 1 - j] = pts[j % 4]                        # and on the special points, each point under several scalars
    enc[:4] = pts                                          # the special points under random scalars
    enc[4] = 0
    k[4] = 0                                               # the identity times 0
    out, st = oracle.scalar_mul_var(enc, k)
    xyzt, st_d = oracle.decompress(valid)
    assert not st_d.any()
    el_in = oracle.scalar_mul_xyzt(xyzt, rng.integers(0, 256, (N, 32), dtype=np.uint8))    # Elements with Z != 1
    assert (el_in[:, 8:12] != oracle.identity_xyzt().reshape(-1, 16)[:, 8:12]).any(axis=1).all()
    el_out = oracle.compress(oracle.scalar_mul_xyzt(el_in, k))
    return {"enc": enc, "k": k, "out": out, "st": st, "el_in": np.ascontiguousarray(el_in), "el_out": el_out}


def test_top_digits_of_every_input(vbl, case):
    """digit 63 is 0 and digit 62 lies in 0..5 on every scalar the tests use, in both forms (k / 2 mod r and k mod r), and each
    of the six top digits occurs in both"""
    k = case["k"]
    for halve in (1, 0):
        d62, d63 = np.zeros(N, np.int8), np.full(N, 99, np.int8)
        vbl.vbl_top_digits(halve, _p(k), n_(N), _p(d62), _p(d63))
        assert not d63.any()
        assert set(int(x) for x in d62) == set(range(6)), (halve, sorted(set(int(x) for x in d62)))


def test_special_points_are_what_they_claim(case):
    st, out = case["st"], case["out"]
    assert st[0] == 0 and st[1] != 0 and st[2] != 0 and st[3] != 0 and st[4] == 0 and not out[4].any()
    assert not out[st != 0].any()                          # rejected rows are all-zero
    assert 0 < int((st != 0).sum()) < N // 8


@pytest.mark.parametrize("table", TABLES)
def test_lane_form_parity(vbl, case, table):
    """k_scalar_mul_var's lane (signed square root, k / 2 mod r, the compressor without a square root): lean chain =
    reference statement = oracle, bytes and statuses, for want_t false and true"""
    for chain in (1, 0):
        for want_t in (0, 1):
            out, st = np.full((N, 32), 0xA5, np.uint8), np.full(N, 0xA5, np.uint8)
            s0 = vbl.vbl_scalar_mul_var(chain, table, want_t, _p(case["enc"]), _p(case["k"]), n_(N), _p(out), _p(st))
            assert (st == case["st"]).all(), (chain, table, want_t)
            assert (out == case["out"]).all(), (chain, table, want_t)
            assert not out[st != 0].any()
            assert table == 0 or s0 == 0


@pytest.mark.parametrize("table", TABLES)
def test_sqrt_compressor_and_element_parity(vbl, case, table):
    """the chain on the scalar itself with T wanted, through the square-root compressor: from encodings, and from Elements
    with Z != 1 (k_scalar_mul_var_el's inputs)"""
    for chain in (1, 0):
        out, st = np.full((N, 32), 0xA5, np.uint8), np.full(N, 0xA5, np.uint8)
        s0 = vbl.vbl_scalar_mul_var_sqrt(chain, table, _p(case["enc"]), _p(case["k"]), n_(N), _p(out), _p(st))
        assert (st == case["st"]).all() and (out == case["out"]).all(), (chain, table)
        el = np.full((N, 32), 0xA5, np.uint8)
        s0 += vbl.vbl_scalar_mul_var_el(chain, table, _p(case["el_in"]), _p(case["k"]), n_(N), _p(el))
        assert (el == case["el_out"]).all(), (chain, table)
        assert table == 0 or s0 == 0


def test_lean_chain_bounds_and_counts(case, tmp_path):
    """-DD377_BOUNDS: a violated precondition aborts.  32 random elements of the lane form (a lane's rounds of 8) give the
    product counts; then the special scalars and points, the other tables, the square-root compressor and Elements with
    Z != 1 are walked too."""
    lib = _build("libd377_vb_lean_sim_bounds.so", ["-O1", "-g", "-DD377_BOUNDS", "-DD377_FB_BITS=8"])
    sp = special_scalars()
    m = len(sp)
    work = str(tmp_path / "lean_inputs.npz")
    np.savez(work, enc=case["enc"][N - m:], k=case["k"][N - m:], enc_v=case["enc"][8:8 + m], k_v=case["k"][8:8 + m],
             el_in=case["el_in"][N - m:])
    code = r"""
import ctypes, sys, numpy as np
L = ctypes.CDLL(sys.argv[1]); L.sim_init.restype = ctypes.c_int; assert L.sim_init() == 0
p = lambda a: a.ctypes.data_as(ctypes.c_void_p); n_ = ctypes.c_size_t
rng = np.random.default_rng(1); mm = ctypes.c_ulong(); ss = ctypes.c_ulong()
n = 32
r0 = rng.integers(0, 256, (n, 32), dtype=np.uint8); k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
enc = np.zeros((n, 32), np.uint8); out = np.zeros((n, 32), np.uint8); st = np.zeros(n, np.uint8)
L.sim_encode_to_curve(p(r0), n_(n), p(enc), None); L.sim_op_counts(ctypes.byref(mm), ctypes.byref(ss))
L.vbl_scalar_mul_var(1, 2, 0, p(enc), p(k), n_(n), p(out), p(st))
L.sim_op_counts(ctypes.byref(mm), ctypes.byref(ss)); print(mm.value / n, ss.value / n)
z = np.load(sys.argv[2]); g = lambda s: np.ascontiguousarray(z[s])
m = len(z["k"]); out = np.zeros((m, 32), np.uint8); st = np.zeros(m, np.uint8)
L.vbl_scalar_mul_var(1, 2, 0, p(g("enc")), p(g("k")), n_(m), p(out), p(st))          # special scalars on special points
for table in (2, 1, 0):
    L.vbl_scalar_mul_var(1, table, 1, p(g("enc_v")), p(g("k_v")), n_(m), p(out), p(st))   # ... on valid points
L.vbl_scalar_mul_var_sqrt(1, 2, p(g("enc_v")), p(g("k_v")), n_(m), p(out), p(st))
L.vbl_scalar_mul_var_el(1, 2, p(g("el_in")), p(g("k")), n_(m), p(out))
L.vbl_scalar_mul_var_el(1, 0, p(g("el_in")), p(g("k")), n_(8), p(out))
print("walked")
"""
    res = subprocess.run([sys.executable, "-c", code, lib, work], capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, res.stderr[-3000:]
    f = res.stdout.split()
    print("lean chain, products per element: %s M + %s S" % (f[0], f[1]))
    assert f[2] == "walked"
    assert (float(f[0]), float(f[1])) == LEAN_OPS
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        assert "1396.5 M + 1245 S" in fh.read()            # the numbers this test pins are the ones the design states


def test_sanitized_program_runs_clean(case):
    """tests/cpp/vb_lean_chain.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain executable: the special
    scalars on valid and on special points, both chains over the three tables; its output is the oracle's"""
    exe = os.path.join(ROOT, "build", "tests", "vb_lean_chain_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if _stale(exe, _sources() + [PROG]):
        subprocess.check_call(["g++", "-std=c++17", "-I" + CSRC, "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-DD377_HOST_OUTLINE", "-DD377_FB_BITS=8", PROG, "-o", exe])
    m = len(special_scalars())
    idx = list(range(0, 8 + m, 3)) + list(range(N - m, N, 2))
    lines = ["S %s %s\n" % (bytes(case["enc"][i]).hex(), bytes(case["k"][i]).hex()) for i in idx]
    res = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.returncode, res.stderr[-3000:])
    out = res.stdout.split("\n")
    assert out[-2] == "OK" and len(out) == len(idx) + 2
    for i, line in zip(idx, out):
        f = line.split()
        want = bytes(case["out"][i]).hex()
        assert f[0] == "S" and f[1] == want and f[3] == want, (i, line)
        assert (int(f[2]) != 0) == (int(f[4]) != 0) == (case["st"][i] != 0), (i, line)
