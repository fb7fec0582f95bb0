"""Many multiscalar sums of 9 .. 4096 terms (d377_batch_msm_long) without a GPU.

The plan (decaf377_amd/csrc/batch_msm_long_plan.hpp) is checked for every m, and the walk the device runs -- groups of at most
8 terms as Straus chains with dead padded slots, partial sums as Element records, fold levels of 16 records per lane, the
chunked compressor -- is compiled for the host (tests/host_sim/batch_msm_long_sim.cpp) and checked, byte for byte, against the
oracle's fold of scalar multiplications and additions.  The ABI checks need no device either: both symbols are declared,
exported and bound, neither is a `_dev` entry point, and bad arguments are refused in the documented order before any device
is touched.

The case builder and the oracle's fold are in tests/_batch_msm_long_cases.py, shared with tests/test_batch_msm_long_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _batch_msm_long_cases import make_case, oracle_fold, plan
from _oracle import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAMES = ("d377_batch_msm_long", "d377_batch_msm_long_encoded")
FOLD = 16
# (m, n): 9 = g 2, b 5, one padded slot; 16 = exact groups; 17 = g 3, b 6; 129 = g 17, the second fold level at 16 records per
# lane; 2049 = g 257, the third
CASES = [(9, 7), (16, 7), (17, 7), (64, 7), (65, 7), (129, 2), (2049, 1)]


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libd377_bml_sim.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("batch_msm_long_sim.cpp", "sim.cpp")]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "batch_msm_long_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.sim_init.restype = ctypes.c_int
    L.sim_init()
    L.bml_plan.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    L.bml_levels.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    L.bml_msm_long.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


def test_plan_properties_for_every_m(sim):
    assert sim.bml_fold() == FOLD
    out = np.zeros(2 + 2 * 512, np.uint64)
    for m in range(9, 4097):
        sim.bml_plan(m, _p(out))
        g, b = int(out[0]), int(out[1])
        assert (g, b) == plan(m)
        first, count = out[2:2 + 2 * g:2].astype(np.int64), out[3:3 + 2 * g:2].astype(np.int64)
        assert b <= 8 and g * b - m < g
        assert (count >= 1).all() and (count <= b).all()                           # no group is empty
        assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == m   # they tile [0, m)
        assert (first == np.arange(g) * b).all()
    sim.bml_plan(9, _p(out))
    assert list(out[:6].astype(int)) == [2, 5, 0, 5, 5, 4]                         # two chains of 5 and 4 terms, not 8 and 1


def test_fold_levels(sim):
    lv = np.zeros(8, np.uint64)
    for g, want in ((2, [1]), (16, [1]), (17, [2, 1]), (256, [16, 1]), (257, [17, 2, 1]), (512, [32, 2, 1])):
        assert sim.bml_levels(g, _p(lv)) == len(want) and list(lv[:len(want)].astype(int)) == want
    assert plan(129)[0] == 17 and plan(128)[0] == 16                               # the smallest m with a second level
    assert plan(2049)[0] == 257 and plan(2048)[0] == 256                           # ... and with a third


@pytest.mark.parametrize("m,n", CASES)
def test_walk_matches_oracle_fold(sim, oracle, m, n):
    rng = np.random.default_rng(m)
    pts, k, info = make_case(oracle, rng, n, m)
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    touched = np.zeros(n * m, np.uint8)
    assert sim.bml_msm_long(0, _p(pts), _p(k), m, n, _p(enc), _p(el), None, _p(touched)) == 0
    assert (touched == 1).all()                                  # every term read once; the dead padded slots read nothing
    want_enc, want_el, _ = oracle_fold(oracle, pts, k, m)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    for s in info["identity"]:
        assert not enc[s].any() and oracle.is_identity(el[s:s + 1]).all()


@pytest.mark.parametrize("m,n", [(9, 7), (17, 7), (129, 2)])
def test_walk_on_encodings_reports_invalid_ones(sim, oracle, m, n):
    rng = np.random.default_rng(1000 + m)
    raw, k, info = make_case(oracle, rng, n, m, encoded=True)
    g, b = plan(m)
    assert g * b == m or info["dead"][m - 1]                     # an invalid Encoding in a padded last group
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    st = np.full(n * m, 0xEE, np.uint8)
    assert sim.bml_msm_long(1, _p(raw), _p(k), m, n, _p(enc), _p(el), _p(st), None) == 0
    want_enc, want_el, want_st = oracle_fold(oracle, raw, k, m)
    assert ((want_st != 0) == info["dead"]).all()
    assert (st == want_st).all()
    assert (enc == want_enc).all()
    assert oracle.eq_xyzt(el, want_el).all()


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    lib = _native.load()
    for name, nargs in zip(NAMES, (7, 8)):
        assert re.search(r"\b%s\(" % name, header)
        assert name in exported
        assert name in _native.EXPORTS
        assert not name.endswith("_dev")
        assert len(getattr(lib, name).argtypes) == nargs
    assert re.search(r"#define D377_BATCH_MSM_LONG_MAX_TERMS 4096\b", header)
    assert not [s for s in exported if "msm_long" in s and s not in NAMES]          # no device-pointer form under any name


def test_refuses_bad_arguments_without_a_device_in_order(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    pts = np.zeros((18, 16), np.uint64)
    raw = np.zeros((18, 32), np.uint8)
    k = np.zeros((18, 32), np.uint8)
    enc = np.full((2, 32), 0xA5, np.uint8)
    st = np.full(18, 0xA5, np.uint8)
    err = lambda: lib.d377_last_error().decode()
    el, en = lib.d377_batch_msm_long, lib.d377_batch_msm_long_encoded
    for m in (0, 4097):                                          # m first: a null context and null buffers alike
        assert el(None, None, None, m, 2, None, None) == -2
        assert re.search(r"\bm = %d\b" % m, err()) and "d377_msm" in err()
        assert en(None, None, None, m, 2, None, None, None) == -2
        assert re.search(r"\bm = %d\b" % m, err())
        assert el(None, _p(pts), _p(k), m, 2, _p(enc), None) == -2
        assert re.search(r"\bm = %d\b" % m, err())
        assert el(None, None, None, m, 0, None, None) == -2      # ... and with n = 0
        assert re.search(r"\bm = %d\b" % m, err())
    for m in (9, 3):                                             # then the buffers, then the context
        assert el(None, None, _p(k), m, 2, _p(enc), None) == -2 and "xyzt" in err()
        assert el(None, _p(pts), None, m, 2, _p(enc), None) == -2 and "scalar32" in err()
        assert el(None, _p(pts), _p(k), m, 2, None, None) == -2 and "enc32_out" in err()
        assert en(None, None, _p(k), m, 2, _p(enc), None, _p(st)) == -2 and "enc32" in err()
        assert en(None, _p(raw), _p(k), m, 2, _p(enc), None, None) == -2 and "status" in err()
        assert el(None, _p(pts), _p(k), m, 2, _p(enc), None) == -2 and "ctx" in err()
        assert en(None, _p(raw), _p(k), m, 2, _p(enc), None, _p(st)) == -2 and "ctx" in err()
        assert el(None, None, None, m, 0, None, None) == -2 and "ctx" in err()     # n = 0 excuses the null buffers, not the null context
    assert (enc == 0xA5).all() and (st == 0xA5).all()
