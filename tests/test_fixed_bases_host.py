"""Fixed-base combs for caller-chosen points (d377_fixed_bases_create / d377_batch_fixed_msm) without a GPU.

The multi-comb walk the lane kernel runs (curve.hpp: ge_fixed_msm_w8) is compiled for the host together with the
square-root-free compressor (tests/host_sim/fixed_bases_sim.cpp) and checked, byte for byte, against the oracle's fold of
scalar multiplications and additions.  The ABI checks here need no device either: the new symbols are declared, exported and
bound, none of them is a `_dev` entry point, and bad arguments are refused before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _sums_support import _p, host_bases as _bases, host_scalars as _scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NEW_SYMBOLS = ["d377_fixed_bases_create", "d377_fixed_bases_info", "d377_fixed_bases_destroy", "d377_batch_fixed_msm"]


@pytest.fixture(scope="module")
def fx():
    lib = os.path.join(SIM_DIR, "libd377_fx_sim.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("fixed_bases_sim.cpp", "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "fixed_bases_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.fx_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fx_msm.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


def _fold(oracle, bases, k, n, m):
    """The oracle's sums: sum_j k[i m + j] * B_j by scalar multiplications and additions -> (encodings, records)."""
    terms = oracle.scalar_mul_xyzt(np.tile(bases, (n, 1)), k).reshape(n, m, 16)
    acc = np.ascontiguousarray(terms[:, 0])
    for j in range(1, m):
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(terms[:, j]))
    return oracle.compress(acc), acc


@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_walk_matches_oracle_fold(fx, oracle, bits, m):
    rng = np.random.default_rng(1000 * bits + m)
    bases = _bases(oracle, rng, m)
    n = 40
    k = _scalars(rng, n, m)
    assert fx.fx_build(_p(bases), m, bits) == 0
    enc = np.zeros((n, 32), np.uint8)
    el = np.zeros((n, 16), np.uint64)
    assert fx.fx_msm(_p(k), n, _p(enc), _p(el)) == 0
    want_enc, want_el = _fold(oracle, bases, k, n, m)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()


def test_generator_comb_is_the_context_comb(fx, oracle):
    """[GENERATOR] as a registered base gives what the oracle's fixed-base multiplication gives."""
    rng = np.random.default_rng(5)
    g = oracle.generator_xyzt().reshape(1, 16)
    k = _scalars(rng, 64, 1)
    assert fx.fx_build(_p(g), 1, 12) == 0
    enc = np.zeros((64, 32), np.uint8)
    assert fx.fx_msm(_p(k), 64, _p(enc), None) == 0
    assert (enc == oracle.scalar_mul_base(k)).all()


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert re.search(r"#define D377_FIXED_BASES_MAX 64\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert name in _native.EXPORTS, name
        assert not name.endswith("_dev")
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes, name                 # bound with argument types, not called blindly


def test_no_new_dev_export():
    """The fixed-base sums have no device-pointer entry point: every `_dev` export of the binding predates them."""
    from decaf377_amd import _native
    assert not [n for n in _native.EXPORTS if "fixed" in n and n.endswith("_dev")]


@pytest.mark.parametrize("m,bits,word", [(0, 16, "m"), (65, 16, "m"), (1, 7, "comb_bits"), (2, 14, "comb_bits"),
                                         (3, 23, "comb_bits"), (1, -1, "comb_bits")])
def test_create_refuses_bad_arguments_without_a_device(libpath, m, bits, word):
    from decaf377_amd import _native
    lib = _native.load()
    rec = np.zeros((max(m, 1), 16), np.uint64)
    h = ctypes.c_int64(-1)
    rc = lib.d377_fixed_bases_create(None, _p(rec), m, bits, ctypes.byref(h))
    assert rc == -2                                               # D377_ERR_ARG
    assert not h.value
    assert re.search(r"\b%s\b" % word, lib.d377_last_error().decode())


def test_create_refuses_null_pointers_without_a_device(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    rec = np.zeros((1, 16), np.uint64)
    h = ctypes.c_int64(0)
    assert lib.d377_fixed_bases_create(None, None, 1, 16, ctypes.byref(h)) == -2
    assert "xyzt" in lib.d377_last_error().decode()
    assert lib.d377_fixed_bases_create(None, _p(rec), 1, 16, None) == -2
    assert "handle_out" in lib.d377_last_error().decode()
    assert lib.d377_fixed_bases_create(None, _p(rec), 1, 0, ctypes.byref(h)) == -2
    assert "ctx" in lib.d377_last_error().decode()
    assert lib.d377_batch_fixed_msm(None, 1, None, 0, None, None) == -2
    assert lib.d377_fixed_bases_info(None, 1, None, None, None) == -2
    assert lib.d377_fixed_bases_destroy(None, 1) == -2
