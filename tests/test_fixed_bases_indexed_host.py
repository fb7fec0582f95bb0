"""Fixed-base sums whose terms name their bases (d377_batch_fixed_msm_indexed) without a GPU.

The indexed walk the lane kernel runs (curve.hpp: ge_fixed_msm_indexed_w8, with the kernel's own term loader) is compiled for
the host (tests/host_sim/fixed_bases_indexed_sim.cpp) and checked, byte for byte, against the oracle's fold of scalar
multiplications and additions, and against the dense host walk on the index row 0 .. m-1.  The ABI checks need no device
either: the symbol is declared, exported and bound, it is no `_dev` entry point, and bad arguments are refused in the
documented order before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _sums_support import (R, _p, host_bases as _bases, host_scalars as _scalars, indexed_fold_by_scalar_mul as _fold,
                           scalar_bytes as _scalar_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAME = "d377_batch_fixed_msm_indexed"
M = 5
N = 40


@pytest.fixture(scope="module")
def fxi():
    lib = os.path.join(SIM_DIR, "libd377_fxi_sim.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("fixed_bases_indexed_sim.cpp", "fixed_bases_sim.cpp", "sim.cpp")]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "fixed_bases_indexed_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.fx_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fx_msm.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.fx_msm_indexed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


@pytest.fixture(scope="module")
def bases(oracle):
    """The same five bases for every case: a random point, the identity, GENERATOR, Z != 1, the torsion twin."""
    return _bases(oracle, np.random.default_rng(55), M)


def _rows(rng, n, t, m, k):
    """n x t index rows, random with the planted ones; writes the scalars of the cancelling row into k ([n * t, 32]).
    Returns (index rows, the row of all -1, the row that sums to the identity or None)."""
    idx = rng.integers(0, m, (n, t)).astype(np.int32)
    idx[0] = m - 1                                               # every term the last base
    idx[1] = -1                                                  # no term at all
    idx[2] = 1 % m                                               # one index repeated
    cancel = None
    if t >= 2:                                                   # a twice, with k and r - k: the identity
        cancel, a = 3, m - 1
        idx[3] = -1
        idx[3, 0] = idx[3, t - 1] = a
        kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
        k[3 * t] = _scalar_bytes(kv)
        k[3 * t + t - 1] = _scalar_bytes(R - kv)
    idx[4, 0] = -1                                               # absent first, middle, last
    idx[5, t // 2] = -1
    idx[6, t - 1] = -1
    return idx, 1, cancel


@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("t", [1, 2, 3, 7])
def test_indexed_walk_matches_oracle_fold(fxi, oracle, bases, bits, t):
    rng = np.random.default_rng(1000 * bits + t)
    k = _scalars(rng, N, t)                                      # 0, 1, r - 1, r and 2^256 - 1 among them
    idx, absent, cancel = _rows(rng, N, t, M, k)
    assert fxi.fx_build(_p(bases), M, bits) == 0
    enc = np.full((N, 32), 0xA5, np.uint8)
    el = np.zeros((N, 16), np.uint64)
    assert fxi.fx_msm_indexed(_p(idx), _p(k), t, N, _p(enc), _p(el)) == 0
    want_enc, want_el = _fold(oracle, bases, idx, k)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    assert not enc[absent].any() and oracle.is_identity(el[absent:absent + 1]).all()
    if cancel is not None:
        assert not enc[cancel].any() and oracle.is_identity(el[cancel:cancel + 1]).all()


@pytest.mark.parametrize("bits", [8, 12])
def test_indexed_walk_in_registration_order_is_the_dense_walk(fxi, oracle, bases, bits):
    rng = np.random.default_rng(bits)
    k = _scalars(rng, N, M)
    idx = np.ascontiguousarray(np.tile(np.arange(M, dtype=np.int32), (N, 1)))
    assert fxi.fx_build(_p(bases), M, bits) == 0
    enc_d, el_d = np.zeros((N, 32), np.uint8), np.zeros((N, 16), np.uint64)
    enc_i, el_i = np.ones((N, 32), np.uint8), np.ones((N, 16), np.uint64)
    assert fxi.fx_msm(_p(k), N, _p(enc_d), _p(el_d)) == 0
    assert fxi.fx_msm_indexed(_p(idx), _p(k), M, N, _p(enc_i), _p(el_i)) == 0
    assert (enc_i == enc_d).all()
    assert (el_i == el_d).all()                                  # the same additions in the same order: the same limbs


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert re.search(r"\b%s\(" % NAME, header)
    assert NAME in exported
    assert NAME in _native.EXPORTS
    assert not NAME.endswith("_dev")
    assert len(getattr(_native.load(), NAME).argtypes) == 8


def test_refuses_bad_arguments_without_a_device_in_order(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    f = getattr(lib, NAME)
    idx = np.zeros((2, 2), np.int32)
    k = np.zeros((4, 32), np.uint8)
    enc = np.full((2, 32), 0xA5, np.uint8)
    err = lambda: lib.d377_last_error().decode()
    for t in (0, 65):                                            # t first: everything else is bad as well
        assert f(None, 1, None, None, t, 2, None, None) == -2
        assert re.search(r"\bt\b", err())
    assert f(None, 1, None, _p(k), 2, 2, _p(enc), None) == -2
    assert "base_index" in err()
    assert f(None, 1, _p(idx), None, 2, 2, _p(enc), None) == -2
    assert "scalar32" in err()
    assert f(None, 1, _p(idx), _p(k), 2, 2, None, None) == -2
    assert "enc32_out" in err()
    assert f(None, 1, _p(idx), _p(k), 2, 2, _p(enc), None) == -2
    assert "ctx" in err()
    assert f(None, 1, None, None, 2, 0, None, None) == -2        # n = 0 excuses the null buffers, not the null context
    assert "ctx" in err()
    assert (enc == 0xA5).all()
