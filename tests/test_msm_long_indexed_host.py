"""The long sums on device buffers and over a pool of points (include/decaf377_amd_long_sums.h), without a GPU.

The walk the device runs for d377_batch_long_msm_indexed -- the cut of batch_msm_long_plan.hpp for any m, every slot classified
by batch_msm_long_indexed_plan.hpp (the kernels' own function), live slots gathering their record from the pool -- is compiled
for the host (tests/host_sim/batch_msm_long_indexed_sim.cpp) and checked, byte for byte, against the oracle's fold on the
materialised gather, absent terms as Z = 0 records.  The ABI checks need no device either: the four symbols are declared by
their header, defined, bound and in rust/src/ffi_long_sums.rs, and bad arguments are refused in the documented order before
any device is touched.

The case builder is tests/_msm_long_indexed_cases.py, shared with tests/test_msm_long_resident_gpu.py."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from _batch_msm_long_cases import oracle_fold, plan
from _msm_long_indexed_cases import DEAD_RECORD, POOL, make_indexed, make_pool, materialise
from _oracle import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAMES = {"d377_batch_long_msm_resident": 9, "d377_batch_long_msm_encoded_resident": 10, "d377_batch_long_msm_indexed": 9,
         "d377_batch_long_msm_indexed_resident": 12}
# (m, n): 1 and 8 = one chain per sum, no fold level; 9 = g 2 with a padded slot; 17 = g 3; 129 = g 17, two fold levels;
# 4096 = g 512, three
CASES = [(1, 3), (8, 3), (9, 3), (17, 3), (129, 3), (4096, 1)]
ERR_ARG = -2


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libd377_bmli_sim.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("batch_msm_long_indexed_sim.cpp", "sim.cpp")]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "batch_msm_long_indexed_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.sim_init.restype = ctypes.c_int
    L.sim_init()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bmli_slots.argtypes = [sz, sz, vp, ctypes.c_uint32, vp, vp]
    L.bmli_slots.restype = None
    L.bmli_msm.argtypes = [vp, ctypes.c_uint32, vp, vp, sz, sz, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


@pytest.mark.parametrize("m", [1, 5, 8, 9, 17, 129])
def test_slot_classification_against_numpy(sim, m):
    """Every slot of every chain: past the end where the cut pads the last group, absent for -1 and for every other index
    outside the pool (both ends of int among them), live with the named record otherwise."""
    n = 4
    g, b = plan(m) if m > 8 else (1, m)
    rng = np.random.default_rng(m)
    idx = rng.integers(-1, POOL, (n, m)).astype(np.int32)
    edge = [-(1 << 31), -2, -1, 0, POOL - 1, POOL, (1 << 31) - 1]
    flat = idx.reshape(-1)
    flat[:min(len(edge), len(flat))] = edge[:len(flat)]
    kind = np.full(n * g * b, 9, np.int32)
    rec = np.full(n * g * b, 9, np.int64)
    sim.bmli_slots(m, n, _p(idx), POOL, _p(kind), _p(rec))
    kind, rec = kind.reshape(n, g * b), rec.reshape(n, g * b)
    assert (kind[:, m:] == 0).all() and (rec[:, m:] == -1).all()               # past the end: g b - m slots per sum
    live = (idx >= 0) & (idx < POOL)
    assert (kind[:, :m] == np.where(live, 2, 1)).all()
    assert (rec[:, :m] == np.where(live, idx, -1)).all()


@pytest.mark.parametrize("m,n", CASES)
def test_gathered_walk_matches_oracle_fold(sim, oracle, m, n):
    rng = np.random.default_rng(4000 + m)
    pool = make_pool(oracle, rng)
    idx, k, info = make_indexed(rng, n, m)
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    pool_touched = np.zeros(POOL, np.uint32)
    scalar_touched = np.zeros(n * m, np.uint8)
    assert sim.bmli_msm(_p(pool), POOL, _p(idx), _p(k), m, n, _p(enc), _p(el), _p(pool_touched), _p(scalar_touched)) == 0
    flat = idx.reshape(-1)
    assert (scalar_touched == (flat != -1)).all()                              # an absent term reads no scalar ...
    assert (pool_touched == np.bincount(flat[flat != -1], minlength=POOL)).all()   # ... and no point; a live one reads its own, once
    want_enc, want_el, _ = oracle_fold(oracle, materialise(pool, idx), k, m)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    for s in info["identity"]:
        assert not enc[s].any() and oracle.is_identity(el[s:s + 1]).all()
    if m > 1:
        assert info["absent"][0, m - 1] and enc[0].any()
    assert 0 in flat and POOL - 1 in flat
    assert len(flat) < 5 or DEAD_RECORD in flat


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_defined_bound_and_in_the_rust_block(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd_long_sums.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.LONG_SUMS_EXPORTS)
    main = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert main.index('#include "decaf377_amd_resident.h"') < main.index('#include "decaf377_amd_long_sums.h"')
    assert not set(NAMES) & (set(_native.EXPORTS) | set(_native.RESIDENT_EXPORTS))
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_long_sums.rs")).read()
    protos = gen.prototypes(header)
    assert sorted(p[0] for p in protos) == sorted(NAMES)
    for name, ret, params in protos:
        assert name in defined and not name.endswith("_dev"), name
        assert len(params) == NAMES[name] and len(getattr(lib, name).argtypes) == NAMES[name], name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name


def _refused(lib, rc, word):
    assert rc == ERR_ARG
    msg = lib.d377_last_error().decode()
    assert re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(word), msg), (word, msg)   # named as a word of its own
    return msg


def test_plain_resident_forms_refuse_in_the_host_forms_order(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    pts, raw, k = np.zeros((18, 16), np.uint64), np.zeros((18, 32), np.uint8), np.zeros((18, 32), np.uint8)
    enc, st = np.full((2, 32), 0xA5, np.uint8), np.full(18, 0xA5, np.uint8)
    el, en = lib.d377_batch_long_msm_resident, lib.d377_batch_long_msm_encoded_resident
    for m in (0, 4097):                                          # m first: a null context and null buffers alike, also with n = 0
        for n in (2, 0):
            assert "m = %d" % m in _refused(lib, el(None, 0, None, None, None, m, n, None, None), "m")
            assert "m = %d" % m in _refused(lib, en(None, 0, None, None, None, m, n, None, None, None), "m")
    for m in (9, 3):                                             # then the buffers, then the context: the host form's texts
        _refused(lib, el(None, 0, None, None, _p(k), m, 2, _p(enc), None), "xyzt")
        _refused(lib, el(None, 0, None, _p(pts), None, m, 2, _p(enc), None), "scalar32")
        _refused(lib, el(None, 0, None, _p(pts), _p(k), m, 2, None, None), "enc32_out")
        _refused(lib, en(None, 0, None, None, _p(k), m, 2, _p(enc), None, _p(st)), "enc32")
        _refused(lib, en(None, 0, None, _p(raw), _p(k), m, 2, _p(enc), None, None), "status")
        _refused(lib, el(None, 0, None, _p(pts), _p(k), m, 2, _p(enc), None), "ctx")
        _refused(lib, en(None, 0, None, _p(raw), _p(k), m, 2, _p(enc), None, _p(st)), "ctx")
        _refused(lib, el(None, 0, None, None, None, m, 0, None, None), "ctx")       # n = 0 excuses the null buffers, not the null context
        host = lib.d377_batch_msm_long(None, _p(pts), None, m, 2, _p(enc), None), lib.d377_last_error().decode()
        assert (el(None, 0, None, _p(pts), None, m, 2, _p(enc), None), lib.d377_last_error().decode()) == host
    assert (enc == 0xA5).all() and (st == 0xA5).all()


def test_indexed_forms_refuse_in_order_without_a_device(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    pool, k = np.zeros((POOL, 16), np.uint64), np.zeros((18, 32), np.uint8)
    idx = np.zeros((2, 9), np.int32)
    enc = np.full((2, 32), 0xA5, np.uint8)
    host = lambda *a: lib.d377_batch_long_msm_indexed(None, *a)
    res = lambda *a: lib.d377_batch_long_msm_indexed_resident(None, 0, None, *a, None)
    for call in (host, res):
        for m in (0, 4097):                                      # m before pool_count, the buffers and ctx
            for n in (2, 0):
                assert "m = %d" % m in _refused(lib, call(None, 0, None, None, m, n, None, None), "m")
        for count in (0, 1 << 31):                               # then pool_count
            for n in (2, 0):
                _refused(lib, call(None, count, None, None, 9, n, None, None), "pool_count")
        _refused(lib, call(None, POOL, _p(idx), _p(k), 9, 2, _p(enc), None), "pool_xyzt")       # then the buffers, in their order
        _refused(lib, call(_p(pool), POOL, None, None, 9, 2, None, None), "point_index")
        _refused(lib, call(_p(pool), POOL, _p(idx), None, 9, 2, None, None), "scalar32")
        _refused(lib, call(_p(pool), POOL, _p(idx), _p(k), 9, 2, None, None), "enc32_out")
        _refused(lib, call(_p(pool), POOL, _p(idx), _p(k), 9, 2, _p(enc), None), "ctx")         # then the context
        _refused(lib, call(None, POOL, None, None, 9, 0, None, None), "ctx")
        _refused(lib, call(None, (1 << 31) - 1, None, None, 4096, 0, None, None), "ctx")        # the largest good sizes
    bad = idx.copy()
    bad[1, 3] = POOL                                             # ctx comes before the indices: a null context is not asked to read them
    _refused(lib, host(_p(pool), POOL, _p(bad), _p(k), 9, 2, _p(enc), None), "ctx")
    assert (enc == 0xA5).all()
