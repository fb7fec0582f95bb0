"""Many sums of any length each (d377_batch_ragged_msm, include/decaf377_amd_ragged_sums.h) without a GPU.

The plan (decaf377_amd/csrc/msm_ragged_plan.hpp) is checked against the header's statements, restated in
tests/_ragged_sums_cases.py, and against the uniform call's plan on equal lengths.  The lookup is checked exhaustively against a
linear scan, and on arrays that are not monotone.  The walk the device runs is compiled for the host
(tests/host_sim/ragged_sums_sim.cpp) and checked, byte for byte, against the oracle's fold per sum; the same file, as a
stand-alone program over one fixed case, runs once under the address and undefined-behaviour sanitizers.  The ABI checks and the
refusals need no device either."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import _bucket_sums_cases as bc
from _oracle import _p
from _ragged_sums_cases import (CASES, MAX_TERMS, WIDTH_CASE, assert_cover_sums_cover, device_cuts, make_case, offsets_of, passes,
                                ragged_fold, sum_of_term, width)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAMES = {"d377_batch_ragged_msm": 8, "d377_batch_ragged_msm_encoded": 9, "d377_batch_ragged_msm_resident": 11,
         "d377_batch_ragged_msm_encoded_resident": 12, "d377_ragged_msm_plan": 10}
ERR_ARG = -2
SIM_SRC = os.path.join(SIM_DIR, "ragged_sums_sim.cpp")


def _stale(target):
    srcs = [SIM_SRC, os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libd377_rgs_sim.so")
    if _stale(lib):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC, SIM_SRC, "-o", lib])
    L = ctypes.CDLL(lib)
    L.sim_init.restype = ctypes.c_int
    L.sim_init()
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    L.rgs_sum_of_term.argtypes = [vp, ctypes.c_uint32, u64]
    L.rgs_sum_of_term.restype = ctypes.c_uint32
    L.rgs_tile_sum.argtypes = [vp, ctypes.c_uint32, u64, sz, sz]
    L.rgs_tile_sum.restype = ctypes.c_uint32
    L.rgs_window.argtypes = [u64, sz, ctypes.c_int]
    L.rgs_first_bad_sum.argtypes = [vp, sz]
    L.rgs_first_bad_sum.restype = sz
    L.rgs_device_cut.argtypes = [vp, sz, sz, sz]
    L.rgs_device_cut.restype = sz
    L.rgs_plan.argtypes = [vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.rgs_plan.restype = None
    L.rgs_passes.argtypes = [vp, sz, ctypes.c_int, vp, sz]
    L.rgs_passes.restype = sz
    L.rgs_walk.argtypes = [ctypes.c_int, vp, vp, vp, sz, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def bucket_sim():
    lib = os.path.join(SIM_DIR, "libd377_bks_sim.so")
    if _stale(lib):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "bucket_sums_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.bks_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


def _plan(sim, off, wb, cus=256):  # noqa: F811
    head = np.zeros(5, np.int64)
    sim.rgs_plan(_p(off), len(off) - 1, wb, cus, 4, _p(head))
    return dict(zip(("c", "passes", "max_sums", "max_points", "bytes"), map(int, head)))


def _cuts(sim, off, c):  # noqa: F811
    out = np.zeros(3 * 4096, np.uint64)
    cnt = sim.rgs_passes(_p(off), len(off) - 1, c, _p(out), 4096)
    return cnt, [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(min(cnt, 4096))]


def _uniform_plan(bucket_sim, n, m, wb, cus=256):
    head, full, last = np.zeros(5, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int64)
    off = [np.zeros(64, np.uint64) for _ in range(4)]
    consts = np.zeros(16, np.int32)
    bucket_sim.bks_plan(n, m, wb, cus, 4, _p(head), _p(full), _p(off[0]), _p(off[1]), _p(last), _p(off[2]), _p(off[3]), _p(consts))
    return dict(zip(("c", "spp", "passes", "last_sums", "bytes"), map(int, head)))


ALL_CASES = list(CASES.values()) + [WIDTH_CASE, ((300,), 0)]


def test_pass_cuts_and_width_of_the_gpu_cases(sim):
    for lengths, wb in ALL_CASES:
        off = offsets_of(lengths)
        c = width(off, wb)
        p = _plan(sim, off, wb)
        want = passes(off, c)
        cnt, got = _cuts(sim, off, c)
        assert p["c"] == c and cnt == len(want) == p["passes"] and got == want, (lengths, wb)
        assert p["max_sums"] == max(K for _, K, _ in want) and p["max_points"] == max(n for _, _, n in want)
        assert sum(K for _, K, _ in want) == len(lengths) and sum(n for _, _, n in want) == int(off[-1])
        assert p["bytes"] > p["max_points"] * 128
    assert [K for _, K, _ in passes(offsets_of(CASES["passes_middle_empty"][0]), 16)] == [4, 4, 1]
    assert [n for _, _, n in passes(offsets_of(CASES["passes_middle_empty"][0]), 16)] == [44, 0, 33]       # the middle pass has no point
    assert width(offsets_of(WIDTH_CASE[0])) == bc.window_rule(1127) == sim.rgs_window(6762, 6, 0)
    assert sim.rgs_window(0, 0, 0) == bc.window_rule(1) and sim.rgs_window(0, 5, 0) == bc.window_rule(1) and sim.rgs_window(999, 3, 7) == 7


def test_equal_lengths_give_the_uniform_plan(sim, bucket_sim):
    shapes = list(bc.WALK) + [(n, m, 0) for m in (256, 4096, 1 << 16) for n in (1, 3, 300)]
    shapes += [(5000, 4096, 8), (40, 1 << 20, 14), (70000, 3, 4)]          # passes closed by the points and by the keys
    for n, m, wb in shapes:
        off = offsets_of([m] * n)
        for cus in (256, 304):
            p, u = _plan(sim, off, wb, cus), _uniform_plan(bucket_sim, n, m, wb, cus)
            assert (p["c"], p["passes"], p["bytes"], p["max_sums"]) == (u["c"], u["passes"], u["bytes"], u["spp"]), (n, m, wb)
            assert p["max_points"] == u["spp"] * m
        assert [(f, K) for f, K, _ in passes(off, width(off, wb))] == bc.passes(n, m, width(off, wb))


def test_a_million_one_term_sums_and_a_pass_closed_by_the_points(sim):
    off = offsets_of(np.ones(1 << 20, np.uint64))
    p = _plan(sim, off, 4)
    cnt, got = _cuts(sim, off, 4)
    assert p["passes"] == cnt == 64 and p["max_sums"] == p["max_points"] == 1 << 14
    assert got == [(i << 14, 1 << 14, 1 << 14) for i in range(64)] == passes(off, 4)
    off = offsets_of([MAX_TERMS] * 17)                           # sixteen sums fill the 2^24 points of a pass
    for wb in (14, 4):
        cnt, got = _cuts(sim, off, wb)
        assert got == [(0, 16, 1 << 24), (16, 1, 1 << 20)] == passes(off, wb) and cnt == 2
        assert _plan(sim, off, wb)["max_points"] == 1 << 24
    off = offsets_of([MAX_TERMS] * 15 + [MAX_TERMS // 2] * 2 + [5])   # seventeen sums fill them exactly; five more terms do not fit
    assert _cuts(sim, off, 4)[1] == [(0, 17, 1 << 24), (17, 1, 5)] == passes(off, 4)
    off = offsets_of([MAX_TERMS - 1] * 8 + [8] + [0] * 9)
    assert _cuts(sim, off, 14)[1] == [(0, 16, 8 * MAX_TERMS), (16, 2, 0)] == passes(off, 14)       # (closed by the keys: 16 * 2^13)
    assert sim.rgs_first_bad_sum(_p(offsets_of([3, MAX_TERMS, MAX_TERMS + 1, 2])), 4) == 2
    assert sim.rgs_first_bad_sum(_p(np.array([0, 5, 4, 9], np.uint64)), 3) == 1
    assert sim.rgs_first_bad_sum(_p(offsets_of([0, 0, MAX_TERMS])), 3) == 3


def test_device_slices_are_balanced_by_terms(sim):
    shapes = [lengths for lengths, _ in ALL_CASES] + [(0, 0, 0), (5,), (1000, 1, 1, 1), (1, 1, 1, 1000), (10, 10, 10, 10, 10, 10), (0, 7, 0, 0, 7, 0)]
    for lengths in shapes:
        off = offsets_of(lengths)
        n = len(lengths)
        for nd in (1, 2, 3):
            got = [sim.rgs_device_cut(_p(off), n, nd, k) for k in range(nd + 1)]
            assert got == device_cuts(off, nd), (lengths, nd)
            assert got[0] == 0 and got[-1] == n and all(a <= b for a, b in zip(got, got[1:]))
    off = offsets_of((1000, 1, 1, 1))
    assert device_cuts(off, 2) == [0, 1, 4]                      # by terms, not by sums: the long sum alone
    assert device_cuts(offsets_of((10,) * 6), 3) == [0, 2, 4, 6] and device_cuts(offsets_of(WIDTH_CASE[0]), 2) == [0, 2, 6]


def test_lookup_against_a_linear_scan(sim):
    for lengths, wb in ALL_CASES:
        off = offsets_of(lengths)
        c = width(off, wb)
        for first, K, N in passes(off, c):
            po = np.ascontiguousarray(off[first:first + K + 1])
            base = int(po[0])
            for i in range(N):
                want = sum_of_term(po, K, base + i)
                assert lengths[first + want] > 0                 # a run of empty sums resolves to the non-empty sum behind it
                assert sim.rgs_sum_of_term(_p(po), K, base + i) == want, (lengths, first, i)
                assert sim.rgs_tile_sum(_p(po), K, base, N, i) == want, (lengths, first, i)


def test_lookup_stays_in_range_whatever_the_array_holds(sim):
    rng = np.random.default_rng(5)
    big = (1 << 64) - 1
    arrays = [np.array(a, np.uint64) for a in ([big, 3, 0, big, 1, 2, 0], [9, 8, 7, 6, 5, 4, 3], [0, 0, 0, 0, 0, 0, 0], [big] * 7, [5, 0, 5, 0, 5, 0, 5])]
    arrays += [rng.integers(0, 600, 7).astype(np.uint64) for _ in range(50)]
    for a in arrays:
        for K in range(1, 7):                                    # (a holds K + 1 values at least; a[K] is never needed)
            for g in (0, 1, 2, 3, 5, 255, 256, 599, 10 ** 6, big):
                assert 0 <= sim.rgs_sum_of_term(_p(a), K, g) < K
                for n, i in ((700, 0), (700, 300), (700, 699), (1, 0), (256, 255), (257, 256)):
                    assert 0 <= sim.rgs_tile_sum(_p(a), K, g, n, i) < K
    off = offsets_of((3, 4, 5))                                  # a g past the end: the last sum
    assert sim.rgs_sum_of_term(_p(off), 3, 12) == sim.rgs_sum_of_term(_p(off), 3, big) == 2


def _walk(sim, encoded, pts, k, off, wb):  # noqa: F811
    n = len(off) - 1
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    st = np.full(int(off[-1]), 0xEE, np.uint8) if encoded else None
    stats = np.zeros(5, np.int64)
    assert sim.rgs_walk(int(encoded), _p(pts), _p(k), _p(off), n, wb, 256, _p(enc), _p(el), _p(st) if encoded else None, _p(stats)) == 0
    return enc, el, st, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_matches_oracle_fold(sim, oracle, name):
    lengths, c = CASES[name]
    for encoded in (False, True):
        rng = np.random.default_rng(len(lengths) * 1000 + c + encoded)
        pts, k, off, info = make_case(oracle, rng, lengths, c, encoded=encoded)
        assert_cover_sums_cover(k, off, info, c)
        assert info["dead"].any() and "specials" in info
        enc, el, st, stats = _walk(sim, encoded, pts, k, off, c)
        want_enc, want_el, want_st = ragged_fold(oracle, pts, k, off)
        assert (enc == want_enc).all(), (name, np.nonzero((enc != want_enc).any(1))[0])
        assert oracle.eq_xyzt(el, want_el).all() and (oracle.compress(el) == enc).all()
        if encoded:
            assert (st == want_st).all() and ((want_st != 0) == info["dead"]).all()
        for s in info["empty"]:
            assert not enc[s].any() and oracle.is_identity(el[s:s + 1]).all()
        assert stats[0] == len(passes(off, c))
        if name == "passes_middle_empty":
            assert stats[0] == 3 and stats[4] == 1
        if name == "int32_keys":
            assert stats[2] == 1 and stats[3] == 0 and stats[1] > 1 << 15
        if name == "int16_keys":
            assert stats[2] == 0 and stats[3] == 1 and stats[1] == 1 << 15


def test_sanitized_walk_as_a_stand_alone_program():
    """The same file with its own main over one fixed case, under the address and undefined-behaviour sanitizers: host code
    only, a child process, never loaded into Python."""
    exe = os.path.join(SIM_DIR, "ragged_sums_sim_san")
    if _stale(exe):
        # (-fwhole-program: everything but main is local, so the simulations this program never calls are dropped before they
        # are instrumented)
        subprocess.check_call(["g++", "-O1", "-fwhole-program", "-std=c++17", "-DD377_FB_BITS=12", "-DRAGGED_SIM_MAIN", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, SIM_SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RAGGED_SIM_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_defined_bound_and_in_the_rust_block(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd_ragged_sums.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.RAGGED_SUMS_EXPORTS)
    assert re.search(r"#define D377_BATCH_RAGGED_MSM_MAX_TERMS \(1u << 20\)", header)
    main = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert main.index('#include "decaf377_amd_bucket_sums.h"') < main.index('#include "decaf377_amd_ragged_sums.h"')
    others = set(_native.EXPORTS) | set(_native.RESIDENT_EXPORTS) | set(_native.LONG_SUMS_EXPORTS) | set(_native.BUCKET_SUMS_EXPORTS)
    assert not set(NAMES) & others and len(_native.EXPORTS) == 102
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {d for d in defined if "ragged" in d} == set(NAMES)
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_ragged_sums.rs")).read()
    protos = gen.prototypes(header)
    assert sorted(p[0] for p in protos) == sorted(NAMES)
    lines = set(re.findall(r"pub fn (d377_[a-z0-9_]+)\(", ffi))
    assert lines == set(NAMES)
    for name, ret, params in protos:
        assert len(params) == NAMES[name] and len(getattr(lib, name).argtypes) == NAMES[name], name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name
    gpu_rs = open(os.path.join(ROOT, "rust", "src", "gpu.rs")).read()
    assert "pub mod ffi_ragged_sums;" in gpu_rs
    for fn in ("vartime_multiscalar_mul_batch_ragged_gpu", "msm_ragged_resident"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, gpu_rs), fn


def _refused(lib, rc, word):
    assert rc == ERR_ARG
    msg = lib.d377_last_error().decode()
    assert re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(word), msg), (word, msg)   # named as a word of its own
    return msg


def test_refusals_come_in_the_documented_order_without_a_device(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    pts, raw, k = np.zeros((18, 16), np.uint64), np.zeros((18, 32), np.uint8), np.zeros((18, 32), np.uint8)
    enc, st = np.full((2, 32), 0xA5, np.uint8), np.full(18, 0xA5, np.uint8)
    good, empty = np.array([0, 9, 18], np.uint64), np.array([0, 0, 0], np.uint64)
    h_el = lambda a, b, o, n, wb, e, x: lib.d377_batch_ragged_msm(None, a, b, o, n, wb, e, x)                              # noqa: E731
    h_en = lambda a, b, o, n, wb, e, x, s: lib.d377_batch_ragged_msm_encoded(None, a, b, o, n, wb, e, x, s)                 # noqa: E731
    r_el = lambda a, b, o, n, wb, e, x: lib.d377_batch_ragged_msm_resident(None, 0, None, a, b, o, None, n, wb, e, x)      # noqa: E731
    r_en = lambda a, b, o, n, wb, e, x, s: lib.d377_batch_ragged_msm_encoded_resident(None, 0, None, a, b, o, None, n, wb, e, x, s)   # noqa: E731
    huge = (1 << 64) - 1
    bad_offsets = [(np.array([1, 9, 18], np.uint64), 0), (np.array([0, 9, 8], np.uint64), 1), (np.array([0, 5, 5 + (1 << 20) + 1], np.uint64), 1),
                   (np.array([0, 0, 1 << 21], np.uint64), 1), (np.array([0, 9, 3, 2], np.uint64), 1)]
    for el, en in ((h_el, h_en), (r_el, r_en)):
        for n in (huge, huge // 8):                              # n first: a bad window_bits, null offsets and a null context alike
            assert "n = %d" % n in _refused(lib, el(None, None, None, n, 99, None, None), "n")
            assert "n = %d" % n in _refused(lib, en(None, None, None, n, 99, None, None, None), "n")
        for wb in (-1, 1, 3, 17, 18):                            # then window_bits
            for n in (2, 0):
                assert "window_bits = %d" % wb in _refused(lib, el(None, None, None, n, wb, None, None), "window_bits")
                assert "window_bits = %d" % wb in _refused(lib, en(None, None, None, n, wb, None, None, None), "window_bits")
        _refused(lib, el(None, None, None, 2, 0, None, None), "offsets")         # then null offsets
        _refused(lib, en(None, None, None, 2, 16, None, None, None), "offsets")
        for off, first in bad_offsets:                           # then their values, before any null buffer
            n = len(off) - 1
            msg = _refused(lib, el(None, None, _p(off), n, 0, None, None), "offsets")
            assert re.search(r"sum %d\b" % first, msg), msg
            assert re.search(r"sum %d\b" % first, _refused(lib, en(None, None, _p(off), n, 4, None, None, None), "offsets"))
        for wb in (0, 16, 4):                                    # then the buffers, then the context
            _refused(lib, el(None, _p(k), _p(good), 2, wb, _p(enc), None), "xyzt")
            _refused(lib, el(_p(pts), None, _p(good), 2, wb, _p(enc), None), "scalar32")
            _refused(lib, el(_p(pts), _p(k), _p(good), 2, wb, None, None), "enc32_out")
            _refused(lib, en(None, _p(k), _p(good), 2, wb, _p(enc), None, _p(st)), "enc32")
            _refused(lib, en(_p(raw), _p(k), _p(good), 2, wb, _p(enc), None, None), "status")
            _refused(lib, el(_p(pts), _p(k), _p(good), 2, wb, _p(enc), None), "ctx")
            _refused(lib, en(_p(raw), _p(k), _p(good), 2, wb, _p(enc), None, _p(st)), "ctx")
            # no term: the term buffers are not required, enc32_out still is
            _refused(lib, el(None, None, _p(empty), 2, wb, None, None), "enc32_out")
            _refused(lib, en(None, None, _p(empty), 2, wb, None, None, None), "enc32_out")
            _refused(lib, el(None, None, _p(empty), 2, wb, _p(enc), None), "ctx")
            _refused(lib, en(None, None, _p(empty), 2, wb, _p(enc), None, None), "ctx")
            _refused(lib, el(None, None, None, 0, wb, None, None), "ctx")        # n = 0 excuses the null buffers, not the null context
    plan = lambda o, n, wb: lib.d377_ragged_msm_plan(None, 0, o, n, wb, None, None, None, None, None)                      # noqa: E731
    assert "window_bits = 17" in _refused(lib, plan(_p(good), 2, 17), "window_bits")
    _refused(lib, plan(None, 2, 0), "offsets")
    assert "sum 1" in _refused(lib, plan(_p(bad_offsets[1][0]), 2, 0), "offsets")
    _refused(lib, plan(_p(good), 2, 0), "ctx")
    assert (enc == 0xA5).all() and (st == 0xA5).all()


def test_python_rejects_bad_arguments_before_any_native_call():
    import decaf377_amd as d
    from decaf377_amd import engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("native call: " + name)

    c = object.__new__(d.Context)
    c._lib, c._h, c.device_ids = NoLib(), None, [0]
    pts, k = np.zeros((18, 16), np.uint64), np.zeros((18, 32), np.uint8)
    with pytest.raises(ValueError, match="points must be"):
        c.msm_ragged(np.zeros((18, 15), np.uint64), k, [0, 9, 18])
    with pytest.raises(ValueError, match="expected shape"):
        c.msm_ragged(pts, k[:17], [0, 9, 18])                    # len(scalar32) != offsets[n]
    with pytest.raises(ValueError, match="offsets\\[n\\] = 17"):
        c.msm_ragged(pts, k, [0, 9, 17])
    with pytest.raises(ValueError, match="never decrease"):
        c.msm_ragged(pts, k, [0, 19, 18])
    with pytest.raises(ValueError, match="never decrease"):
        c.msm_ragged(pts, k, np.array([1, 9, 18], np.uint64))
    with pytest.raises(ValueError, match="negative"):
        c.msm_ragged(pts, k, [0, -1, 18])
    with pytest.raises(ValueError, match="integers"):
        c.msm_ragged(pts, k, [0.0, 9.0, 18.0])
    with pytest.raises(ValueError, match="2 output arrays expected"):
        c.msm_ragged(pts, k, [0, 9, 18], outs=[np.zeros((2, 32), np.uint8)], elements=True)
    with pytest.raises(ValueError, match="never decrease"):
        c.msm_ragged_plan([0, 5, 4])
    assert engine.Context.msm_ragged.__doc__ and "ALLOCATES" in engine.Context.msm_ragged.__doc__
