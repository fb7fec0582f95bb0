"""Many sums of any length each by Straus chains (d377_batch_segmented_msm, include/decaf377_amd_segmented_sums.h) without a GPU.

The plan (decaf377_amd/csrc/msm_segmented_plan.hpp) is checked against the header's statements, restated in
tests/_segmented_sums_cases.py with Python integers and linear scans: on the GPU cases and on seeded random lengths.  The walk
the device runs is compiled for the host (tests/host_sim/segmented_sums_sim.cpp) and checked, byte for byte, against the
oracle's fold per sum, every term read exactly once and no record read that nobody wrote; the same file, as a stand-alone
program over one fixed case, runs once under the address and undefined-behaviour sanitizers.  The ABI checks and the refusals
need no device either."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import _segmented_sums_cases as sc
from _oracle import _p
from _ragged_sums_cases import offsets_of, ragged_fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAMES = {"d377_batch_segmented_msm": 7, "d377_batch_segmented_msm_encoded": 8, "d377_batch_segmented_msm_resident": 10,
         "d377_batch_segmented_msm_encoded_resident": 11, "d377_segmented_msm_plan": 10}
ERR_ARG = -2
SIM_SRC = os.path.join(SIM_DIR, "segmented_sums_sim.cpp")
ALL_CASES = list(sc.CASES.values()) + list(sc.EQUAL.values())


def _stale(target):
    srcs = [SIM_SRC, os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libd377_sgs_sim.so")
    if _stale(lib):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC, SIM_SRC, "-o", lib])
    L = ctypes.CDLL(lib)
    L.sim_init.restype = ctypes.c_int
    L.sim_init()
    vp, sz, u64, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
    L.sgs_plan.argtypes = [vp, sz, vp]
    L.sgs_plan.restype = None
    L.sgs_chains_below_mean.restype = u64
    L.sgs_start.argtypes = [vp, sz, i32]
    L.sgs_start.restype = u64
    L.sgs_space.argtypes = [u64, sz, i32]
    L.sgs_space.restype = sz
    L.sgs_records.argtypes = [u64, i32]
    L.sgs_records.restype = sz
    L.sgs_levels.argtypes = [u64]
    L.sgs_find.argtypes = [vp, sz, i32, u64]
    L.sgs_find.restype = sz
    L.sgs_chain.argtypes = [vp, sz, u64, i32, u64, vp]
    L.sgs_chain.restype = None
    L.sgs_fold.argtypes = [vp, sz, i32, sz, u64, vp]
    L.sgs_fold.restype = None
    L.sgs_last.argtypes = [vp, sz, i32, sz, vp]
    L.sgs_last.restype = None
    L.sgs_walk.argtypes = [i32, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


def _plan(sim, off):  # noqa: F811
    out = np.zeros(19, np.uint64)
    sim.sgs_plan(_p(off), len(off) - 1, _p(out))
    v = [int(x) for x in out]
    lv = v[4]
    return {"terms": v[0], "chain_slots": v[1], "chains": v[2], "max_len": v[3], "levels": lv, "bmax": v[5], "records": v[6], "route": v[7],
            "space": v[8:9 + lv], "base": v[13:15 + lv]}


def _check_plan(sim, off):  # noqa: F811
    """The header's plan against the restatement, slot by slot and level by level."""
    n = len(off) - 1
    lens = [int(off[i + 1]) - int(off[i]) for i in range(n)]
    want, got = sc.plan(off), _plan(sim, off)
    for key in ("terms", "chain_slots", "chains", "levels", "bmax", "space", "records", "route"):
        assert got[key] == want[key], (key, got[key], want[key], lens[:20])
    assert got["base"] == [sum(want["space"][:l]) for l in range(want["levels"] + 2)]
    sc.assert_layout(off)
    T, buf = want["terms"], np.zeros(6, np.uint64)
    seen = np.zeros(T, np.int64)
    for level in range(want["levels"] + 1):
        st = sc.starts(off, level)
        assert [sim.sgs_start(_p(off), i, level) for i in range(n)] == st
        assert sim.sgs_space(T, n, level) == want["space"][level]
        expect = {}                                              # slot -> (sum, index within the sum)
        for i in range(n):
            for j in range(sc.records(lens[i], level)):
                assert st[i] + j not in expect                   # no overlap
                expect[st[i] + j] = (i, j)
        assert len(expect) >= want["space"][level] - n * (level + 1) and max(expect, default=-1) < want["space"][level]
        for p in range(want["space"][level]):
            i = sim.sgs_find(_p(off), n, level, p)
            assert i == sc.owner(st, p), (level, p)
            if level == 0 and T:
                sim.sgs_chain(_p(off), n, T, want["bmax"], p, _p(buf))
                live, s, q, first, count, b = (int(x) for x in buf)
                assert bool(live) == (p in expect), (p, lens[:20])
                if live:
                    assert (s, q) == expect[p]
                    f, c = sc.cut(lens[s])[q]
                    assert (first, count) == (int(off[s]) - int(off[0]) + f, c) and b == sc.cut(lens[s])[0][1]
                    seen[first:first + count] += 1
            if level > 0:
                sim.sgs_fold(_p(off), n, level - 1, want["space"][level - 1], p, _p(buf))
                live, s, lo, count = (int(x) for x in buf[:4])
                assert bool(live) == (p in expect), (level, p)
                if live:
                    j = expect[p][1]
                    c = sc.records(lens[s], level - 1)
                    assert s == expect[p][0] and lo == sc.starts(off, level - 1)[s] + sc.FOLD * j and count == min(sc.FOLD, c - sc.FOLD * j)
    assert (seen == 1).all()                                     # the live chains cover every term exactly once
    lv = want["levels"]
    st = sc.starts(off, lv)
    for i in range(n):
        sim.sgs_last(_p(off), i, lv, want["space"][lv], _p(buf))
        live, s, lo, count = (int(x) for x in buf[:4])
        c = sc.records(lens[i], lv)
        assert c <= sc.FOLD and count == c and bool(live) == (c > 0) and s == i
        if live:
            assert lo == st[i]


def test_plan_of_the_gpu_cases(sim):
    for lengths in ALL_CASES + [(0, 0, 0, 5, 0, 0, 9, 0, 0, 0), (9,), (8,), (1 << 20,) + (0,) * 3]:
        if max(lengths) < 1 << 20:
            _check_plan(sim, offsets_of(lengths))
    assert sc.cut(9) == [(0, 5), (5, 4)] and sc.cut(8) == [(0, 8)] and sc.cut(17) == [(0, 6), (6, 6), (12, 5)]
    assert [sc.levels(L) for L in (0, 1, 128, 129, 2048, 2049, 4097, 1 << 20)] == [0, 0, 0, 1, 1, 2, 2, 4]
    assert [sim.sgs_levels(L) for L in (0, 1, 128, 129, 2048, 2049, 4097, 1 << 20)] == [0, 0, 0, 1, 1, 2, 2, 4]
    assert [sc.records(2049, l) for l in range(4)] == [257, 17, 2, 1] == [sim.sgs_records(2049, l) for l in range(4)]
    p = _plan(sim, offsets_of((1 << 20,) + (0,) * 3))            # the longest sum allowed: the most levels
    assert p["levels"] == 4 == sc.plan(offsets_of((1 << 20,) + (0,) * 3))["levels"] and p["chains"] == 1 << 17 and p["bmax"] == 8
    assert p["space"] == sc.plan(offsets_of((1 << 20,) + (0,) * 3))["space"]
    # a device's slice: the first offset is not 0
    off = offsets_of(sc.CASES["crossing_eights"])
    _check_plan(sim, np.ascontiguousarray(off[3:]))


def test_plan_on_seeded_random_lengths(sim):
    rng = np.random.default_rng(377)
    for trial in range(60):
        n = int(rng.integers(1, 40))
        kind = trial % 4
        lens = rng.integers(0, (3, 20, 140, 600)[kind], n)
        lens[rng.random(n) < 0.3] = 0                            # runs of empty sums, wherever they fall
        if trial % 5 == 0:
            lens[:3] = 0
        if trial % 7 == 0:
            lens[-3:] = 0
        _check_plan(sim, offsets_of(lens))
    for trial in range(20000):                                   # the layout alone, on many more vectors
        n = int(rng.integers(1, 12))
        lens = rng.integers(0, (2, 10, 40, 300, 5000)[trial % 5], n) * (rng.random(n) < 0.7)
        sc.assert_layout(offsets_of(lens))


def test_advised_route(sim):
    assert sim.sgs_chains_below_mean() == sc.CHAINS_BELOW_MEAN == 1024
    for lengths, want in (((1023,), 0), ((1024,), 1), ((0, 1023, 0, 1024), 0), ((0, 1023, 0, 1025), 1), ((0, 0), 0), ((1, 4096), 1),
                          ((100,) * 50 + (4096,), 0)):
        assert _plan(sim, offsets_of(lengths))["route"] == want == sc.plan(offsets_of(lengths))["route"], lengths


def test_lookups_stay_in_range_whatever_the_array_holds(sim):
    rng = np.random.default_rng(5)
    big = (1 << 64) - 1
    arrays = [np.array(a, np.uint64) for a in ([big, 3, 0, big, 1, 2, 0], [9, 8, 7, 6, 5, 4, 3], [0] * 7, [big] * 7, [5, 0, 5, 0, 5, 0, 5],
                                               [0, 1 << 40, 5, 1 << 63, 6, 7, 8])]
    arrays += [rng.integers(0, 600, 7).astype(np.uint64) for _ in range(50)]
    buf = np.zeros(6, np.uint64)
    T, S = 40, 11
    for a in arrays:
        for n in range(1, 7):                                    # (a holds n + 1 values at least)
            for p in (0, 1, 2, 7, 8, 255, 599, 10 ** 6, big):
                for level in range(5):
                    assert 0 <= sim.sgs_find(_p(a), n, level, p) < n
                    if level < 4:
                        sim.sgs_fold(_p(a), n, level, S, p, _p(buf))
                        live, s, lo, count = (int(x) for x in buf[:4])
                        assert s < n and (not live or (1 <= count <= 16 and lo + count <= S))
                    for i in range(n):
                        sim.sgs_last(_p(a), i, level, S, _p(buf))
                        live, s, lo, count = (int(x) for x in buf[:4])
                        assert count <= 16 and (not live or lo + count <= S)
                for bmax in (1, 5, 8):
                    sim.sgs_chain(_p(a), n, T, bmax, p, _p(buf))
                    live, s, q, first, count, b = (int(x) for x in buf)
                    assert s < n and (not live or (1 <= count <= b <= bmax and first + count <= T))


def _walk(sim, encoded, pts, k, off):  # noqa: F811
    n, terms = len(off) - 1, int(off[-1]) - int(off[0])
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    st = np.full(max(terms, 1), 0xEE, np.uint8)
    touched = np.zeros(max(terms, 1), np.uint8)
    stats = np.zeros(5, np.int64)
    assert sim.sgs_walk(int(encoded), _p(pts), _p(k), _p(off), n, _p(enc), _p(el), _p(st), _p(touched), _p(stats)) == 0
    return enc, el, st[:terms], touched[:terms], stats


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_walk_matches_oracle_fold(sim, oracle, name):
    lengths = sc.CASES[name]
    for encoded in (False, True):
        rng = np.random.default_rng(len(lengths) * 1000 + encoded)
        pts, k, off, dead = sc.build(oracle, rng, lengths, encoded=encoded)
        enc, el, st, touched, stats = _walk(sim, encoded, pts, k, off)
        want_enc, want_el, want_st = ragged_fold(oracle, pts, k, off)
        assert (enc == want_enc).all(), (name, np.nonzero((enc != want_enc).any(1))[0])
        assert oracle.eq_xyzt(el, want_el).all() and (oracle.compress(el) == enc).all()
        assert (touched == 1).all()                              # every term read exactly once: no dead slot reads, none is skipped
        if encoded:
            assert (st == want_st).all() and ((want_st != 0) == dead).all()
        for s, L in enumerate(lengths):
            if L == 0:
                assert not enc[s].any() and oracle.is_identity(el[s:s + 1]).all()
        want = sc.plan(off)
        assert stats[0] == want["chains"] and stats[1] == (want["chain_slots"] - want["chains"] if want["terms"] else 0)
        assert stats[2] == want["levels"] and stats[4] == 0
    if name == "two_levels":
        assert stats[2] == 2
    if name == "fold_lane_full":
        assert stats[2] == 1


def test_walk_of_a_slice_whose_first_offset_is_not_zero(sim, oracle):
    lengths = sc.CASES["crossing_eights"]
    pts, k, off, _ = sc.build(oracle, np.random.default_rng(11), lengths)
    want_enc, _, _ = ragged_fold(oracle, pts, k, off)
    for lo in (2, 4, 6):
        t0 = int(off[lo])
        enc, _, _, touched, _ = _walk(sim, False, np.ascontiguousarray(pts[t0:]), np.ascontiguousarray(k[t0:]), np.ascontiguousarray(off[lo:]))
        assert (enc == want_enc[lo:]).all() and (touched == 1).all()


def test_sanitized_walk_as_a_stand_alone_program():
    """The same file with its own main over one fixed case, under the address and undefined-behaviour sanitizers: host code
    only, a child process, never loaded into Python."""
    exe = os.path.join(SIM_DIR, "segmented_sums_sim_san")
    if _stale(exe):
        subprocess.check_call(["g++", "-O1", "-fwhole-program", "-std=c++17", "-DD377_FB_BITS=12", "-DSEGMENTED_SIM_MAIN",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, SIM_SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SEGMENTED_SIM_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_defined_bound_and_in_the_rust_block(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd_segmented_sums.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.SEGMENTED_SUMS_EXPORTS)
    assert not any("ragged" in name for name in NAMES)
    assert re.search(r"#define D377_BATCH_SEGMENTED_MSM_MAX_TERMS \(1u << 20\)", header)
    main = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert main.index('#include "decaf377_amd_ragged_sums.h"') < main.index('#include "decaf377_amd_segmented_sums.h"')
    others = (set(_native.EXPORTS) | set(_native.RESIDENT_EXPORTS) | set(_native.LONG_SUMS_EXPORTS) | set(_native.BUCKET_SUMS_EXPORTS)
              | set(_native.RAGGED_SUMS_EXPORTS))
    assert not set(NAMES) & others and len(_native.EXPORTS) == 102
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {d for d in defined if "segmented" in d} == set(NAMES)
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_segmented_sums.rs")).read()
    protos = gen.prototypes(header)
    assert sorted(p[0] for p in protos) == sorted(NAMES)
    assert set(re.findall(r"pub fn (d377_[a-z0-9_]+)\(", ffi)) == set(NAMES)
    for name, ret, params in protos:
        assert len(params) == NAMES[name] and len(getattr(lib, name).argtypes) == NAMES[name], name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name
    gpu_rs = open(os.path.join(ROOT, "rust", "src", "gpu.rs")).read()
    assert "pub mod ffi_segmented_sums;" in gpu_rs
    for fn in ("vartime_multiscalar_mul_batch_segmented_gpu", "msm_segmented_resident"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, gpu_rs), fn
    hpp = open(os.path.join(ROOT, "include", "decaf377_amd.hpp")).read()
    for fn in ("vartime_multiscalar_mul_batch_segmented", "msm_segmented_resident"):
        assert re.search(r"\b%s\(" % fn, hpp), fn


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
    h_el = lambda a, b, o, n, e, x: lib.d377_batch_segmented_msm(None, a, b, o, n, e, x)                                    # noqa: E731
    h_en = lambda a, b, o, n, e, x, s: lib.d377_batch_segmented_msm_encoded(None, a, b, o, n, e, x, s)                       # noqa: E731
    r_el = lambda a, b, o, n, e, x: lib.d377_batch_segmented_msm_resident(None, 0, None, a, b, o, None, n, e, x)            # noqa: E731
    r_en = lambda a, b, o, n, e, x, s: lib.d377_batch_segmented_msm_encoded_resident(None, 0, None, a, b, o, None, n, e, x, s)   # noqa: E731
    huge = (1 << 64) - 1
    bad_offsets = [(np.array([1, 9, 18], np.uint64), 0), (np.array([0, 9, 8], np.uint64), 1), (np.array([0, 5, 5 + (1 << 20) + 1], np.uint64), 1),
                   (np.array([0, 0, 1 << 21], np.uint64), 1), (np.array([0, 9, 3, 2], np.uint64), 1)]
    for el, en in ((h_el, h_en), (r_el, r_en)):
        for n in (huge, huge // 8):                              # n first: null offsets and a null context alike
            assert "n = %d" % n in _refused(lib, el(None, None, None, n, None, None), "n")
            assert "n = %d" % n in _refused(lib, en(None, None, None, n, None, None, None), "n")
        _refused(lib, el(None, None, None, 2, None, None), "offsets")            # then null offsets
        _refused(lib, en(None, None, None, 2, None, None, None), "offsets")
        for off, first in bad_offsets:                           # then their values, before any null buffer
            n = len(off) - 1
            msg = _refused(lib, el(None, None, _p(off), n, None, None), "offsets")
            assert re.search(r"sum %d\b" % first, msg), msg
            assert re.search(r"sum %d\b" % first, _refused(lib, en(None, None, _p(off), n, None, None, None), "offsets"))
        _refused(lib, el(None, _p(k), _p(good), 2, _p(enc), None), "xyzt")        # then the buffers, then the context
        _refused(lib, el(_p(pts), None, _p(good), 2, _p(enc), None), "scalar32")
        _refused(lib, el(_p(pts), _p(k), _p(good), 2, None, None), "enc32_out")
        _refused(lib, en(None, _p(k), _p(good), 2, _p(enc), None, _p(st)), "enc32")
        _refused(lib, en(_p(raw), _p(k), _p(good), 2, _p(enc), None, None), "status")
        _refused(lib, el(_p(pts), _p(k), _p(good), 2, _p(enc), None), "ctx")
        _refused(lib, en(_p(raw), _p(k), _p(good), 2, _p(enc), None, _p(st)), "ctx")
        # no term: the term buffers are not required, enc32_out still is
        _refused(lib, el(None, None, _p(empty), 2, None, None), "enc32_out")
        _refused(lib, en(None, None, _p(empty), 2, None, None, None), "enc32_out")
        _refused(lib, el(None, None, _p(empty), 2, _p(enc), None), "ctx")
        _refused(lib, en(None, None, _p(empty), 2, _p(enc), None, None), "ctx")
        _refused(lib, el(None, None, None, 0, None, None), "ctx")                # n = 0 excuses the null buffers, not the null context
    plan = lambda o, n: lib.d377_segmented_msm_plan(None, 0, o, n, None, None, None, None, None, None)                      # noqa: E731
    _refused(lib, plan(None, 2), "offsets")
    assert "sum 1" in _refused(lib, plan(_p(bad_offsets[1][0]), 2), "offsets")
    _refused(lib, plan(_p(good), 2), "ctx")
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
    for call in (c.msm_segmented, lambda *a, **kw: c.msm_by_offsets(*a, route="chains", **kw)):
        with pytest.raises(ValueError, match="points must be"):
            call(np.zeros((18, 15), np.uint64), k, [0, 9, 18])
        with pytest.raises(ValueError, match="expected shape"):
            call(pts, k[:17], [0, 9, 18])                        # len(scalar32) != offsets[n]
        with pytest.raises(ValueError, match="offsets\\[n\\] = 17"):
            call(pts, k, [0, 9, 17])
        with pytest.raises(ValueError, match="never decrease"):
            call(pts, k, [0, 19, 18])
        with pytest.raises(ValueError, match="negative"):
            call(pts, k, [0, -1, 18])
        with pytest.raises(ValueError, match="integers"):
            call(pts, k, [0.0, 9.0, 18.0])
    with pytest.raises(ValueError, match="2 output arrays expected"):
        c.msm_segmented(pts, k, [0, 9, 18], outs=[np.zeros((2, 32), np.uint8)], elements=True)
    with pytest.raises(ValueError, match="never decrease"):
        c.msm_segmented_plan([0, 5, 4])
    with pytest.raises(ValueError, match="route must be"):
        c.msm_by_offsets(pts, k, [0, 9, 18], route="sorted")
    with pytest.raises(ValueError, match="points must be"):
        c.msm_by_offsets(np.zeros((18, 15), np.uint64), k, [0, 9, 18], route="buckets")
    assert engine.Context.msm_segmented.__doc__ and "ALLOCATES" in engine.Context.msm_segmented.__doc__
