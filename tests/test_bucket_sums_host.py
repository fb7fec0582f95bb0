"""Many sums by the bucket method (d377_batch_bucket_msm, include/decaf377_amd_bucket_sums.h) without a GPU.

The plan (decaf377_amd/csrc/msm_batch_plan.hpp, over msm_plan.hpp's msm_plan with `sums`) is checked over a grid of (n, m,
window_bits, CUs) against the header's statements, restated in tests/_bucket_sums_cases.py.  The walk the device runs --
composite keys by the shared function, in the digit type the plan chooses, buckets, owner and weight by the shared decode,
Horner over the windows, the encoding -- is compiled for the host (tests/host_sim/bucket_sums_sim.cpp) and checked, byte for
byte, against the oracle's fold.  The ABI checks need no device either."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from _bucket_sums_cases import (MAX_TERMS, WALK, assert_boundary_sums_cover, key, make_case, oracle_fold, passes, sums_per_pass, window_rule,
                                windows)
from _oracle import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
NAMES = {"d377_batch_bucket_msm": 8, "d377_batch_bucket_msm_encoded": 9, "d377_batch_bucket_msm_resident": 10,
         "d377_batch_bucket_msm_encoded_resident": 11, "d377_bucket_msm_plan": 9}
ERR_ARG = -2
FIELDS = ("W", "nb", "sums", "pw", "wide_digits", "packed", "tree", "ws_depth", "ws_m", "ws_nblk", "ws8", "ws_mid", "top_m", "top_nblk",
          "top_stride", "wsb_lds", "count_parts", "count_nbr", "hist_bytes", "bytes", "c", "scan_chunks", "S", "per", "max_segs", "span_lanes_max")
CONSTS = ("PT_WORDS", "NODE_STRIDE", "R_NODES", "R_SUMS", "R_BUCKETS", "R_DIGITS", "R_IDX", "R_PTS", "R_CHUNKS", "R_FOLD0", "R_FOLD1", "R_MID")
KIB = 1024


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libd377_bks_sim.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("bucket_sums_sim.cpp", "sim.cpp")]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC,
                               os.path.join(SIM_DIR, "bucket_sums_sim.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.sim_init.restype = ctypes.c_int
    L.sim_init()
    L.bks_window.argtypes = [ctypes.c_size_t]
    L.bks_key.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
    L.bks_key_digit.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.bks_bucket_owner.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.bks_leaf_base.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
    L.bks_leaf_base.restype = ctypes.c_uint64
    L.bks_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    L.bks_walk.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


class Plan:
    def __init__(self, sim, n, m, window_bits, cus, span_blocks=4):  # noqa: F811
        head, full, last = np.zeros(5, np.int64), np.zeros(len(FIELDS), np.int64), np.zeros(len(FIELDS), np.int64)
        off = [np.zeros(64, np.uint64) for _ in range(4)]
        consts = np.zeros(len(CONSTS), np.int32)
        self.nregions = sim.bks_plan(n, m, window_bits, cus, span_blocks, _p(head), _p(full), _p(off[0]), _p(off[1]), _p(last), _p(off[2]),
                                     _p(off[3]), _p(consts))
        self.c, self.spp, self.passes, self.last_sums, self.bytes = (int(v) for v in head)
        self.full, self.last = dict(zip(FIELDS, map(int, full))), dict(zip(FIELDS, map(int, last)))
        self.regions = {"full": ([int(v) for v in off[0][:self.nregions]], [int(v) for v in off[1][:self.nregions]]),
                        "last": ([int(v) for v in off[2][:self.nregions]], [int(v) for v in off[3][:self.nregions]])}
        self.k = dict(zip(CONSTS, map(int, consts)))


GRID_M = (1, 2, 3, 9, 255, 256, 4096, 4097, 65536, (1 << 20) - 1, 1 << 20)
GRID_N = (1, 2, 5, 64, 65, 4096, 100000)


def test_plan_over_the_grid(sim):
    seen_types = set()
    for cus in (8, 256, 304):
        for m in GRID_M:
            for n in GRID_N:
                for wb in (0, 4, 5, 11, 12, 15, 16):
                    p = Plan(sim, n, m, wb, cus)
                    tag = (cus, n, m, wb)
                    c = p.c
                    assert 4 <= c <= 16 and (c == wb if wb else c == window_rule(m)), tag   # window_bits_used equals a forced width
                    assert p.spp == sums_per_pass(n, m, c), tag
                    cuts = passes(n, m, c)
                    assert p.passes == len(cuts) and p.last_sums == cuts[-1][1], tag
                    # the passes cover every sum exactly once
                    assert [lo for lo, _ in cuts] == [i * p.spp for i in range(p.passes)] and sum(cnt for _, cnt in cuts) == n, tag
                    assert all(cnt == p.spp for _, cnt in cuts[:-1]) and 1 <= p.last_sums <= p.spp, tag
                    for which, K in (("full", p.spp), ("last", p.last_sums)):
                        f = getattr(p, which)
                        N = K * m
                        assert f["sums"] == K and f["c"] == c and f["W"] == windows(c) and f["pw"] == f["W"] * K, tag
                        assert (K << (c - 1)) <= 1 << 17 and N <= 1 << 24, tag               # the sort's limit, packed placement
                        assert f["nb"] == (K << (c - 1)) + 1 and f["packed"] == 1, tag
                        assert f["wide_digits"] == int((K << (c - 1)) > 1 << 15), tag      # the digit type switches exactly at 2^15
                        seen_types.add((f["wide_digits"], (K << (c - 1)) in (1 << 15, (1 << 15) + (1 << (c - 1)))))
                        assert f["count_parts"] * f["count_nbr"] >= f["nb"] and f["count_nbr"] <= (1 << 15) + 1, tag
                        assert f["hist_bytes"] <= 160 * KIB and f["wsb_lds"] <= 160 * KIB, tag
                        # the tree: no middle level, a whole number of blocks per pseudo-window of 2^(c-1) leaves
                        assert f["tree"] == 1 and f["ws_mid"] == 0 and f["ws_depth"] == c - 1, tag
                        assert f["ws_nblk"] << f["ws_m"] == 1 << (c - 1) and 2 <= f["ws_m"] <= (9 if f["ws8"] else 8), tag
                        assert (f["top_m"], f["top_nblk"], f["top_stride"]) == (f["ws_m"], f["ws_nblk"], p.k["NODE_STRIDE"]), tag
                        assert f["ws_m"] + 1 <= p.k["NODE_STRIDE"], tag
                        # the regions: aligned, disjoint, in order, inside the workspace the call reserves
                        off, sz = p.regions[which]
                        end = 0
                        for o, s in zip(off, sz):
                            assert o % 256 == 0 and o >= end and o + s <= f["bytes"] <= p.bytes, tag
                            end = o + s
                        pt = p.k["PT_WORDS"] * 4
                        assert sz[p.k["R_NODES"]] >= f["pw"] * f["ws_nblk"] * p.k["NODE_STRIDE"] * pt, tag
                        assert sz[p.k["R_SUMS"]] >= f["pw"] * pt and sz[p.k["R_BUCKETS"]] >= f["W"] * f["nb"] * pt, tag
                        assert sz[p.k["R_DIGITS"]] >= f["W"] * N * (4 if f["wide_digits"] else 2), tag
                        assert sz[p.k["R_IDX"]] >= f["W"] * N * 4 and sz[p.k["R_PTS"]] >= N * 128, tag   # (R_IDX stages the int16 digits)
                        assert sz[p.k["R_CHUNKS"]] == sz[p.k["R_FOLD0"]] == sz[p.k["R_FOLD1"]] == sz[p.k["R_MID"]] == 0 or K == 1, tag
                    assert p.bytes == max(p.full["bytes"], p.last["bytes"]), tag
    assert {(0, True), (1, True)} <= seen_types                  # both sides of the switch were met at the switch
    # the rule is a function of m alone, in range, and the restated rule agrees for every length class
    for m in list(range(1, 3000)) + [1 << e for e in range(12, 21)] + [(1 << e) + 1 for e in range(12, 20)]:
        assert sim.bks_window(m) == window_rule(m) and 4 <= window_rule(m) <= 16
    assert [window_rule(m) for m in (1, 256, 4096, 1 << 16, MAX_TERMS)] == [5, 6, 8, 11, 14]     # the widths the sweep has ahead


def test_one_sum_is_the_single_msm_plan(sim):
    """sums = 1 leaves msm_plan what tests/test_msm_plan_host.py pins (nb = 2^(c-1) + 1, int16 up to 16 bits)."""
    for c in range(4, 17):
        p = Plan(sim, 1, 5000, c, 256)
        assert p.full["nb"] == (1 << (c - 1)) + 1 and p.full["wide_digits"] == 0 and p.full["pw"] == p.full["W"]


def test_key_decode_inverts_encode_at_the_edges(sim):
    for c in range(4, 17):
        K = (1 << 17) >> (c - 1)
        half = 1 << (c - 1)
        sum_, wt = ctypes.c_uint32(), ctypes.c_uint32()
        for k in (0, 1, K // 2, K - 1):
            for d in (1, -1, -half, half - 1, -(half - 1), 2 if half > 2 else 1):
                v = sim.bks_key(k, c, d)
                assert v == key(k, c, d) and 1 <= abs(v) <= K * half
                assert (v > 0) == (d > 0)
                back = ctypes.c_uint32(99)
                assert sim.bks_key_digit(v, c, ctypes.byref(back)) == d and back.value == k
                # the bucket |v| belongs to sum k with weight |d|, and is leaf |d| - 1 of pseudo-window (w, k)
                sim.bks_bucket_owner(abs(v), c, ctypes.byref(sum_), ctypes.byref(wt))
                assert (sum_.value, wt.value) == (k, abs(d))
                nb = K * half + 1
                assert sim.bks_leaf_base(3, k, nb, c) + abs(d) == 3 * nb + abs(v)
            assert sim.bks_key(k, c, 0) == 0
        # int16 holds every key while K 2^(c-1) <= 2^15: -2^15 is the one key of that magnitude
        K16 = (1 << 15) >> (c - 1)
        assert sim.bks_key(K16 - 1, c, -half) == -(1 << 15) and sim.bks_key(K16 - 1, c, half - 1) == (1 << 15) - 1


@pytest.mark.parametrize("n,m,c", WALK)
def test_walk_matches_oracle_fold(sim, oracle, n, m, c):
    rng = np.random.default_rng(100 * n + m)
    pts, k, info = make_case(oracle, rng, n, m, c)
    if m >= 3:
        assert_boundary_sums_cover(k, info, m, c)                # (one term cannot hold the three scalars that cover a layout)
        cuts = passes(n, m, c)
        assert sorted(info["boundary"]) == sorted({s for lo, cnt in cuts for s in (lo, lo + cnt - 1)})
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    stats = np.zeros(5, np.int64)
    assert sim.bks_walk(0, _p(pts), _p(k), m, n, c, 256, _p(enc), _p(el), None, _p(stats)) == 0
    want_passes = {(9, 33, 16): 3}.get((n, m, c), 1)
    assert stats[0] == want_passes == len(passes(n, m, c))
    if (n, m, c) == (9, 33, 16):
        assert [cnt for _, cnt in passes(n, m, c)] == [4, 4, 1]
    if (n, m, c) == (17, 40, 12):
        assert stats[2] == 1 and stats[3] == 0 and stats[1] > 1 << 15       # int32 keys
    if (n, m, c) == (16, 40, 12):
        assert stats[2] == 0 and stats[3] == 1 and stats[1] == 1 << 15      # int16 keys whose magnitude reaches 2^15
    want_enc, want_el, _ = oracle_fold(oracle, pts, k, m)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    for s in info["identity"]:
        assert not enc[s].any() and oracle.is_identity(el[s:s + 1]).all()
    if n >= 9:
        assert len(info["identity"]) == 2


@pytest.mark.parametrize("n,m,c", [(3, 5, 4), (9, 33, 16)])
def test_walk_on_encodings_reports_invalid_ones(sim, oracle, n, m, c):
    rng = np.random.default_rng(7000 + m)
    raw, k, info = make_case(oracle, rng, n, m, c, encoded=True)
    assert info["dead"].any()
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    st = np.full(n * m, 0xEE, np.uint8)
    assert sim.bks_walk(1, _p(raw), _p(k), m, n, c, 256, _p(enc), _p(el), _p(st), None) == 0
    want_enc, want_el, want_st = oracle_fold(oracle, raw, k, m)
    assert ((want_st != 0) == info["dead"]).all()
    assert (st == want_st).all() and (enc == want_enc).all()
    assert oracle.eq_xyzt(el, want_el).all()


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_defined_bound_and_in_the_rust_block(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd_bucket_sums.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.BUCKET_SUMS_EXPORTS)
    assert re.search(r"#define D377_BATCH_BUCKET_MSM_MAX_TERMS \(1u << 20\)", header)
    main = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert main.index('#include "decaf377_amd_long_sums.h"') < main.index('#include "decaf377_amd_bucket_sums.h"')
    assert not set(NAMES) & (set(_native.EXPORTS) | set(_native.RESIDENT_EXPORTS) | set(_native.LONG_SUMS_EXPORTS))
    assert len(_native.EXPORTS) == 102
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_bucket_sums.rs")).read()
    protos = gen.prototypes(header)
    assert sorted(p[0] for p in protos) == sorted(NAMES)
    for name, ret, params in protos:
        assert name in defined and not name.endswith("_dev") and "msm_long" not in name, name
        assert len(params) == NAMES[name] and len(getattr(lib, name).argtypes) == NAMES[name], name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name
    gpu_rs = open(os.path.join(ROOT, "rust", "src", "gpu.rs")).read()
    assert "pub mod ffi_bucket_sums;" in gpu_rs and not re.search(r"\bffi::d377_(batch_)?bucket", gpu_rs)
    for fn in ("vartime_multiscalar_mul_batch_buckets_gpu", "msm_buckets_resident"):
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
    h_el = lambda a, b, m, n, wb, o, x: lib.d377_batch_bucket_msm(None, a, b, m, n, wb, o, x)                          # noqa: E731
    h_en = lambda a, b, m, n, wb, o, x, s: lib.d377_batch_bucket_msm_encoded(None, a, b, m, n, wb, o, x, s)             # noqa: E731
    r_el = lambda a, b, m, n, wb, o, x: lib.d377_batch_bucket_msm_resident(None, 0, None, a, b, m, n, wb, o, x)        # noqa: E731
    r_en = lambda a, b, m, n, wb, o, x, s: lib.d377_batch_bucket_msm_encoded_resident(None, 0, None, a, b, m, n, wb, o, x, s)   # noqa: E731
    for el, en in ((h_el, h_en), (r_el, r_en)):
        for m in (0, (1 << 20) + 1):                             # m first: a bad window_bits, null buffers and a null context alike
            for n in (2, 0):
                msg = _refused(lib, el(None, None, m, n, 99, None, None), "m")
                assert "m = %d" % m in msg and "d377_msm" in msg
                assert "m = %d" % m in _refused(lib, en(None, None, m, n, 99, None, None, None), "m")
        for wb in (-1, 1, 3, 17, 18):                            # then window_bits
            for n in (2, 0):
                assert "window_bits = %d" % wb in _refused(lib, el(None, None, 9, n, wb, None, None), "window_bits")
                assert "window_bits = %d" % wb in _refused(lib, en(None, None, 1 << 20, n, wb, None, None, None), "window_bits")
        for m, wb in ((9, 0), (1 << 20, 16), (1, 4)):            # then the buffers, then the context
            _refused(lib, el(None, _p(k), m, 2, wb, _p(enc), None), "xyzt")
            _refused(lib, el(_p(pts), None, m, 2, wb, _p(enc), None), "scalar32")
            _refused(lib, el(_p(pts), _p(k), m, 2, wb, None, None), "enc32_out")
            _refused(lib, en(None, _p(k), m, 2, wb, _p(enc), None, _p(st)), "enc32")
            _refused(lib, en(_p(raw), _p(k), m, 2, wb, _p(enc), None, None), "status")
            _refused(lib, el(_p(pts), _p(k), m, 2, wb, _p(enc), None), "ctx")
            _refused(lib, en(_p(raw), _p(k), m, 2, wb, _p(enc), None, _p(st)), "ctx")
            _refused(lib, el(None, None, m, 0, wb, None, None), "ctx")      # n = 0 excuses the null buffers, not the null context
    plan = lambda n, m, wb: lib.d377_bucket_msm_plan(None, 0, n, m, wb, None, None, None, None)                        # noqa: E731
    assert "m = 0" in _refused(lib, plan(4, 0, 99), "m")
    assert "window_bits = 17" in _refused(lib, plan(4, 9, 17), "window_bits")
    _refused(lib, plan(4, 9, 0), "ctx")
    assert (enc == 0xA5).all() and (st == 0xA5).all()
