"""The one long sum over 8- and 16-byte scalars (d377_msm_short, include/decaf377_amd_short_msm.h) without a GPU.

tests/host_sim/msm_short_sim.cpp is a host build of decaf377_amd/csrc/msm_plan.hpp alone: the window shape for any bit count
(win_shape_bits), the digits as msm.hip's short loader forms them, and msm_plan with the bit count as an input.  Checked here:
the shape for 252 bits is field for field what win_shape(c) was; the short shapes tile their bits; the digits sum back to the
scalar exactly (Python integers); short plans satisfy every invariant tests/test_msm_plan_host.py asserts of a plan; the C ABI
refuses bad arguments in the documented order before any device is touched; the sim runs clean under the sanitizers as a
stand-alone program."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import test_msm_plan_host as plan_host
from _msm_short_cases import BITS, edge_scalars, pick_window, py_shape, records
from _oracle import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
SRC = os.path.join(SIM_DIR, "msm_short_sim.cpp")
NAMES = {"d377_msm_short": 7, "d377_msm_short_encoded": 8, "d377_msm_short_dev": 9, "d377_msm_short_encoded_dev": 10,
         "d377_msm_short_plan": 7}
ERR_ARG = -2
PLAN_N = (1, 64, 4097, 1 << 16, 1 << 20, 3 << 20)


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def _sources():
    return [SRC] + [os.path.join(CSRC, f) for f in ("msm_plan.hpp", "launch_plan.hpp", "curve.hpp")]


@pytest.fixture(scope="module")
def sim():
    lib = os.path.join(SIM_DIR, "libmsm_short_sim.so")
    if _stale(lib, _sources()):
        tmp = "%s.%d" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=8", "-I" + CSRC, SRC, "-o", tmp])
        os.replace(tmp, lib)
    L = ctypes.CDLL(lib)
    L.sim_short_digits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


def shape(sim, B, c):
    out = np.zeros(3 + 128, np.int32)
    sim.sim_short_shape(B, c, _p(out))
    cw, W, nwide = (int(v) for v in out[:3])
    return cw, W, nwide, [int(v) for v in out[3:3 + W]], [int(v) for v in out[67:67 + W]]


# ---- the shape -----------------------------------------------------------------------------------------------------------
def test_shape_for_252_bits_is_the_parent_win_shape(sim):
    for c in range(4, 19):
        new, old, today = np.zeros(3 + 128, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        sim.sim_short_shape(252, c, _p(new))
        sim.sim_parent_shape(c, _p(old))
        sim.sim_win_shape(c, _p(today))
        assert list(new[:3]) == list(old) == list(today) and old[0] == c, c
        assert old[1] == -(-252 // c) and old[2] == old[1] - (old[1] * c - 252), c


@pytest.mark.parametrize("nbytes", [8, 16])
def test_short_shapes_tile_their_bits(sim, nbytes):
    B = BITS[nbytes]
    assert sim.sim_short_scalar_bits(nbytes) == B
    for c in range(4, 17):
        cw, W, nwide, first, width = shape(sim, B, c)
        assert (cw, W, nwide, first, width) == py_shape(B, c), (B, c)     # the restatement the GPU test builds its edge scalars from
        assert W == -(-B // c) and W <= 63, (B, c)               # k_msm_final's table of cached sums holds 63 records
        assert cw == -(-B // W) and cw <= c and nwide == W - (W * cw - B) and 1 <= nwide <= W, (B, c)
        assert first[0] == 0 and all(first[w] + width[w] == first[w + 1] for w in range(W - 1)) and first[-1] + width[-1] == B, (B, c)
        assert set(width) <= {cw, cw - 1} and width == [cw] * nwide + [cw - 1] * (W - nwide), (B, c)


def test_window_counts_of_the_issue(sim):
    want = {65: (6, 5, 5), 129: (11, 10, 9), 252: (21, 18, 16)}
    for B, ws in want.items():
        assert tuple(shape(sim, B, c)[1] for c in (12, 14, 16)) == ws, B
    assert shape(sim, 65, 16)[:3] == (13, 5, 5) and shape(sim, 129, 16)[:3] == (15, 9, 3)


# ---- the digits ------------------------------------------------------------------------------------------------------------
def digits_of(sim, ks, nbytes, c):
    rec = records(ks, nbytes)
    dg = np.zeros((len(ks), 64), np.int32)
    sim.sim_short_digits(_p(rec), nbytes, len(ks), c, _p(dg))
    return dg


@pytest.mark.parametrize("nbytes", [8, 16])
def test_digits_sum_back_to_the_scalar(sim, nbytes):
    bits = 8 * nbytes
    rng = np.random.default_rng(377 + nbytes)
    for c in range(4, 17):
        _, W, _, first, width = shape(sim, BITS[nbytes], c)
        edges = edge_scalars(nbytes, c)
        rnd = [int.from_bytes(rng.bytes(nbytes), "little") for _ in range(1 << 12)]
        ks = edges + rnd
        dg = digits_of(sim, ks, nbytes, c)
        assert not dg[:, 63].any(), c                            # no carry is left after the top window
        assert not dg[:, W:63].any(), c
        lim = np.array([1 << (wd - 1) for wd in width])
        assert (np.abs(dg[:, :W]) <= lim).all(), c
        assert (dg[:, :W - 1] < lim[:W - 1]).all() and (dg[:, W - 1] >= 0).all(), c   # wrapped below the top; the top is not
        for k, row in zip(ks, dg):
            assert sum(int(d) << b for d, b in zip(row[:W], first)) == k, (c, hex(k))
        # the edges do what they are there for
        top = digits_of(sim, [(1 << bits) - 1], nbytes, c)[0]
        assert top[0] == -1 and not top[1:W - 1].any() and top[W - 1] == 1 << (bits - first[-1]), c
        hit = np.zeros(W, bool)
        for row in digits_of(sim, edges, nbytes, c):
            hit |= np.abs(row[:W]) == lim
        assert hit.all(), c                                      # every window met +-2^(width-1), the top one from 2^bits - 1


# ---- the plan --------------------------------------------------------------------------------------------------------------
def _plan(sim, n, c, bits, cus=256, span_blocks=4):
    return plan_host.Plan(sim, [n, c, cus, span_blocks, -1, -1, -1, -1, -1, -1, bits])


@pytest.fixture(scope="module")
def short_plans(sim):
    return {(nbytes, n): _plan(sim, n, pick_window(n), BITS[nbytes]) for nbytes in (8, 16) for n in PLAN_N}


def test_short_plans_satisfy_the_plan_invariants(sim, short_plans):
    plans = list(short_plans.values())
    plans += [_plan(sim, n, c, B, cus) for B in BITS.values() for c in range(4, 17) for n, cus in ((300, 256), (70000, 8), (1 << 20, 304))]
    assert len(plan_host.REGIONS) == plans[0].nregions
    plan_host.test_plan_invariants(plans)                       # regions disjoint and inside the workspace, folds, tree, WSM_CAP, lanes
    for p in plans:
        f, k = p.f, p.k
        assert not f["ws_mid"] and f["ws_depth"] <= 15           # (the WSM_CAP rule is about a middle level: short shapes never have one)
        assert not f["wide_digits"] and f["nb"] - 1 <= 1 << 15   # int16 digits whatever the width asked for


@pytest.mark.parametrize("nbytes", [8, 16])
def test_short_plan_follows_the_narrowed_width_and_needs_no_more_workspace(sim, short_plans, nbytes):
    for n in PLAN_N:
        c = pick_window(n)
        p, full = short_plans[(nbytes, n)], _plan(sim, n, c, 252)
        cw, W, nwide, _, _ = shape(sim, BITS[nbytes], c)
        consts = np.zeros(16, np.int32)
        out, off, sz, fold = np.zeros(64, np.int64), np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(48, np.int32)
        sim.sim_msm_plan(_p(np.array([n, c, 256, 4, -1, -1, -1, -1, -1, -1, BITS[nbytes]], np.int64)), _p(out), _p(off), _p(sz), _p(fold), _p(consts))
        assert consts[10] == cw                                  # the shape carries c'
        assert (p.f["W"], p.f["nwide"]) == (W, nwide) and p.f["nb"] == (1 << (cw - 1)) + 1 and p.f["ws_depth"] == cw - 1, (nbytes, n)
        assert p.f["W"] < full.f["W"] and p.f["bytes"] <= full.f["bytes"], (nbytes, n)
    # 252 bits through the same entry point is the plan of today
    for case in plan_host.CASES[::7]:
        a, b = plan_host.Plan(sim, case["in"] + [252]), case
        assert a.out == b["out"] and a.off == b["off"] and a.sz == b["sz"], case["in"]


# ---- the C ABI, without a device -------------------------------------------------------------------------------------------
def test_symbols_declared_defined_bound_and_in_the_rust_block(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd_short_msm.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.SHORT_MSM_EXPORTS)
    main = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    assert main.index('#include "decaf377_amd_segmented_sums.h"') < main.index('#include "decaf377_amd_short_msm.h"')
    others = (set(_native.EXPORTS) | set(_native.RESIDENT_EXPORTS) | set(_native.LONG_SUMS_EXPORTS) | set(_native.BUCKET_SUMS_EXPORTS)
              | set(_native.RAGGED_SUMS_EXPORTS) | set(_native.SEGMENTED_SUMS_EXPORTS))
    assert not set(NAMES) & others
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_short_msm.rs")).read()
    protos = gen.prototypes(header)
    assert sorted(p[0] for p in protos) == sorted(NAMES)
    for name, ret, params in protos:
        assert name in defined, name
        assert len(params) == NAMES[name] and len(getattr(lib, name).argtypes) == NAMES[name], name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name
    gpu_rs = open(os.path.join(ROOT, "rust", "src", "gpu.rs")).read()
    assert "pub mod ffi_short_msm;" in gpu_rs
    for fn in ("vartime_multiscalar_mul_short_gpu", "msm_short_resident"):
        assert re.search(r"pub (unsafe )?fn %s(<[^>]*>)?\(" % fn, gpu_rs), fn


def _refused(lib, rc, word):
    assert rc == ERR_ARG
    msg = lib.d377_last_error().decode()
    assert re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(word), msg), (word, msg)   # named as a word of its own
    return msg


def test_refusals_come_in_the_documented_order_without_a_device(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    pts, raw, k = np.zeros((4, 16), np.uint64), np.zeros((4, 32), np.uint8), np.zeros((4, 16), np.uint8)
    enc, st = np.full(32, 0xA5, np.uint8), np.full(4, 0xA5, np.uint8)
    h_el = lambda a, b, sb, n, o, x: lib.d377_msm_short(None, a, b, sb, n, o, x)                                         # noqa: E731
    h_en = lambda a, b, sb, n, o, x, s: lib.d377_msm_short_encoded(None, a, b, sb, n, o, x, s)                            # noqa: E731
    d_el = lambda a, b, sb, n, o, x: lib.d377_msm_short_dev(None, 0, None, a, b, sb, n, o, x)                            # noqa: E731
    d_en = lambda a, b, sb, n, o, x, s: lib.d377_msm_short_encoded_dev(None, 0, None, a, b, sb, n, o, x, s)               # noqa: E731
    for el, en in ((h_el, h_en), (d_el, d_en)):
        for sb in (0, 4, 12, 32):                                # scalar_bytes first: null buffers and a null context alike
            for n in (4, 0, 1 << 31):
                assert "got %d" % sb in _refused(lib, el(None, None, sb, n, None, None), "scalar_bytes")
                assert "got %d" % sb in _refused(lib, en(None, None, sb, n, None, None, None), "scalar_bytes")
        for sb in (8, 16):                                       # then the buffers and n, then the context
            _refused(lib, el(None, _p(k), sb, 4, _p(enc), None), "xyzt")
            _refused(lib, el(_p(pts), None, sb, 4, _p(enc), None), "scalars")
            _refused(lib, el(_p(pts), _p(k), sb, 4, None, None), "enc32_out")
            _refused(lib, en(None, _p(k), sb, 4, _p(enc), None, _p(st)), "enc32")
            _refused(lib, en(_p(raw), _p(k), sb, 4, _p(enc), None, None), "status")
            _refused(lib, el(_p(pts), _p(k), sb, 1 << 31, _p(enc), None), "n")
            _refused(lib, en(_p(raw), _p(k), sb, 1 << 31, _p(enc), None, _p(st)), "n")
            _refused(lib, el(_p(pts), _p(k), sb, 4, _p(enc), None), "context")      # good arguments get as far as the device check
            _refused(lib, en(_p(raw), _p(k), sb, 4, _p(enc), None, _p(st)), "context")
            _refused(lib, el(None, None, sb, 0, _p(enc), None), "context")          # n = 0 excuses the null inputs, not the null context
    plan = lambda n, sb: lib.d377_msm_short_plan(None, 0, n, sb, None, None, None)                                       # noqa: E731
    assert "got 32" in _refused(lib, plan(4, 32), "scalar_bytes")
    _refused(lib, plan(1 << 31, 8), "n")
    _refused(lib, plan(4, 16), "context")
    assert (enc == 0xA5).all() and (st == 0xA5).all()


def test_python_binding_refuses_scalars_of_another_shape():
    from decaf377_amd.engine import Context
    for shape_, dt in (((4, 8), np.uint8), ((4, 16), np.uint8), ((4,), np.uint64), ((4, 2), np.uint64), ((4, 1), np.int64)):
        a, nb = Context._short_scalars(np.zeros(shape_, dt), 4, None)
        assert nb * 4 == a.nbytes
    for shape_, dt in (((4, 32), np.uint8), ((4, 12), np.uint8), ((5, 8), np.uint8), ((4, 3), np.uint64), ((4, 8), np.uint16)):
        with pytest.raises(ValueError, match="msm_short scalars"):
            Context._short_scalars(np.zeros(shape_, dt), 4, None)


# ---- the sanitizers: the sim as its own program ----------------------------------------------------------------------------
def test_sim_runs_clean_under_the_sanitizers():
    exe = os.path.join(SIM_DIR, "msm_short_san")
    if _stale(exe, _sources()):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DMSM_SHORT_SIM_MAIN", "-DD377_FB_BITS=8", "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MSM_SHORT_SIM_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
