"""Fixed-base sums over up to 4096 bases, cut into segments (d377_fixed_bases_create_long / d377_batch_fixed_long_msm /
d377_fixed_long_msm_plan) without a GPU.

The cut (decaf377_amd/csrc/fixed_msm_long_plan.hpp) is checked for every m, and the walk the device runs -- one segment of
consecutive bases per lane through the table wrapper that offsets the comb index, partial sums as Element records, fold levels
of 16 records per lane, the chunked compressor -- is compiled for the host (tests/host_sim/fixed_msm_long_sim.cpp, once with
-DD377_FB_BITS=12 and once with 8) and checked, byte for byte, against the oracle's fold of scalar multiplications and
additions.  The same source is built as a stand-alone program under AddressSanitizer and UBSan and run on the m = 101 case.
The ABI checks need no device either: the symbols are declared, exported, bound and in the Rust FFI, none is a `_dev` entry
point, and bad arguments are refused in the documented order before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _fixed_msm_long_cases import levels, make_bases, make_scalars, oracle_fold, plan
from _oracle import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
SRC = os.path.join(SIM_DIR, "fixed_msm_long_sim.cpp")
NAMES = ("d377_fixed_bases_create_long", "d377_batch_fixed_long_msm", "d377_fixed_long_msm_plan")
# (m, n, L) -> (b, g): one segment (m = 1; n >= L), two segments of 5 and 4 bases, single-base segments with two and three
# fold levels, and segments of 4 bases whose last holds one
CASES = {(1, 6, 1000): (1, 1), (5, 6, 6): (5, 1), (9, 4, 8): (5, 2), (17, 3, 51): (1, 17), (101, 2, 52): (4, 26),
         (257, 2, 514): (1, 257)}
SAN_CASE = (101, 2, 52)


def _stale(out):
    srcs = [SRC, os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope="module")
def built():
    """The three host builds, compiled side by side: the simulation with D377_FB_BITS = 12 and 8, and the sanitized program."""
    outs = {12: os.path.join(SIM_DIR, "libd377_fml_sim12.so"), 8: os.path.join(SIM_DIR, "libd377_fml_sim8.so"),
            "san": os.path.join(SIM_DIR, "fixed_msm_long_sim_san")}
    cmds = {b: ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=%d" % b, "-I" + CSRC, SRC, "-o", outs[b]] for b in (12, 8)}
    # (-fwhole-program: everything but main is local, so the simulations this program never calls are dropped before they are
    # instrumented -- a third of the compile time)
    cmds["san"] = ["g++", "-O1", "-g", "-fwhole-program", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                   "-DFML_SIM_MAIN", "-DD377_FB_BITS=8", "-I" + CSRC, SRC, "-o", outs["san"]]
    procs = {k: subprocess.Popen(cmds[k]) for k in cmds if _stale(outs[k])}
    for k, p in procs.items():
        assert p.wait() == 0, cmds[k]
    return outs


def _load(path):
    L = ctypes.CDLL(path)
    L.sim_init.restype = ctypes.c_int
    assert L.sim_init() == 0
    L.fml_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.fml_seg_min.restype = ctypes.c_size_t
    L.fml_levels.argtypes = [ctypes.c_size_t]
    L.fml_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fml_msm_long.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def sims(built):
    return {b: _load(built[b]) for b in (12, 8)}


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


@pytest.fixture(scope="module")
def cases(oracle):
    """Bases, scalars and the oracle's sums of every case, made once."""
    out = {}
    for (m, n, L), (b, g) in CASES.items():
        rng = np.random.default_rng(100 * m + n)
        bases = make_bases(oracle, rng, m, b)
        k = make_scalars(rng, n, m, g, b)
        out[(m, n, L)] = (bases, k) + oracle_fold(oracle, bases, k, n, m)
    return out


def test_plan_properties_for_every_m(sims):
    sim = sims[12]
    seg_min = int(sim.fml_seg_min())
    out = np.zeros(2 + 2 * 4096, np.uint64)
    for L in (65536, 131072):
        for n in (1, 2, 63, 4097, L - 1, L, L + 1):
            for m in range(1, 4097):
                sim.fml_plan(m, n, L, _p(out))
                g, b = int(out[0]), int(out[1])
                assert (g, b) == plan(m, n, L, seg_min), (m, n, L)
                first, count = out[2:2 + 2 * g:2].astype(np.int64), out[3:3 + 2 * g:2].astype(np.int64)
                assert (count >= 1).all() and (count <= b).all(), (m, n, L)          # no segment is empty
                assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == m, (m, n, L)
                if n >= L:
                    assert g == 1, (m, n, L)
                assert n * g >= min(L, n * -(-m // seg_min)) - n, (m, n, L)           # the cut fills the chip where the sum is long enough
                assert sim.fml_levels(g) <= 3 and sim.fml_levels(g) == levels(g), (m, n, L)


def test_plan_of_the_cases(sims):
    out = np.zeros(2 + 2 * 4096, np.uint64)
    for (m, n, L), (b, g) in CASES.items():
        sims[8].fml_plan(m, n, L, _p(out))
        assert (int(out[1]), int(out[0])) == (b, g), (m, n, L)
    sims[8].fml_plan(9, 4, 8, _p(out))
    assert list(out[:6].astype(int)) == [2, 5, 0, 5, 5, 4]                            # segments of 5 and 4 bases
    sims[8].fml_plan(101, 2, 52, _p(out))
    assert list(out[2 + 2 * 25:2 + 2 * 26].astype(int)) == [100, 1]                   # the last segment has one base
    assert [levels(g) for g in (1, 2, 17, 26, 257)] == [0, 1, 2, 2, 3]


@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "m%d-n%d" % c[:2])
def test_segment_walk_matches_oracle_fold(sims, oracle, cases, bits, case):
    m, n, L = case
    b, g = CASES[case]
    bases, k, want_enc, want_el = cases[case]
    sim = sims[bits]
    assert sim.fml_build(_p(bases), m, bits) == 0
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    gb = np.zeros(2, np.uint64)
    assert sim.fml_msm_long(_p(k), n, L, _p(enc), _p(el), _p(gb)) == 0
    assert (int(gb[1]), int(gb[0])) == (b, g)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    assert not enc[n - 1].any() and oracle.is_identity(el[n - 1:]).all()              # every scalar 0: the all-zero Encoding


def test_sanitized_program_runs_clean(built, oracle, cases, tmp_path):
    """The simulation as a stand-alone program under AddressSanitizer and UBSan, on the m = 101 case: it finishes clean and
    writes the oracle's sums."""
    m, n, L = SAN_CASE
    bases, k, want_enc, want_el = cases[SAN_CASE]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(bases.tobytes())
        f.write(k.tobytes())
    r = subprocess.run([built["san"], fin, fout, str(m), str(n), str(L), "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.split() == [str(CASES[SAN_CASE][1]), str(CASES[SAN_CASE][0])]
    raw = np.fromfile(fout, np.uint8)
    enc, el = raw[:n * 32].reshape(n, 32), raw[n * 32:].view(np.uint64).reshape(n, 16)
    assert (enc == want_enc).all()
    assert oracle.eq_xyzt(np.ascontiguousarray(el), want_el).all()


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_exported_bound_and_in_the_rust_ffi(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert re.search(r"#define D377_FIXED_BASES_LONG_MAX 4096\b", header)
    assert re.search(r"\bD377_FIXED_BASES_LONG_MAX\b[^;\n]*=\s*4096\b", ffi)
    nm = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    lib = _native.load()
    for name, nargs in zip(NAMES, (5, 6, 6)):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert name in _native.EXPORTS, name
        assert not name.endswith("_dev")
        assert re.search(r"\bfn %s\(" % name, ffi), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert not [n for n in _native.EXPORTS if "fixed" in n and n.endswith("_dev")]


@pytest.mark.parametrize("m,bits,word", [(0, 12, "m"), (4097, 12, "m"), (1, 7, "comb_bits"), (2, 14, "comb_bits"), (3, 23, "comb_bits")])
def test_create_long_refuses_bad_arguments_without_a_device(libpath, m, bits, word):
    from decaf377_amd import _native
    lib = _native.load()
    rec = np.zeros((max(m, 1), 16), np.uint64)
    h = ctypes.c_int64(-1)
    assert lib.d377_fixed_bases_create_long(None, _p(rec), m, bits, ctypes.byref(h)) == -2    # D377_ERR_ARG
    assert not h.value
    assert re.search(r"\b%s\b" % word, lib.d377_last_error().decode())


def test_null_pointers_are_refused_in_order_without_a_device(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    err = lambda: lib.d377_last_error().decode()
    rec = np.zeros((1, 16), np.uint64)
    h = ctypes.c_int64(0)
    assert lib.d377_fixed_bases_create_long(None, None, 1, 12, None) == -2                    # xyzt before handle_out before ctx
    assert "xyzt" in err()
    assert lib.d377_fixed_bases_create_long(None, _p(rec), 1, 12, None) == -2
    assert "handle_out" in err()
    assert lib.d377_fixed_bases_create_long(None, _p(rec), 1, 0, ctypes.byref(h)) == -2       # comb_bits 0 is the default, 12
    assert "ctx" in err()
    assert lib.d377_fixed_bases_create_long(None, None, 0, 7, None) == -2                     # m before everything else
    assert re.search(r"\bm\b", err())
    k = np.zeros((1, 32), np.uint8)
    enc = np.full((1, 32), 0xA5, np.uint8)
    assert lib.d377_batch_fixed_long_msm(None, 1, _p(k), 1, _p(enc), None) == -2
    assert "ctx" in err() and (enc == 0xA5).all()
    g, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.d377_fixed_long_msm_plan(None, 1, 1, 0, ctypes.byref(g), ctypes.byref(b)) == -2
    assert "ctx" in err()


def test_short_create_still_stops_at_64(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    rec = np.zeros((65, 16), np.uint64)
    h = ctypes.c_int64(-1)
    assert lib.d377_fixed_bases_create(None, _p(rec), 65, 16, ctypes.byref(h)) == -2
    assert not h.value and re.search(r"\bm\b", lib.d377_last_error().decode())
