"""Mixed sums, registered bases plus variable points (d377_batch_msm_mixed / _encoded), without a GPU.

The per-sum body the lane kernel runs (decaf377_amd/csrc/mixed_sum.hpp: straus_sum over the variable points,
ge_fixed_msm_indexed_w8 over the registered bases with the kernel's term loader, one ge_add, the square-root-free compressor)
is compiled for the host (tests/host_sim/msm_mixed_sim.cpp) and checked, byte for byte, against the oracle's fold of scalar
multiplications and additions, with planted rows: the special scalars on both sides, a Z = 0 record, every fixed term absent
(the variable sum alone, against sim_batch_msm), every variable scalar zero (the fixed sum alone, against fx_msm_indexed), and
the join doubling and cancelling.  The same source is built with -DD377_BOUNDS (every limb precondition asserted, run in a
child process because a violated one aborts) and, through tests/cpp/msm_mixed.cpp, as a stand-alone program under
AddressSanitizer and UBSan.  The ABI checks need no device: both symbols are declared, exported and bound, neither is a `_dev`
entry point, and bad arguments are refused in the documented order before any device is touched.

Where every fixed term is absent the Element record is the variable sum as a group element (eq_xyzt) but not its limbs: the
join still adds the walk's representative of the identity, (0 : c : c : 0), which scales the coordinates."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _sums_support import (R, _p, host_bases as _bases, host_scalars as _scalars, indexed_fold_by_scalar_mul as _fixed_fold,
                           scalar_bytes as _scalar_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
SRC = os.path.join(SIM_DIR, "msm_mixed_sim.cpp")
PROG = os.path.join(ROOT, "tests", "cpp", "msm_mixed.cpp")
NAMES = {"d377_batch_msm_mixed": 11, "d377_batch_msm_mixed_encoded": 12}
M = 5
N = 40
SHAPES = [(1, 1), (1, 2), (3, 2), (8, 7)]                        # (v, t)
ZROW, ABSENT, VZERO, DOUBLE, CANCEL = 20, 21, 22, 23, 24           # the planted sums
SAN_SHAPE = (3, 2)


def _stale(out, extra=()):
    srcs = [SRC, os.path.join(SIM_DIR, "fixed_bases_indexed_sim.cpp"), os.path.join(SIM_DIR, "fixed_bases_sim.cpp"),
            os.path.join(SIM_DIR, "sim.cpp")] + list(extra) + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope="module")
def built():
    """The three host builds, compiled side by side: the simulation plain and with -DD377_BOUNDS, and the sanitized program."""
    outs = {"sim": os.path.join(SIM_DIR, "libd377_mx_sim.so"), "bounds": os.path.join(SIM_DIR, "libd377_mx_sim_bounds.so"),
            "san": os.path.join(SIM_DIR, "msm_mixed_san")}
    cmds = {"sim": ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DD377_FB_BITS=12", "-I" + CSRC, SRC, "-o", outs["sim"]],
            "bounds": ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-DD377_BOUNDS", "-DD377_FB_BITS=8", "-I" + CSRC, SRC,
                       "-o", outs["bounds"]],
            # (-fwhole-program: everything but main is local, so the simulations this program never calls are dropped before
            # they are instrumented)
            "san": ["g++", "-O1", "-g", "-fwhole-program", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DMSM_MIXED_HOST", "-DD377_FB_BITS=8", "-I" + CSRC, PROG, "-o", outs["san"]]}
    procs = {k: subprocess.Popen(cmds[k]) for k in cmds if _stale(outs[k], (PROG,) if k == "san" else ())}
    for k, p in procs.items():
        assert p.wait() == 0, cmds[k]
    return outs


def _bind(L):
    L.fx_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fx_msm_indexed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.mx_msm_mixed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                               ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.mx_msm_small.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def sim(built):
    return _bind(ctypes.CDLL(built["sim"]))


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


@pytest.fixture(scope="module")
def bases(oracle):
    """The five bases of test_fixed_bases_indexed_host.py: a random point, the identity, GENERATOR, Z != 1, the torsion twin."""
    return _bases(oracle, np.random.default_rng(55), M)


def make_case(oracle, bases, v, t):
    """N sums of t fixed and v variable terms with the planted rows -> dict of arrays (index rows, scalars, points)."""
    rng = np.random.default_rng(100 * v + t)
    fk = _scalars(rng, N, t)                                     # 0, 1, r - 1, r and 2^256 - 1 among them, on both sides
    vk = _scalars(rng, N, v)
    idx = rng.integers(0, M, (N, t)).astype(np.int32)
    idx[4, 0] = -1                                               # absent first and last
    idx[6, t - 1] = -1
    idx[2] = 1 % M                                               # one index repeated
    pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (N * v, 32), dtype=np.uint8)), dtype=np.uint64)
    pts[5 * v] = oracle.identity_xyzt()
    pts[ZROW * v, 8:12] = 0                                      # a record with Z = 0: counts as the identity
    idx[ABSENT] = -1                                             # no fixed term at all: the variable sum alone
    vk[VZERO * v:(VZERO + 1) * v] = 0                            # every variable scalar 0: the fixed sum alone
    kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
    for row, other in ((DOUBLE, kv), (CANCEL, R - kv)):          # P_0 = B_0 meets the fixed term on base 0
        idx[row] = -1
        idx[row, t - 1] = 0
        fk[row * t + t - 1] = _scalar_bytes(kv)
        vk[row * v:(row + 1) * v] = 0
        vk[row * v] = _scalar_bytes(other)
        pts[row * v] = bases[0]
    return {"idx": np.ascontiguousarray(idx), "fk": fk, "vk": vk, "pts": pts}


def oracle_sums(oracle, bases, c, v, t):
    """sum_j fk * B_idx + sum_p vk * P by the oracle's scalar multiplications and additions -> (encodings, records)."""
    pts = c["pts"].copy()
    dead = ~pts[:, 8:12].any(1)
    pts[dead] = oracle.identity_xyzt()
    terms = oracle.scalar_mul_xyzt(pts, c["vk"]).reshape(N, v, 16)
    acc = _fixed_fold(oracle, bases, c["idx"], c["fk"])[1]
    for p in range(v):
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(terms[:, p]))
    return oracle.compress(acc), acc


@pytest.fixture(scope="module")
def cases(oracle, bases):
    out = {}
    for v, t in SHAPES:
        c = make_case(oracle, bases, v, t)
        out[(v, t)] = (c,) + oracle_sums(oracle, bases, c, v, t)
    return out


def run_mixed(L, c, v, t, n=N):
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.zeros((n, 16), np.uint64)
    assert L.mx_msm_mixed(_p(c["idx"]), _p(c["fk"]), t, _p(c["pts"]), _p(c["vk"]), v, n, _p(enc), _p(el)) == 0
    return enc, el


@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("v,t", SHAPES)
def test_walk_matches_oracle_fold(sim, oracle, bases, cases, bits, v, t):
    c, want_enc, want_el = cases[(v, t)]
    assert sim.fx_build(_p(bases), M, bits) == 0
    enc, el = run_mixed(sim, c, v, t)
    assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
    assert oracle.eq_xyzt(el, want_el).all()
    assert (oracle.compress(el) == enc).all()
    # every fixed term absent: d377_batch_msm_small's lane on the variable part
    small = np.zeros((N, 32), np.uint8)
    assert sim.mx_msm_small(_p(c["pts"]), _p(c["vk"]), v, N, _p(small)) == 0
    assert (enc[ABSENT] == small[ABSENT]).all()
    dead = ~c["pts"][ABSENT * v:(ABSENT + 1) * v, 8:12].any(1)
    vpts = np.where(dead[:, None], oracle.identity_xyzt()[None, :], c["pts"][ABSENT * v:(ABSENT + 1) * v])
    vterms = oracle.scalar_mul_xyzt(np.ascontiguousarray(vpts, dtype=np.uint64), np.ascontiguousarray(c["vk"][ABSENT * v:(ABSENT + 1) * v]))
    vsum = np.ascontiguousarray(vterms[:1])
    for p in range(1, v):
        vsum = oracle.add_xyzt(vsum, np.ascontiguousarray(vterms[p:p + 1]))
    assert oracle.eq_xyzt(el[ABSENT:ABSENT + 1], vsum).all()    # the record: the variable sum as a group element (not its limbs)
    # every variable scalar zero: d377_batch_fixed_msm_indexed's lane on the fixed part
    fenc = np.zeros((N, 32), np.uint8)
    fel = np.zeros((N, 16), np.uint64)
    assert sim.fx_msm_indexed(_p(c["idx"]), _p(c["fk"]), t, N, _p(fenc), _p(fel)) == 0
    assert (enc[VZERO] == fenc[VZERO]).all() and oracle.eq_xyzt(el[VZERO:VZERO + 1], fel[VZERO:VZERO + 1]).all()
    # the join doubling (k B_0 + k B_0) and cancelling (k B_0 + (r - k) B_0): the unified addition takes both
    k2 = c["fk"][DOUBLE * t + t - 1][None, :]
    twice = oracle.scalar_mul_xyzt(bases[:1], k2)
    assert (enc[DOUBLE] == oracle.compress(oracle.add_xyzt(twice, twice))[0]).all()
    assert not enc[CANCEL].any() and oracle.is_identity(el[CANCEL:CANCEL + 1]).all()


def test_bounds_build_walks_every_case(built, bases, cases, tmp_path):
    """-DD377_BOUNDS: a violated limb precondition aborts.  Every shape over both comb widths, the planted rows included -- the
    ge_add of two product-carried halves among them."""
    work = str(tmp_path / "mixed_cases.npz")
    arrays = {"bases": bases}
    for (v, t), (c, want_enc, _) in cases.items():
        for k, a in c.items():
            arrays["%s_%d_%d" % (k, v, t)] = a
        arrays["enc_%d_%d" % (v, t)] = want_enc
    np.savez(work, **arrays)
    code = r"""
import ctypes, sys, numpy as np
L = ctypes.CDLL(sys.argv[1]); z = np.load(sys.argv[2])
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
L.mx_msm_mixed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
L.fx_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
bases = np.ascontiguousarray(z["bases"])
for bits in (8, 12):
    assert L.fx_build(p(bases), bases.shape[0], bits) == 0
    for v, t in %r:
        a = {k: np.ascontiguousarray(z["%%s_%%d_%%d" %% (k, v, t)]) for k in ("idx", "fk", "pts", "vk", "enc")}
        n = a["idx"].shape[0]
        enc = np.zeros((n, 32), np.uint8); el = np.zeros((n, 16), np.uint64)
        assert L.mx_msm_mixed(p(a["idx"]), p(a["fk"]), t, p(a["pts"]), p(a["vk"]), v, n, p(enc), p(el)) == 0
        assert (enc == a["enc"]).all(), (bits, v, t)
print("BOUNDS_OK")
""" % (SHAPES,)
    r = subprocess.run([sys.executable, "-c", code, built["bounds"], work], capture_output=True, text=True)
    assert r.returncode == 0 and "BOUNDS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_sanitized_program_runs_clean(built, oracle, bases, cases, tmp_path):
    """The simulation as a stand-alone program under AddressSanitizer and UBSan: it finishes clean and writes the oracle's sums."""
    v, t = SAN_SHAPE
    c, want_enc, want_el = cases[SAN_SHAPE]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in (bases, c["idx"], c["fk"], c["pts"], c["vk"]):
            f.write(a.tobytes())
    r = subprocess.run([built["san"], fin, fout, str(M), "8", str(v), str(t), str(N)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "MSM_MIXED_HOST_OK" in r.stdout
    raw = np.fromfile(fout, np.uint8)
    enc, el = raw[:N * 32].reshape(N, 32), raw[N * 32:].view(np.uint64).reshape(N, 16)
    assert (enc == want_enc).all()
    assert oracle.eq_xyzt(np.ascontiguousarray(el), want_el).all()


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(libpath):
    from decaf377_amd import _native
    header = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert re.search(r"#define D377_BATCH_MSM_MIXED_MAX_VAR 8\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    lib = _native.load()
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert name in _native.EXPORTS, name
        assert not name.endswith("_dev") and name + "_dev" not in exported
        assert re.search(r"\bfn %s\(" % name, ffi), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert len(_native.EXPORTS) == 102


def test_refuses_bad_arguments_without_a_device_in_order(libpath):
    from decaf377_amd import _native
    lib = _native.load()
    err = lambda: lib.d377_last_error().decode()
    n, t, v = 2, 2, 3
    idx = np.zeros((n, t), np.int32)
    fk = np.zeros((n * t, 32), np.uint8)
    pts = np.zeros((n * v, 16), np.uint64)
    encs = np.zeros((n * v, 32), np.uint8)
    vk = np.zeros((n * v, 32), np.uint8)
    enc = np.full((n, 32), 0xA5, np.uint8)
    el = np.full((n, 16), 0xA5A5A5A5A5A5A5A5, np.uint64)
    st = np.full((n * v,), 0xA5, np.uint8)
    f, g = lib.d377_batch_msm_mixed, lib.d377_batch_msm_mixed_encoded
    for bad_v in (0, 9):                                         # v first: everything else is bad as well
        assert f(None, 1, None, None, 0, None, None, bad_v, n, None, None) == -2
        assert re.search(r"\bv\b", err()) and "d377_batch_fixed_msm_indexed" in err()
    for bad_t in (0, 65):                                        # then t
        assert f(None, 1, None, None, bad_t, None, None, v, n, None, None) == -2
        assert re.search(r"\bt\b", err()) and "d377_batch_msm_small" in err()
    args = [_p(idx), _p(fk), t, _p(pts), _p(vk), v, n, _p(enc), _p(el)]
    for pos, word in ((0, "base_index"), (1, "fixed_scalar32"), (3, "xyzt"), (4, "var_scalar32"), (7, "enc32_out")):
        a = list(args)
        a[pos] = None
        assert f(None, 1, *a) == -2
        assert word in err(), (word, err())
    assert f(None, 1, *args) == -2                              # every buffer given: the context
    assert "ctx" in err()
    a = list(args)
    a[8] = None                                                  # xyzt_out is optional
    assert f(None, 1, *a) == -2 and "ctx" in err()
    assert f(None, 1, None, None, t, None, None, v, 0, None, None) == -2    # n = 0 excuses the null buffers, not the null context
    assert "ctx" in err()
    eargs = [_p(idx), _p(fk), t, _p(encs), _p(vk), v, n, _p(enc), _p(el), _p(st)]
    for pos, word in ((3, "enc32"), (9, "status")):
        a = list(eargs)
        a[pos] = None
        assert g(None, 1, *a) == -2
        assert word in err(), (word, err())
    assert g(None, 1, *eargs) == -2 and "ctx" in err()
    assert (enc == 0xA5).all() and (el == 0xA5A5A5A5A5A5A5A5).all() and (st == 0xA5).all()
