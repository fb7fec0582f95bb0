"""The resident forms of the sums over registered bases (d377_batch_*_resident, d377_check_base_index_resident), without a GPU.

The six symbols are defined by the built library, declared by their header and bound; none ends in `_dev`.  With a null context
each call refuses a term count out of range with D377_ERR_ARG and a message that names the argument -- those checks come
before ctx is looked at, so they need no device.  The index verdict's predicate and its rule for combining two verdicts
(decaf377_amd/csrc/index_verdict.hpp) are compiled into a stand-alone host program (tests/cpp/resident_sums.cpp with
-DINDEX_VERDICT_HOST), which folds them in the kernel's order -- striding lanes, the lanes of a wave, the waves -- and is
compared with numpy; the same program is built with -fsanitize=address,undefined and run as an ordinary program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
PROG = os.path.join(ROOT, "tests", "cpp", "resident_sums.cpp")
NAMES = ["d377_batch_fixed_msm_resident", "d377_batch_fixed_long_msm_resident", "d377_batch_fixed_msm_indexed_resident", "d377_batch_msm_mixed_resident",
         "d377_batch_msm_mixed_encoded_resident", "d377_check_base_index_resident"]
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
NONE = (1 << 64) - 1
ERR_ARG = -2


@pytest.fixture(scope="module")
def libpath():
    from decaf377_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build_native()
    return _native.LIB_PATH


@pytest.fixture(scope="module")
def lib(libpath):
    from decaf377_amd import _native
    return _native.load()


def test_the_library_defines_the_symbols(libpath):
    """The resident forms are declared in include/decaf377_amd_resident.h, which decaf377_amd.h includes; the library defines
    them, _native.RESIDENT_EXPORTS lists exactly them and binds them, and rust/src/ffi_resident.rs is the tool's current output."""
    import importlib.util
    import re
    from decaf377_amd import _native
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "decaf377_amd_resident.h")).read()
    declared = sorted(set(re.findall(r"\b(d377_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES) == sorted(_native.RESIDENT_EXPORTS)
    assert '#include "decaf377_amd_resident.h"' in open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    lib = _native.load()
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi_resident.rs")).read()
    for name, ret, params in gen.prototypes(header):
        assert name in defined and not name.endswith("_dev"), name
        assert len(getattr(lib, name).argtypes) == len(params), name
        assert "pub fn %s(%s) -> c_int;" % (name, ", ".join("%s: %s" % (p, gen.rust_type(t)) for t, p in params)) in ffi, name


def _refused(lib, rc, word):
    assert rc == ERR_ARG
    msg = lib.d377_last_error().decode()
    assert word in msg.split(), msg                              # the argument is named as a word of its own
    return msg


@pytest.mark.parametrize("v", [0, 9])
def test_mixed_calls_refuse_v_without_a_device(lib, v):
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    _refused(lib, lib.d377_batch_msm_mixed_resident(None, 0, None, 1, p, p, 1, p, p, v, 1, p, None, None), "v")
    _refused(lib, lib.d377_batch_msm_mixed_encoded_resident(None, 0, None, 1, p, p, 1, p, p, v, 1, p, None, p, None), "v")


@pytest.mark.parametrize("t", [0, 65])
def test_mixed_and_indexed_calls_refuse_t_without_a_device(lib, t):
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    _refused(lib, lib.d377_batch_msm_mixed_resident(None, 0, None, 1, p, p, t, p, p, 1, 1, p, None, None), "t")
    _refused(lib, lib.d377_batch_msm_mixed_encoded_resident(None, 0, None, 1, p, p, t, p, p, 1, 1, p, None, p, None), "t")
    _refused(lib, lib.d377_batch_fixed_msm_indexed_resident(None, 0, None, 1, p, p, t, 1, p, None, None), "t")


def test_good_ranges_get_as_far_as_the_null_context(lib):
    """... so the refusals above are the range checks' and not a blanket one: with the ranges good the next complaint is ctx."""
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = [lib.d377_batch_msm_mixed_resident(None, 0, None, 1, p, p, 1, p, p, 1, 1, p, None, None),
             lib.d377_batch_fixed_msm_indexed_resident(None, 0, None, 1, p, p, 1, 1, p, None, None),
             lib.d377_batch_fixed_msm_resident(None, 0, None, 1, p, 1, p, None),
             lib.d377_batch_fixed_long_msm_resident(None, 0, None, 1, p, 1, p, None),
             lib.d377_check_base_index_resident(None, 0, None, 1, p, 1, p)]
    assert calls == [ERR_ARG] * len(calls)
    assert "ctx" in lib.d377_last_error().decode()


# ---- the verdict's logic on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs():
    """The host program plain and under AddressSanitizer + UBSan, compiled side by side."""
    outs = {"plain": os.path.join(ROOT, "tests", "cpp", "index_verdict_host"), "san": os.path.join(ROOT, "tests", "cpp", "index_verdict_host_san")}
    cmds = {"plain": ["g++", "-O2", "-std=c++17", "-DINDEX_VERDICT_HOST", "-I" + CSRC, PROG, "-o", outs["plain"]],
            "san": ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DINDEX_VERDICT_HOST",
                    "-I" + CSRC, PROG, "-o", outs["san"]]}
    srcs = [PROG, os.path.join(CSRC, "index_verdict.hpp"), os.path.join(CSRC, "fq29.hpp")]
    stale = lambda o: not os.path.exists(o) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs)
    procs = {k: subprocess.Popen(cmds[k]) for k in cmds if stale(outs[k])}
    for k, pr in procs.items():
        assert pr.wait() == 0, cmds[k]
    return outs


def _numpy_verdict(idx, m):
    idx = np.asarray(idx, dtype=np.int64)
    bad = np.nonzero((idx != -1) & ((idx < 0) | (idx >= m)))[0]
    return (len(bad), int(bad[0]) if len(bad) else NONE)


def _cases(m):
    """name -> array.  The values the issue names, around both ends of 0 .. m-1 and of int; an empty array and one without an
    offender; the first offender at position 0, at 63 and 64 (the last lane of a wave and the first of the next) and at the last."""
    edge = [INT_MIN, -2, -1, 0, m - 1, m, INT_MAX]
    rng = np.random.default_rng(m)
    clean = rng.integers(-1, m, 300).tolist()
    cases = {"edges": edge, "edges reversed": edge[::-1], "empty": [], "clean": clean, "all absent": [-1] * 130}
    for pos in (0, 63, 64, len(clean) - 1):
        a = list(clean)
        a[pos] = m
        cases["first at %d" % pos] = a
        b = list(a)
        for later, val in ((pos + 1, -2), (len(clean) - 1, INT_MAX), (200, INT_MIN)):
            if later < len(b) and later > pos:
                b[later] = val
        cases["first at %d, more behind" % pos] = b
    cases["random"] = rng.choice(np.array(edge + [1 % m, m // 2]), 1000).tolist()
    # the table holds what its names claim, by the reference the program is compared with
    assert _numpy_verdict(cases["edges"], m) == (4, 0) and _numpy_verdict(cases["edges reversed"], m) == (4, 0)
    assert _numpy_verdict(cases["empty"], m) == (0, NONE) and _numpy_verdict(cases["clean"], m) == (0, NONE)
    for pos in (0, 63, 64, len(clean) - 1):
        assert _numpy_verdict(cases["first at %d" % pos], m) == (1, pos)
        assert _numpy_verdict(cases["first at %d, more behind" % pos], m)[1] == pos
    return cases


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("m", [1, 64, 4096])
def test_verdict_logic_against_numpy(programs, build, m):
    for name, idx in _cases(m).items():
        want = _numpy_verdict(idx, m)
        for lanes in (64, 256):                                  # one wave; four waves, so the waves' verdicts are joined too
            r = subprocess.run([programs[build], str(m), str(lanes)], input=" ".join(str(x) for x in idx), capture_output=True,
                               text=True, timeout=60)
            assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
            got = tuple(int(x) for x in r.stdout.split())
            assert got == want, (m, name, lanes, got, want)
