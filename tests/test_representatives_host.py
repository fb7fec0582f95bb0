"""Every representative of a group element on the CPU: the records tests/_representatives.py builds are valid Elements, the
oracle does not tell them apart, and the host simulation of the device functions (tests/host_sim/sim.cpp) gives the oracle's
values on every one of them -- in the plain build and in the -DD377_BOUNDS build, where every primitive asserts its
precondition, so that the records scaled by -1 (Z = q - 1, every limb near the top of the canonical range) walk every asserted
bound.  tests/test_representatives_gpu.py runs the same records through the kernels.

The expected value is always the oracle's on the PLAIN record (Z = 1) of the same group element.

Simulation entry points and what they take: sim_compress, sim_compress_assisted, sim_to_affine_raw, sim_raw_forms,
sim_group_misc and sim_batch_msm (m = 1, 3, 8) take every kind of _representatives.KINDS and every form of the identity class;
none had to be left out.  sim_to_affine_raw is compared with the oracle's to_affine of the SAME record (the twin kinds
legitimately give (-x, -y)) and, for the scaled kinds, limb for limb with to_affine of the plain record."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _representatives as rp
from _batch_msm_long_cases import oracle_fold
from test_host_sim import CSRC, SIM_DIR, sim  # noqa: F401  (sim: the fixture)

COUNT = 64


@pytest.fixture(scope="module")
def reps(oracle):
    return rp.build(oracle, 9100, COUNT)


def test_builder_emits_valid_elements(oracle, reps):
    """Canonical limbs, Z != 0, T Z = X Y and the curve equation, in integers, for every record of every kind and of the identity
    class; the kinds are what their names say; the scalars' halves take both parities."""
    for kind in rp.KINDS:
        rp.assert_valid(oracle, reps.kinds[kind], kind)
    rp.assert_valid(oracle, reps.ident, "identity class")
    one = 1
    A = rp.to_ints(oracle, reps.A)
    assert all(a[2] == one for a in A)
    for kind in rp.KINDS:
        for (X, Y, Z, T), (x, y, _, t) in zip(rp.to_ints(oracle, reps.kinds[kind]), A):
            s = -1 if kind in rp.TWIN_KINDS else 1              # (X, Y, Z, T) = l (s x, s y, 1, t)
            if kind != "proj":                                   # (the Elligator record may be the twin of what its encoding decodes to)
                assert (X - s * Z * x) % rp.Q == 0 and (Y - s * Z * y) % rp.Q == 0 and (T - Z * t) % rp.Q == 0, kind
            if kind in ("affine", "twin"):
                assert Z == 1, kind
            elif kind in ("minus", "twin_minus"):
                assert Z == rp.Q - 1, kind
            else:
                assert Z not in (0, 1, rp.Q - 1), kind
    for j, (X, Y, Z, T) in enumerate(rp.to_ints(oracle, reps.ident)):
        form = rp.IDENTITY_FORMS[j % 6]
        assert X == 0 and T == 0 and Y in (Z, rp.Q - Z), form
        assert (Y == Z) == (form in ("canonical", "scaled", "p_minus_p")), form
        assert (Z == 1) == (form in ("canonical", "torsion")), form
    assert [int.from_bytes(bytes(k), "little") for k in reps.scalars[:7]] == list(rp.FIXED_SCALARS)
    odd = rp.half_is_odd(reps.scalars[7:])
    assert 4 * odd.sum() >= odd.size and 4 * (~odd).sum() >= odd.size
    assert list(rp.half_is_odd(np.stack([rp.scalar_bytes(v) for v in (0, 1, 2, rp.R - 1)]))) == [False, ((rp.R + 1) // 2) & 1 == 1, True,
                                                                                               ((rp.R - 1) // 2) & 1 == 1]


def test_layouts_hold_what_they_promise(oracle, reps):
    for n in (1, 63, 64, 65, 257):
        recs, plain, names = rp.plant(reps, *rp.mixed(reps, n))
        where = sorted({p for p in rp.PLANTS + (n - 1,) if p < n})
        assert [i for i, s in enumerate(names) if s.startswith("identity")] == where
        assert oracle.is_identity(recs)[where].all() and oracle.is_identity(plain)[where].all()
        assert oracle.eq_xyzt(recs, plain).all()
        for w in range(0, n - 63, 64):                           # every full wave holds every kind
            assert set(rp.KINDS) <= set(names[w:w + 64])
    lay = rp.layouts(reps, 257)
    assert sorted(lay) == ["all_identity_but_one", "mixed_planted", "one_identity"]
    assert list(np.nonzero(oracle.is_identity(lay["all_identity_but_one"][0]) == 0)[0]) == [128]
    assert list(np.nonzero(oracle.is_identity(lay["one_identity"][0]))[0]) == [70]
    for recs, plain in lay.values():
        assert oracle.eq_xyzt(recs, plain).all()
        rp.assert_valid(oracle, recs[:80])
    L, LA, _ = rp.mixed(reps, 65)
    Rr, RA = rp.right_operands(oracle, reps, 65)
    assert oracle.eq_xyzt(Rr, RA).all()
    s, d = oracle.add_xyzt(LA, RA), oracle.sub_xyzt(LA, RA)
    assert oracle.is_identity(s)[14:21].all() and oracle.is_identity(d)[7:14].all()       # P + (-P)', P - P'
    # P - twin(P) and twin(P) - P, where exactly one side is of a twin kind: the point of order 2, as records
    tw = [i for i in range(7, 14) if (rp.KINDS[i % 7] in rp.TWIN_KINDS) != (rp.KINDS[(i + 1) % 7] in rp.TWIN_KINDS)]
    diff = rp.to_ints(oracle, oracle.sub_xyzt(L[tw], Rr[tw]))
    assert tw == [10, 13] and all(X == 0 and T == 0 and Y == rp.Q - Z for X, Y, Z, T in diff)


def test_oracle_is_representative_independent(oracle, reps):
    """compress, compress_to_field, eq, is_identity, scalar_mul + compress, msm, add / sub / double / neg + compress: the same on every
    kind as on the plain records; the identity class gives the all-zero Encoding and is_identity = 1."""
    A, k = reps.A, reps.scalars
    B = np.roll(A, 1, axis=0)
    want = {"compress": oracle.compress(A), "field": oracle.compress_to_field(A), "ident": oracle.is_identity(A),
            "mul": oracle.compress(oracle.scalar_mul_xyzt(A, k)), "msm": oracle.msm(A, k)[0],
            "add": oracle.compress(oracle.add_xyzt(A, B)), "sub": oracle.compress(oracle.sub_xyzt(A, B)),
            "rsub": oracle.compress(oracle.sub_xyzt(B, A)), "double": oracle.compress(oracle.double_xyzt(A)),
            "neg": oracle.compress(oracle.neg_xyzt(A))}
    assert not want["ident"].any()
    for kind in rp.KINDS:
        P = reps.kinds[kind]
        got = {"compress": oracle.compress(P), "field": oracle.compress_to_field(P), "ident": oracle.is_identity(P),
               "mul": oracle.compress(oracle.scalar_mul_xyzt(P, k)), "msm": oracle.msm(P, k)[0],
               "add": oracle.compress(oracle.add_xyzt(P, B)), "sub": oracle.compress(oracle.sub_xyzt(P, B)),
               "rsub": oracle.compress(oracle.sub_xyzt(B, P)), "double": oracle.compress(oracle.double_xyzt(P)),
               "neg": oracle.compress(oracle.neg_xyzt(P))}
        for name in want:
            assert (got[name] == want[name]).all(), (kind, name)
        assert oracle.eq_xyzt(P, A).all() and oracle.eq_xyzt(A, P).all(), kind
        assert (oracle.eq_xyzt(P, B) == oracle.eq_xyzt(A, B)).all(), kind
        assert (oracle.eq_xyzt(P, oracle.neg_xyzt(A)) == oracle.eq_xyzt(A, oracle.neg_xyzt(A))).all(), kind
    I = reps.ident
    kk = reps.scalars[np.arange(I.shape[0]) % COUNT]
    assert oracle.is_identity(I).all() and not oracle.compress(I).any() and not oracle.compress_to_field(I).any()
    assert not oracle.compress(oracle.scalar_mul_xyzt(I, kk)).any() and not oracle.msm(I, kk)[0].any()
    for a in range(6):
        assert oracle.eq_xyzt(I, np.roll(I, a, axis=0)).all()
    assert (oracle.compress(oracle.add_xyzt(I, A[:I.shape[0]])) == want["compress"][:I.shape[0]]).all()


# ---- the host simulation ------------------------------------------------------------------------------------------------------------
def _sim_cases(oracle, reps):
    """name -> (P, Q2, k, plain P, plain Q2).  All kinds mixed with the plants at 0, 63, 64 and n - 1 (65 records: two rounds of
    the assisted compressor and a third of one record), the two extreme layouts, and one array per kind (24 records: a whole run of
    one kind through every shared inversion and every Straus table)."""
    cases = {}
    n = 65
    P, PA, _ = rp.mixed(reps, n)
    P, PA, _ = rp.plant(reps, P, PA)
    Q2, QA = rp.right_operands(oracle, reps, n)
    cases["mixed_planted"] = (P, Q2, reps.scalars[np.arange(n) % COUNT], PA, QA)
    P, PA = rp.all_identity_but_one(reps, n)
    cases["all_identity_but_one"] = (P, Q2, np.roll(reps.scalars, 3, axis=0)[np.arange(n) % COUNT], PA, QA)
    P, PA = rp.one_identity(reps, n, where=40)
    cases["one_identity"] = (P, Q2, reps.scalars[np.arange(n) % COUNT], PA, QA)
    m = 24
    for j, kind in enumerate(rp.KINDS):
        other = rp.KINDS[(j + 3) % len(rp.KINDS)]
        cases[kind] = (reps.kinds[kind][:m], np.roll(reps.kinds[other], 1, axis=0)[:m], np.roll(reps.scalars, j, axis=0)[:m], reps.A[:m],
                       np.roll(reps.A, 1, axis=0)[:m])
    m = reps.ident.shape[0]
    cases["identity_class"] = (reps.ident, np.roll(reps.ident, 1, axis=0), reps.scalars[1:m + 1], np.tile(reps.ident[0], (m, 1)),
                               np.tile(reps.ident[0], (m, 1)))
    return {name: tuple(np.ascontiguousarray(a) for a in c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def sim_cases(oracle, reps):
    return _sim_cases(oracle, reps)


def _check_sim(oracle, name, case, got):
    P, Q2, k, PA, QA = case
    n = P.shape[0]
    enc = oracle.compress(PA)
    assert (got["compress"] == enc).all(), (name, np.nonzero((got["compress"] != enc).any(1))[0][:8])
    assert (got["compress_assisted"] == enc).all(), (name, np.nonzero((got["compress_assisted"] != enc).any(1))[0][:8])
    assert (got["to_affine"] == oracle.to_affine(P)).all(), name
    if name in rp.SCALED_KINDS + ("affine",):
        assert (got["to_affine"] == oracle.to_affine(PA)).all(), name
    sums = oracle.add_xyzt(PA, QA)
    for key in ("raw_add", "misc_add"):
        assert oracle.eq_xyzt(got[key], sums).all() and (oracle.compress(got[key]) == oracle.compress(sums)).all(), (name, key)
        assert (got[key] == oracle.add_xyzt(P, Q2)).all(), (name, key)            # the reference's formulas on the records as given
        rp.assert_valid(oracle, got[key][:16], name)
    dbl = oracle.double_xyzt(PA)
    assert oracle.eq_xyzt(got["raw_double"], dbl).all() and (oracle.compress(got["raw_double"]) == oracle.compress(dbl)).all(), name
    assert (got["raw_double"] == oracle.double_xyzt(P)).all(), name
    for key in ("raw_neg", "misc_neg"):
        assert (got[key] == oracle.neg_xyzt(P)).all() and oracle.eq_xyzt(got[key], oracle.neg_xyzt(PA)).all(), (name, key)
    assert got["raw_neg_ok"].all() and got["raw_f_ok"].all(), name
    assert (got["raw_eq"] == oracle.eq_xyzt(PA, QA)).all(), name
    for m in rp.SIM_MSM_M:
        terms = n // m * m
        want = oracle_fold(oracle, PA[:terms], k[:terms], m)[0]
        assert (got["msm%d" % m] == want).all(), (name, m, np.nonzero((got["msm%d" % m] != want).any(1))[0][:8])
    if name in ("identity_class",):
        assert not got["compress"].any() and not got["msm3"].any() and got["raw_eq"].all()


def test_host_simulation_on_every_representative(sim, oracle, sim_cases):  # noqa: F811
    """The plain build, in this process."""
    for name, case in sim_cases.items():
        _check_sim(oracle, name, case, rp.run_sim(sim, case[0], case[1], case[2]))


def test_host_simulation_with_bounds_on_every_representative(oracle, sim_cases, tmp_path):
    """The -DD377_BOUNDS build that test_static_bounds makes (built here the same way if it is missing or stale), in a child
    process: a violated precondition aborts it.  The same records, the same comparisons."""
    lib = os.path.join(SIM_DIR, "libd377_sim_bounds.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("sim.cpp", "launch_plan_sim.inc")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s_) > os.path.getmtime(lib) for s_ in srcs):
        subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-fPIC", "-shared", "-DD377_BOUNDS", "-DD377_FB_BITS=8", "-I" + CSRC,
                               os.path.join(SIM_DIR, "sim.cpp"), "-o", lib])
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, **{name + "." + key: a for name, c in sim_cases.items() for key, a in zip(("P", "Q", "k"), c[:3])})
    r = subprocess.run([sys.executable, rp.__file__, lib, inp, out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "REPRESENTATIVES_SIM_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = np.load(out)
    for name, case in sim_cases.items():
        _check_sim(oracle, name, case, {key.split(".", 1)[1]: res[key] for key in res.files if key.split(".", 1)[0] == name})
