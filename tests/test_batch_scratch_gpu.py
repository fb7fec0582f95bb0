"""The Straus table scratch of a device is ONE area that three units grow through one function (batch_host.hpp:
straus_scratch_reserve): the small sums (m tables per lane), the mixed sums (v tables) and the long sums (a group's b tables).
On one fresh context, with the wave routes off so that every call takes its lane kernel, the three grow the area in turn and
every result is compared with the oracle; then the first call runs again in the larger area and must give the same bytes,
and the mixed sums run on a context that lists the device twice (the shared slicer in front of the shared reserve).

n = 257 is two workgroups of 256 lanes with one live lane in the second.  The cases are those of
tests/test_msm_mixed_gpu.py and tests/_batch_msm_long_cases.py."""
import numpy as np
import pytest

from _batch_msm_long_cases import make_case, oracle_fold, plan
from _sums_support import Fold, join as _join, mixed_case as _case, var_terms as _var_terms

pytestmark = pytest.mark.gpu

N = 257


def _same(oracle, step, got, want_enc, want_el, want_status=None):
    enc, el = got[0], got[1]
    assert (enc == want_enc).all(), (step, np.nonzero((enc != want_enc).any(1))[0][:8])
    assert oracle.eq_xyzt(el, want_el).all(), step
    assert (oracle.compress(el) == enc).all(), step
    if want_status is not None:
        assert (got[2] == want_status).all(), step


def test_three_units_grow_one_table_scratch(oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(2718)

    # the cases and the oracle's results, before any call
    p1 = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (N, 32), dtype=np.uint8)), dtype=np.uint64)
    p1[5, 8:12] = 0                                              # a record with Z = 0: the identity
    k1 = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    want1 = oracle_fold(oracle, p1, k1, 1)
    assert not want1[0][5].any()

    v, t, m = 3, 1, 2
    bases, idx, fk, pts, vk = _case(oracle, v, t, m, N)
    good = pts.copy()
    good[~good[:, 8:12].any(1)] = oracle.identity_xyzt()
    encs = oracle.compress(good)
    bad = np.zeros(N * v, bool)
    bad[::5] = True
    encs[bad] = 0xFF                                             # above q: no canonical Encoding
    want2 = _join(oracle, Fold(oracle, bases).records(idx, fk), _var_terms(oracle, pts, vk, N, v), ~bad.reshape(N, v))

    n3, m3 = 37, 17
    assert plan(m3)[1] > v                                       # a group's terms exceed the mixed sums' v: step 3 really grows
    p3, k3, info3 = make_case(oracle, rng, n3, m3, encoded=True)
    assert info3["dead"].any()
    want3 = oracle_fold(oracle, p3, k3, m3)

    ctx = d.Context([0], comb_lazy=True)
    twice = None
    try:
        with ctx.tuning(tiny_max=0):                             # no wave route: every call takes its lane kernel
            got1 = ctx.msm_small(p1, k1, 1, elements=True)       # 1: the first allocation, one table per lane
            _same(oracle, 1, got1, want1[0], want1[1])
            with ctx.fixed_bases(bases, comb_bits=8) as fb:      # 2: grown by the mixed unit to three tables
                got2 = fb.msm_mixed(idx, fk, encs, vk, elements=True)
            _same(oracle, 2, got2, want2[0], want2[1], bad.astype(np.uint8))
            got3 = ctx.msm_long(p3, k3, m3, elements=True)       # 3: grown by the long unit to a group's six
            _same(oracle, 3, got3, want3[0], want3[1], want3[2])
            again = ctx.msm_small(p1, k1, 1, elements=True)      # 4: no growth; the larger area gives the same bytes
            assert (again[0] == got1[0]).all() and (again[1] == got1[1]).all()
            _same(oracle, 4, again, want1[0], want1[1])
        twice = d.Context([0, 0], comb_lazy=True)                # 5: two slices, each through the shared reserve
        with twice.fixed_bases(bases, comb_bits=8) as fb:
            got5 = fb.msm_mixed(idx, fk, encs, vk, elements=True)
        for a, b in zip(got5, got2):
            assert (a == b).all()
        _same(oracle, 5, got5, want2[0], want2[1], bad.astype(np.uint8))
        for c, devs in ((ctx, (0,)), (twice, (0, 1))):
            for dev in devs:
                claimed, _, gave_up = c.health(dev)
                assert claimed == 0 and gave_up == 0
    finally:
        if twice is not None:
            twice.close()
        ctx.close()
