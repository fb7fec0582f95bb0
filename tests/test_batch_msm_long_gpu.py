"""Many multiscalar sums of 9 .. 4096 terms on the MI355X (d377_batch_msm_long[_encoded]) against the oracle's fold, on both
routes of the chains (a wave / a lane per partial sum), against the library's own oracle-checked calls, and through the
C++ mirror.  The planted cases and the oracle's fold are those of tests/_batch_msm_long_cases.py."""

import numpy as np
import pytest

from _batch_msm_long_cases import make_case, oracle_fold, plan
from _sums_support import build_and_run_cpp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    assert c.health()[0] == 0 and c.health()[2] == 0             # after the file's tests: no lane set claimed, nobody gave up
    c.close()


def _wave_max(ctx):
    """The most partial sums that run a wave each: four per SIMD (batch_msm_launch's rule)."""
    import torch
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count


def _ran_another_route(a, b):
    """Which route ran is not reported by the library; its witness is the Element records.  A wave runs its chain in the
    lane-spread form (row_ops.hpp) and a lane in the per-lane form (straus.hpp, with the dead padded slots), so the two
    routes leave DIFFERENT extended representatives of the same sums: records that are equal byte for byte came from one
    route run twice."""
    return (a != b).any()


def _check(ctx, oracle, n, m, encoded, seed):
    rng = np.random.default_rng(seed)
    pts, k, info = make_case(oracle, rng, n, m, encoded=encoded)
    want_enc, want_el, want_st = oracle_fold(oracle, pts, k, m)
    got = ctx.msm_long(pts, k, m, elements=True)
    enc, el = got[0], got[1]
    assert (enc == want_enc).all(), (n, m, np.nonzero((enc != want_enc).any(1))[0][:8])
    assert oracle.eq_xyzt(el, want_el).all(), (n, m)
    if encoded:
        g, b = plan(m)
        assert g * b == m or info["dead"][m - 1]                 # an invalid Encoding sits in a padded last group
        assert (got[2] == want_st).all(), (n, m)
        e2, s2 = ctx.msm_long(pts, k, m)                         # without Element records
        assert (e2 == enc).all() and (s2 == want_st).all()
    else:
        assert (ctx.msm_long(pts, k, m) == enc).all()
        for s in info["identity"]:
            assert not enc[s].any()
    return pts, k, got


@pytest.mark.parametrize("encoded", [False, True], ids=["elements", "encodings"])
@pytest.mark.parametrize("n,m", [(3, 9), (3, 17), (2, 129), (1, 2049), (1, 4096)])
def test_wave_route(ctx, oracle, n, m, encoded):
    assert n * plan(m)[0] <= _wave_max(ctx)
    _check(ctx, oracle, n, m, encoded, 10 * m + n)


@pytest.mark.parametrize("encoded", [False, True], ids=["elements", "encodings"])
@pytest.mark.parametrize("n,m", [(37, 9), (37, 17), (5, 129)])
def test_lane_route_forced(ctx, oracle, n, m, encoded):
    with ctx.tuning(tiny_max=0):                                 # wave_max = 0: every call takes the lanes
        pts, k, got = _check(ctx, oracle, n, m, encoded, 20 * m + n)
    assert n * plan(m)[0] <= _wave_max(ctx)                      # the same call at default tuning takes the waves
    assert _ran_another_route(got[1], ctx.msm_long(pts, k, m, elements=True)[1])


@pytest.mark.parametrize("encoded", [False, True], ids=["elements", "encodings"])
@pytest.mark.parametrize("shape", ["9", "100"])
def test_lane_route_default_tuning(ctx, oracle, shape, encoded):
    """n g just above the wave route's limit and no multiple of 64: the last wave has idle lanes.  On 256 CUs (limit 4 096):
    (2100, 9) -> 4 200 partial sums, (330, 100) -> 4 290."""
    m = int(shape)
    g = plan(m)[0]
    n = _wave_max(ctx) // g + (52 if m == 9 else 15)
    if (n * g) % 64 == 0:
        n += 1
    assert n * g > _wave_max(ctx) and (n * g) % 64
    _check(ctx, oracle, n, m, encoded, 30 * m)


@pytest.mark.parametrize("encoded", [False, True], ids=["elements", "encodings"])
@pytest.mark.parametrize("n,m", [(11, 9), (6, 65), (3, 129)])
def test_both_routes_agree(ctx, oracle, n, m, encoded):
    rng = np.random.default_rng(40 * m + n)
    pts, k, _ = make_case(oracle, rng, n, m, encoded=encoded)
    wave = ctx.msm_long(pts, k, m, elements=True)
    with ctx.tuning(tiny_max=0):
        lane = ctx.msm_long(pts, k, m, elements=True)
    assert (wave[0] == lane[0]).all()
    assert oracle.eq_xyzt(wave[1], lane[1]).all()
    assert _ran_another_route(wave[1], lane[1])                  # ... and it was two routes that agreed
    if encoded:
        assert (wave[2] == lane[2]).all()


@pytest.mark.parametrize("m", [8, 3])
def test_short_sums_forward_to_the_small_sums(ctx, oracle, m):
    rng = np.random.default_rng(m)
    n = 50
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8))
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    raw = oracle.compress(pts)
    raw[4::9, 31] |= 0x40
    a, b = ctx.msm_long(pts, k, m, elements=True), ctx.msm_small(pts, k, m, elements=True)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()         # the same bytes, Element records included
    a, b = ctx.msm_long(raw, k, m, elements=True), ctx.msm_small(raw, k, m, elements=True)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def test_consistent_with_one_long_sum_per_call(ctx, oracle):
    rng = np.random.default_rng(300)
    n, m = 4, 300
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8))
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    enc, el = ctx.msm_long(pts, k, m, elements=True)
    for s in range(n):
        e1, x1, _ = ctx.msm(pts[s * m:(s + 1) * m], k[s * m:(s + 1) * m])
        assert (enc[s] == e1).all()
        assert oracle.eq_xyzt(el[s:s + 1], x1.reshape(1, 16)).all()


def test_consistent_with_the_composition(ctx, oracle):
    """(64, 16) against msm_small on the 128 groups of 8 and one add."""
    rng = np.random.default_rng(16)
    n, m = 64, 16
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8))
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    enc, el = ctx.msm_long(pts, k, m, elements=True)
    _, halves = ctx.msm_small(pts, k, 8, elements=True)          # [2 n, 16]: sum s is records 2 s and 2 s + 1
    total = ctx.add(np.ascontiguousarray(halves[0::2]), np.ascontiguousarray(halves[1::2]))
    assert (ctx.compress(total) == enc).all()
    assert oracle.eq_xyzt(total, el).all()


def test_device_listed_twice_slices_the_sums(ctx, oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(517)
    n, m = 5, 17
    c2 = d.Context([0, 0], comb_lazy=True)
    try:
        for encoded in (False, True):
            pts, k, _ = make_case(oracle, rng, n, m, encoded=encoded)
            want_enc, want_el, want_st = oracle_fold(oracle, pts, k, m)
            got = c2.msm_long(pts, k, m, elements=True)
            assert (got[0] == want_enc).all()
            assert oracle.eq_xyzt(got[1], want_el).all()         # Element records and statuses in place
            if encoded:
                assert (got[2] == want_st).all()
        assert c2.health(0)[0] == 0 and c2.health(1)[0] == 0
    finally:
        c2.close()


def test_torch_tensors_are_staged_through_host_memory(ctx, oracle):
    import torch
    rng = np.random.default_rng(77)
    n, m = 3, 17
    pts, k, _ = make_case(oracle, rng, n, m)
    want = ctx.msm_long(pts, k, m, elements=True)
    dev = torch.device("cuda:0")
    got = ctx.msm_long(torch.from_numpy(pts.view(np.int64)).to(dev), torch.from_numpy(k).to(dev), m, elements=True)
    assert got[0].device.type == "cuda"
    assert (got[0].cpu().numpy() == want[0]).all()
    assert (got[1].cpu().numpy().view(np.uint64) == want[1]).all()


def test_cpp_mirror_batch_msm_long():
    """tests/cpp/batch_msm_long.cpp: msm_long through include/decaf377_amd.hpp against the fold of the mirror's own * and +."""
    build_and_run_cpp("batch_msm_long", "CPP_BATCH_MSM_LONG_OK")
