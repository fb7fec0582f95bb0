"""Fixed-base sums over up to 4096 bases on the MI355X (d377_fixed_bases_create_long / d377_batch_fixed_long_msm /
d377_fixed_long_msm_plan), against the oracle and against the library's own oracle-checked operations.

The cuts are chosen with FixedBases.long_plan, so they happen on whatever CU count the box has: single-base segments with one,
two and three fold levels (few sums over many bases), segments of several bases whose last is shorter, and the one segment per
sum that is d377_batch_fixed_msm's kernel.  The case builders and the oracle's folds are in tests/_fixed_msm_long_cases.py,
shared with tests/test_fixed_msm_long_host.py."""

import numpy as np
import pytest

from _fixed_msm_long_cases import KINDS, SPECIAL, levels, make_bases, make_scalars, oracle_fold, plan
from _sums_support import Fold, _p, build_and_run_cpp, random_bases as _random_bases, scalar_bytes

pytestmark = pytest.mark.gpu


def _tree_fold(oracle, terms):
    """[n, m, 16] records -> their n sums by the oracle's additions, halving m every round."""
    while terms.shape[1] > 1:
        half = terms.shape[1] // 2
        s = oracle.add_xyzt(np.ascontiguousarray(terms[:, :half].reshape(-1, 16)),
                            np.ascontiguousarray(terms[:, half:2 * half].reshape(-1, 16))).reshape(terms.shape[0], half, 16)
        terms = np.concatenate([s, terms[:, 2 * half:]], axis=1)
    return np.ascontiguousarray(terms[:, 0])


def _oracle_sums(oracle, bases, k, n, m):
    terms = oracle.scalar_mul_xyzt(np.ascontiguousarray(np.tile(bases, (n, 1))), k).reshape(n, m, 16)
    acc = _tree_fold(oracle, terms)
    return oracle.compress(acc), acc


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lanes(ctx, oracle):
    """L, the device's resident lanes: the first n at which a sum over two bases is left in one piece."""
    with ctx.fixed_bases_long(_random_bases(oracle, np.random.default_rng(1), 2), comb_bits=8) as fb:
        lo, hi = 1, 1 << 24
        assert fb.long_plan(hi)[0] == 1 and fb.long_plan(lo)[0] == 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fb.long_plan(mid)[0] == 1:
                hi = mid
            else:
                lo = mid
    assert hi % 512 == 0                                         # CUs x WAVES_PER_SIMD x BLOCK
    return hi


@pytest.fixture(scope="module")
def big(ctx, oracle):
    """4096 bases at 8 bits (2.2 GB), registered once for the module."""
    bases = _random_bases(oracle, np.random.default_rng(4096), 4096)
    fb = ctx.fixed_bases_long(bases, comb_bits=8)
    assert fb.info()[:2] == (4096, 8) and 2.1e9 < fb.info()[2] < 2.3e9
    yield bases, fb
    fb.close()


@pytest.mark.parametrize("bits,m,n", [(8, 65, 3), (12, 100, 1), (8, 257, 2), (8, 4096, 2)])
def test_short_n_long_m_against_the_oracle(ctx, oracle, lanes, big, bits, m, n):
    rng = np.random.default_rng(1000 * bits + m)
    if m == 4096:
        bases, fb = big
    else:
        bases = _random_bases(oracle, rng, m)
        fb = ctx.fixed_bases_long(bases, comb_bits=bits)
    try:
        g, b = fb.long_plan(n)
        assert (g, b) == plan(m, n, lanes) == (m, 1)              # single-base segments
        assert levels(g) == {65: 2, 100: 2, 257: 3, 4096: 3}[m]
        k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
        k[0] = scalar_bytes(SPECIAL[2])
        k[m - 1] = scalar_bytes(SPECIAL[4])
        enc, el = fb.msm_long(k, elements=True)
        want_enc, want_el = _oracle_sums(oracle, bases, k, n, m)
        assert (enc == want_enc).all()
        assert oracle.eq_xyzt(el, want_el).all()
        assert (oracle.compress(el) == enc).all()
        assert (fb.msm(k) == enc).all()                           # more than 64 bases: d377_batch_fixed_msm is the same sum
    finally:
        if m != 4096:
            fb.close()


@pytest.fixture(scope="module")
def seg101(ctx, oracle, lanes):
    """m = 101 at 12 bits at the first n from L / 64 on whose cut has segments of b >= 2 bases and a shorter last one; the
    degenerate bases and scalars at segment-first positions; the library's sums and the byte-table fold, made once."""
    m = 101
    rng = np.random.default_rng(101)
    probe = ctx.fixed_bases_long(_random_bases(oracle, rng, m), comb_bits=8)
    found = None
    for n in range(lanes // 64, lanes // 64 + 4096):
        g, b = probe.long_plan(n)
        if b >= 2 and m % b != 0:
            found = (n, g, b)
            break
    probe.close()
    assert found is not None
    n, g, b = found
    bases = make_bases(oracle, rng, m, b)
    k = make_scalars(rng, n, m, g, b)
    with ctx.fixed_bases_long(bases, comb_bits=12) as fb:
        assert fb.long_plan(n) == (g, b)
        enc, el = fb.msm_long(k, elements=True)
    want_enc, want_el = Fold(oracle, bases).dense(k)
    return dict(n=n, g=g, b=b, m=m, bases=bases, k=k, enc=enc, el=el, want_enc=want_enc, want_el=want_el)


def test_multi_base_segments_with_a_shorter_last_one(oracle, lanes, seg101):
    c = seg101
    assert (c["g"], c["b"]) == plan(c["m"], c["n"], lanes)
    assert c["b"] >= 2 and c["m"] % c["b"] != 0 and (c["g"] - 1) * c["b"] < c["m"] < c["g"] * c["b"]
    assert (c["enc"] == c["want_enc"]).all(), np.nonzero((c["enc"] != c["want_enc"]).any(1))[0][:8]
    assert oracle.eq_xyzt(c["el"], c["want_el"]).all()
    assert (oracle.compress(c["el"][::7]) == c["enc"][::7]).all()


def test_degenerate_bases_and_scalars_at_segment_firsts(oracle, seg101):
    c = seg101
    n, m, g, b = c["n"], c["m"], c["g"], c["b"]
    firsts = c["bases"][0:8 * b:b]
    assert oracle.is_identity(firsts).sum() >= 1 and (firsts == oracle.generator_xyzt()).all(1).any() and len(KINDS) == 4
    kk = c["k"].reshape(n, m, 32)
    sums = sorted({t % (n - 1) for t in range(len(SPECIAL))})
    for t, v in enumerate(SPECIAL):                               # where make_scalars put them: the first base of a segment
        assert (kk[t % (n - 1), ((t // (n - 1)) % g) * b] == scalar_bytes(v)).all()
    want_enc, want_el = oracle_fold(oracle, c["bases"], np.ascontiguousarray(kk[sums].reshape(-1, 32)), len(sums), m)
    assert (c["enc"][sums] == want_enc).all()
    assert oracle.eq_xyzt(c["el"][sums], want_el).all()
    assert not kk[n - 1].any() and not c["enc"][n - 1].any() and oracle.is_identity(c["el"][n - 1:]).all()


def test_one_segment_per_sum_is_the_lane_kernel(ctx, oracle, lanes):
    m = 65
    rng = np.random.default_rng(65)
    bases = _random_bases(oracle, rng, m)
    with ctx.fixed_bases_long(bases, comb_bits=8) as fb, ctx.fixed_bases(bases[:64], comb_bits=8) as head, \
            ctx.fixed_bases(bases[64:], comb_bits=8) as tail:
        n = lanes
        assert fb.long_plan(n) == (1, m) and fb.long_plan(n - 1)[0] == 2
        k = rng.integers(0, 256, (n, m, 32), dtype=np.uint8)
        enc, el = fb.msm_long(k.reshape(n * m, 32), elements=True)
        _, a = head.msm(np.ascontiguousarray(k[:, :64]).reshape(n * 64, 32), elements=True)
        _, t = tail.msm(np.ascontiguousarray(k[:, 64]), elements=True)
    want = ctx.compress(ctx.add(a, t))
    assert (enc == want).all(), np.nonzero((enc != want).any(1))[0][:8]
    assert (ctx.compress(el) == enc).all()
    idx = np.arange(0, n, n // 256)[:256]
    o_enc, o_el = _oracle_sums(oracle, bases, np.ascontiguousarray(k[idx]).reshape(-1, 32), len(idx), m)
    assert (enc[idx] == o_enc).all()
    assert oracle.eq_xyzt(el[idx], o_el).all()


def test_indexed_sums_over_4096_bases(ctx, oracle, big):
    bases, fb = big
    n, t, m = 4097, 2, 4096
    rng = np.random.default_rng(2)
    idx = rng.integers(0, m, (n, t)).astype(np.int32)
    idx[0] = (0, 63)
    idx[1] = (64, 4095)
    idx[2] = (4095, -1)
    idx[3] = (-1, -1)
    idx[4] = (4095, 4095)                                         # a repeated index: the terms add
    idx[n - 1] = (-1, 64)
    k = rng.integers(0, 256, (n * t, 32), dtype=np.uint8)
    enc, el = fb.msm_indexed(idx, k, elements=True)
    flat = idx.reshape(-1)
    pts = np.where((flat >= 0)[:, None], bases[np.maximum(flat, 0)], oracle.identity_xyzt()[None, :])
    kk = np.where((flat >= 0)[:, None], k, 0).astype(np.uint8)
    terms = oracle.scalar_mul_xyzt(np.ascontiguousarray(pts, dtype=np.uint64), np.ascontiguousarray(kk)).reshape(n, t, 16)
    want = oracle.add_xyzt(np.ascontiguousarray(terms[:, 0]), np.ascontiguousarray(terms[:, 1]))
    assert (enc == oracle.compress(want)).all()
    assert oracle.eq_xyzt(el, want).all()
    assert not enc[3].any()

    # an index of 4096 names no base: D377_ERR_ARG, and no output is written
    from decaf377_amd import _native
    lib = _native.load()
    bad = idx.copy()
    bad[n // 2, 1] = m
    out_enc = np.full((n, 32), 0xA5, np.uint8)
    out_el = np.full((n, 16), 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = lib.d377_batch_fixed_msm_indexed(ctx._h, fb._h, _p(bad), _p(k), t, n, _p(out_enc), _p(out_el))
    assert rc == -2 and "base_index" in lib.d377_last_error().decode() and "4095" in lib.d377_last_error().decode()
    assert (out_enc == 0xA5).all() and (out_el == 0xA5A5A5A5A5A5A5A5).all()


@pytest.mark.parametrize("m", [3, 64])
def test_a_short_handle_through_the_long_call(ctx, oracle, lanes, m):
    rng = np.random.default_rng(m)
    bases = _random_bases(oracle, rng, m)
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        for n in (5, 4097):
            k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
            assert fb.long_plan(n) == plan(m, n, lanes) and fb.long_plan(n)[0] > 1
            enc, el = fb.msm_long(k, elements=True)
            want, want_el = fb.msm(k, elements=True)
            assert (enc == want).all(), (m, n)
            assert oracle.eq_xyzt(el[::41], want_el[::41]).all()


def test_device_listed_twice_slices_the_sums(oracle, lanes):
    import decaf377_amd as d
    rng = np.random.default_rng(22)
    m, n = 100, 5
    bases = _random_bases(oracle, rng, m)
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    out = []
    for ids in ([0], [0, 0]):
        c = d.Context(ids, comb_lazy=True)
        with c.fixed_bases_long(bases, comb_bits=8) as fb:
            if len(ids) == 2:                                     # 3 sums and 2 sums: each device cuts its own slice
                assert fb.long_plan(n, 0) == plan(m, 3, lanes) and fb.long_plan(n, 1) == plan(m, 2, lanes)
                assert fb.long_plan(1, 1) == (0, 0)
            out.append(fb.msm_long(k, elements=True))
        c.close()
    assert (out[0][0] == out[1][0]).all()
    assert oracle.eq_xyzt(out[0][1], out[1][1]).all()
    assert (out[0][0] == _oracle_sums(oracle, bases, k, n, m)[0]).all()


def test_torch_tensors_are_staged_through_host_memory(ctx, oracle):
    import torch
    rng = np.random.default_rng(6)
    m, n = 70, 4
    bases = _random_bases(oracle, rng, m)
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    with ctx.fixed_bases_long(torch.from_numpy(bases.view(np.int64)).to("cuda:0"), comb_bits=8) as fb:
        want, want_el = fb.msm_long(k, elements=True)
        t_enc, t_el = fb.msm_long(torch.from_numpy(k).to("cuda:0"), elements=True)
    assert t_enc.device.type == "cuda" and t_el.device.type == "cuda" and t_el.dtype == torch.int64
    assert (t_enc.cpu().numpy() == want).all()
    assert (t_el.cpu().numpy().view(np.uint64) == want_el).all()
    assert (want == _oracle_sums(oracle, bases, k, n, m)[0]).all()


def test_cpp_mirror_fixed_bases_long():
    build_and_run_cpp("fixed_bases_long", "CPP_FIXED_BASES_LONG_OK")


def test_context_health_afterwards(ctx):
    """Last in the module: no lane set is left claimed and no workgroup gave up (the segment kernel claims none; the
    compressor pass does)."""
    claimed, _, gave_up = ctx.health()
    assert claimed == 0 and gave_up == 0
