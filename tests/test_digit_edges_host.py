"""The digit edges without a GPU: the builder of tests/_digit_cases.py, the device's own recodings compiled for the host
(fb_digit<BITS> at the six comb widths, fr_recode_signed16: tests/host_sim/sim.cpp) against its big-integer restatement
-- digit for digit, not merely as a sum -- and the comb cases through the host simulation's 8- and 12-bit comb walks
(the context's walk, the dense and the indexed multi-comb walks) against the oracle.  msm_digit has the same check in
tests/test_host_sim.py (test_msm_windows_digits_and_span_plan)."""
import ctypes

import numpy as np
import pytest

import _digit_cases as dc
from test_fixed_bases_indexed_host import fxi  # noqa: F401  (fixture: the host build of the multi-comb walks)
from test_fixed_msm_long_host import built, sims  # noqa: F401  (fixtures: the host builds of the segment walk)
from test_host_sim import sim  # noqa: F401  (fixture: the host build of the per-lane device functions)

LAYOUTS = ([("comb%d" % B, dc.comb(B), B) for B in dc.COMB_WIDTHS] + [("msm%d" % c, dc.msm(c), None) for c in dc.MSM_WIDTHS]
           + [("w4", dc.w4(), None)])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name,layout,bits", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_builder_cases_recode_to_their_digits_and_cover_every_boundary(name, layout, bits):
    """Every case is a scalar below r whose recoding is the digit vector it was built from (from_digits asserts both), and
    the cases of a layout together reach lo = -2^(w-1) and hi = 2^(w-1) - 1 of every window below the top and the top
    window's largest digit.  The layouts tile the scalar: consecutive windows, 252 bits or more, the top bit of r - 1 in
    the top window; the all-ones case really is a window of ones that a carry turns into digit 0."""
    assert layout[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(layout, layout[1:]))
    assert layout[-1][0] + layout[-1][1] >= 252
    top = dc.top_index(layout)
    assert layout[top][0] <= 250 < layout[top][0] + layout[top][1]
    cs = dc.cases(layout, bits)
    assert len(set(h for _, _, h in cs)) == len(cs)
    for cname, d, h in cs:
        assert dc.from_digits(layout, d) == h and dc.recode(layout, h) == d, cname
        assert all(v == 0 for v in d[top + 1:]), cname
        if cname.endswith("ones+carry"):
            i = int(cname[1:cname.index(":")])
            assert dc.raw_windows(layout, h)[i] == (1 << layout[i][1]) - 1 and d[i] == 0, cname
        if cname.endswith("lo<carry"):
            i = int(cname[1:cname.index(":")])
            assert dc.raw_windows(layout, h)[i] == (1 << (layout[i][1] - 1)) - 1, cname      # dd == 2^(w-1) by the carry alone
    dc.assert_covers(layout, [h for _, _, h in cs])
    if bits is not None:                                           # the comb builder's runs: the lone last entry and the run edges
        met = dc.pairs_met(layout, [h for _, _, h in cs])
        for i in range(top):
            for e in dc.run_entries(bits):
                assert (i, -e) in met and ((i, e) in met or e == 1 << (bits - 1)), (i, e)
        assert (1 << (bits - 1)) % dc.FB_RUN == 0                  # entry 2^(B-1) is alone in the builder's last run


def test_restated_layouts_are_the_shipped_shapes():
    """comb(B) is FbShape<B> (windows = ceil(252 / B), all B wide); msm(c) tiles the 252 bits with the wide windows first."""
    assert [len(dc.comb(B)) for B in dc.COMB_WIDTHS] == [32, 21, 16, 14, 12, 11]
    for c in dc.MSM_WIDTHS:
        lay = dc.msm(c)
        widths = [w for _, w in lay]
        assert len(lay) == -(-252 // c) and sum(widths) == 252 and set(widths) <= {c, c - 1}
        assert widths == sorted(widths, reverse=True)
    assert dc.msm(16) == [(16 * i, 16) for i in range(12)] + [(192 + 15 * i, 15) for i in range(4)]
    assert dc.top_max(dc.w4()) == 5 and dc.top_index(dc.w4()) == 62     # r >> 248 = 4, and nibble 61 of r - 1 carries


@pytest.mark.parametrize("name,layout,bits", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_vector_recoding_is_the_big_integer_one(name, layout, bits):
    """recode_rows, which the GPU sweeps use on a million scalars at once, gives recode's digits on the cases and on
    random scalars below r."""
    rng = np.random.default_rng(1600 + len(layout))
    hs = [h for _, _, h in dc.cases(layout, bits)]
    hs += [int.from_bytes(bytes(row), "little") % dc.R for row in rng.integers(0, 256, (300, 32), dtype=np.uint8)]
    got = dc.recode_rows(layout, dc.scalars(hs, False))
    assert [[int(x) for x in row] for row in got] == [dc.recode(layout, h) for h in hs]


def _targets(layout, bits=None):
    """The case scalars of a layout as (h, halved, plus_r) plans with their wanted digits: every case in both forms, and
    the first of every three with r added as well."""
    cs = dc.cases(layout, bits)
    plan = []
    for halved in (0, 1):
        plan += [(h, halved, False, d) for _, d, h in cs]
        plan += [(h, halved, True, d) for _, d, h in cs[::3]]
    return plan


@pytest.mark.parametrize("bits", dc.COMB_WIDTHS)
def test_fb_digit_gives_the_wanted_digits(sim, bits):
    """fb_digit<BITS>, the code every comb walk runs: for the targeted scalars -- as passed, 2 h mod r for a halving walk
    and h for the Element form, some with r added -- and for random ones, the digit vector is the restatement's."""
    layout = dc.comb(bits)
    rng = np.random.default_rng(1700 + bits)
    for halve in (0, 1):
        plan = [p for p in _targets(layout, bits) if p[1] == halve]
        k = np.concatenate([np.stack([dc.scalar(h, bool(hv), pr) for h, hv, pr, _ in plan]), rng.integers(0, 256, (200, 32), dtype=np.uint8)])
        want = [d for _, _, _, d in plan]
        for row in k[len(plan):]:
            kv = int.from_bytes(bytes(row), "little") % dc.R
            want.append(dc.recode(layout, (kv * pow(2, -1, dc.R)) % dc.R if halve else kv))
        dig = np.zeros((len(k), 64), np.int32)
        W = sim.sim_fb_digits(_p(np.ascontiguousarray(k)), ctypes.c_size_t(len(k)), bits, halve, _p(dig))
        assert W == len(layout)
        got = [[int(x) for x in row[:W]] for row in dig]
        bad = [i for i in range(len(k)) if got[i] != want[i]]
        assert not bad, (bits, halve, bad[:5], got[bad[0]], want[bad[0]])
        assert not dig[:, 63].any()                                # the top window never carries out


def test_w4_recoding_gives_the_wanted_digits(sim):
    """fr_recode_signed16 read back through fr_digit: nibble 8 is digit -8, the carry window stays 0 below r."""
    layout = dc.w4()
    rng = np.random.default_rng(1704)
    for halve in (0, 1):
        plan = [p for p in _targets(layout) if p[1] == halve]
        k = np.concatenate([np.stack([dc.scalar(h, bool(hv), pr) for h, hv, pr, _ in plan]), rng.integers(0, 256, (200, 32), dtype=np.uint8)])
        want = [d for _, _, _, d in plan]
        for row in k[len(plan):]:
            kv = int.from_bytes(bytes(row), "little") % dc.R
            want.append(dc.recode(layout, (kv * pow(2, -1, dc.R)) % dc.R if halve else kv))
        dig = np.zeros((len(k), 64), np.int32)
        sim.sim_w4_digits(_p(np.ascontiguousarray(k)), ctypes.c_size_t(len(k)), halve, _p(dig))
        got = [[int(x) for x in row] for row in dig]
        bad = [i for i in range(len(k)) if got[i] != want[i]]
        assert not bad, (halve, bad[:5], got[bad[0]], want[bad[0]])
    dc.assert_covers(layout, [h for h, _, _, _ in _targets(layout)])


def test_comb_cases_through_the_host_context_walk(sim, oracle):
    """ge_scalar_mul_base_w8 on the host simulation's 12-bit generator comb (halved: the Encoding form), every comb(12) case
    and some with r added, against the oracle's fixed-base multiplication."""
    cs = dc.comb_cases(12)
    hs = [h for _, _, h in cs]
    dc.assert_covers(dc.comb(12), hs)
    k = np.concatenate([dc.scalars(hs, True), dc.scalars(hs[::3], True, plus_r=True)])
    out = np.zeros((len(k), 32), np.uint8)
    sim.sim_scalar_mul_base(_p(k), ctypes.c_size_t(len(k)), _p(out))
    want = oracle.scalar_mul_base(k)
    bad = np.nonzero((out != want).any(1))[0]
    assert not bad.size, [cs[i % len(cs)][0] for i in bad[:8]]


@pytest.mark.parametrize("bits", [8, 12])
def test_comb_cases_through_the_host_multi_comb_walks(fxi, oracle, bits):
    """ge_fixed_msm_w8 and ge_fixed_msm_indexed_w8 over host-built combs of two bases (a random point and GENERATOR): each
    base targeted in turn while the other takes a random scalar, so the carry is reset where one base's digits end and
    the next one's begin with a boundary digit; indexed sums of one and of two terms, the same comb twice among them."""
    rng = np.random.default_rng(1800 + bits)
    bases = np.ascontiguousarray(np.stack([oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0], oracle.generator_xyzt()]),
                                 dtype=np.uint64)
    cs = dc.comb_cases(bits)
    hs = [h for _, _, h in cs]
    dc.assert_covers(dc.comb(bits), hs)
    tk = dc.scalars(hs, True)
    n = len(hs)
    assert fxi.fx_build(_p(bases), 2, bits) == 0
    prod = [oracle.scalar_mul_xyzt(np.tile(bases[j], (n, 1)), tk) for j in range(2)]       # target x base j
    # dense, m = 2: (target, random) and (random, target)
    for pos in (0, 1):
        k = rng.integers(0, 256, (n, 2, 32), dtype=np.uint8)
        k[:, pos] = tk
        other = oracle.scalar_mul_xyzt(np.tile(bases[1 - pos], (n, 1)), np.ascontiguousarray(k[:, 1 - pos]))
        want = oracle.compress(oracle.add_xyzt(prod[pos], other))
        enc = np.zeros((n, 32), np.uint8)
        assert fxi.fx_msm(_p(np.ascontiguousarray(k.reshape(2 * n, 32))), n, _p(enc), None) == 0
        bad = np.nonzero((enc != want).any(1))[0]
        assert not bad.size, (pos, [cs[i][0] for i in bad[:8]])
    # indexed, t = 1: each base; t = 2: (j, j) with the target twice, and (j, 1 - j) with the target last
    for j in (0, 1):
        idx = np.full((n, 1), j, np.int32)
        enc = np.zeros((n, 32), np.uint8)
        assert fxi.fx_msm_indexed(_p(idx), _p(tk), 1, n, _p(enc), None) == 0
        assert (enc == oracle.compress(prod[j])).all(), j
        idx = np.full((n, 2), j, np.int32)
        enc = np.zeros((n, 32), np.uint8)
        assert fxi.fx_msm_indexed(_p(idx), _p(np.ascontiguousarray(np.repeat(tk, 2, axis=0))), 2, n, _p(enc), None) == 0
        assert (enc == oracle.compress(oracle.double_xyzt(prod[j]))).all(), j
        k = rng.integers(0, 256, (n, 2, 32), dtype=np.uint8)
        k[:, 1] = tk
        idx = np.tile(np.array([1 - j, j], np.int32), (n, 1))
        other = oracle.scalar_mul_xyzt(np.tile(bases[1 - j], (n, 1)), np.ascontiguousarray(k[:, 0]))
        enc = np.zeros((n, 32), np.uint8)
        assert fxi.fx_msm_indexed(_p(np.ascontiguousarray(idx)), _p(np.ascontiguousarray(k.reshape(2 * n, 32))), 2, n, _p(enc), None) == 0
        assert (enc == oracle.compress(oracle.add_xyzt(prod[j], other))).all(), j


@pytest.mark.parametrize("bits", [8, 12])
def test_comb_cases_through_the_host_segment_walk(sims, oracle, bits):
    """d377_batch_fixed_long_msm's walk on the host, two bases cut into two segments of one base each (a device of 2 n lanes
    for n sums): every segment starts a walk of its own, so the targeted base's first window is the record the sum starts
    from whichever base it is."""
    rng = np.random.default_rng(1900 + bits)
    bases = np.ascontiguousarray(np.stack([oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0], oracle.generator_xyzt()]),
                                 dtype=np.uint64)
    cs = dc.comb_cases(bits)
    hs = [h for _, _, h in cs]
    dc.assert_covers(dc.comb(bits), hs)
    tk = dc.scalars(hs, True)
    n = len(hs)
    sim = sims[bits]
    assert sim.fml_build(_p(bases), 2, bits) == 0
    for pos in (0, 1):
        k = rng.integers(0, 256, (n, 2, 32), dtype=np.uint8)
        k[:, pos] = tk
        k = np.ascontiguousarray(k.reshape(2 * n, 32))
        terms = oracle.scalar_mul_xyzt(np.tile(bases, (n, 1)), k)
        want = oracle.compress(oracle.add_xyzt(np.ascontiguousarray(terms[0::2]), np.ascontiguousarray(terms[1::2])))
        enc = np.zeros((n, 32), np.uint8)
        gb = np.zeros(2, np.uint64)
        assert sim.fml_msm_long(_p(k), n, 2 * n, _p(enc), None, _p(gb)) == 0
        assert (int(gb[0]), int(gb[1])) == (2, 1)
        bad = np.nonzero((enc != want).any(1))[0]
        assert not bad.size, (pos, [cs[i][0] for i in bad[:8]])
