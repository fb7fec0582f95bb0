"""The last comb entry and the last bucket of every window, on the MI355X.

Every scalar-consuming kernel recodes its scalar into signed digits, and a window of B bits takes the boundary digit
-2^(B-1) for one value in 2^B: random scalars do not reach entry 2^(B-1) of a 23-bit comb window, the lone last bucket of a
16-bit MSM window or nibble 8 of a Straus chain often enough to test them.  The scalars here are built from their digits
(tests/_digit_cases.py); every test first asserts, through the big-integer recoding, which (window, digit) pairs its plan
reaches -- the share of claimed pairs left out is zero -- and then compares bit for bit with the oracle, the sweeps of
whole comb tables with the variable-base kernel (independent code, itself checked against the oracle) and a stride of
them with the oracle."""
import numpy as np
import pytest

import _digit_cases as dc

pytestmark = pytest.mark.gpu

R = dc.R
THREADS = 8
ALL_ON = 1 << 24                                                   # a batch limit no test batch reaches


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx():
    """The context of the tests that use no generator comb (it is lazy and never built)."""
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    assert not c.comb_info()[1]
    c.close()


@pytest.fixture(scope="module", params=[18, 21, 23])
def comb_ctx(request):
    """A context per generator-comb width, one after another: the previous one is closed before the next is built."""
    import decaf377_amd as d
    c = d.Context([0], comb_bits=request.param)
    assert c.comb_info()[:2] == (request.param, True)
    yield c
    c.close()


def _healthy(c):
    claimed, _, gave_up = c.health()
    assert claimed == 0 and gave_up == 0, (claimed, gave_up)


def _rows(values):
    """[n, 32] u8 little-endian rows of the integers."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def _mul(oracle, P, k):
    """The oracle's k[i] * P[i] as Element records, on several threads (through its Encoding form, which has a threaded driver)."""
    out, st, _ = oracle.run_threads("scalar_mul_var", oracle.compress(P), k, THREADS)
    assert not st.any()
    return oracle.decompress(out)[0]


def _mul_base(oracle, k):
    return oracle.run_threads("scalar_mul_base", k, None, THREADS)[0]


def _names(cs, bad, n=8):
    """The cases' names for the failing rows of a plan that holds every case and then every third again with r added."""
    return [cs[i][0] if i < len(cs) else cs[3 * (i - len(cs))][0] + ",+r" for i in bad[:n]]


# ---- the generator comb ---------------------------------------------------------------------------------------------------
ENC_ROUTES = ([("wave", dict(small_max=ALL_ON, tiny_max=ALL_ON)), ("quad", dict(small_max=ALL_ON, tiny_max=0))]
              + [("lanes,%s,k=%d" % ("wide" if w else "narrow", k), dict(small_max=0, fb_wide=w, fb_k=k)) for w in (0, 1) for k in (1, 8, 16)])
# the Element form has one lane kernel (no shared inversion: no launch shapes)
EL_ROUTES = [("wave", dict(small_max=ALL_ON, tiny_max=ALL_ON)), ("quad", dict(small_max=ALL_ON, tiny_max=0)), ("lanes", dict(small_max=0))]
_COMB_WANT = {}


def _comb_plan(bits, oracle):
    """The comb cases of a width, with r added to every third: (cases, h per scalar, 2 h mod r as bytes, h as bytes, the
    oracle's encodings of the one and of the other).  Computed once per width."""
    if bits not in _COMB_WANT:
        cs = dc.comb_cases(bits)
        hs = [h for _, _, h in cs]
        layout = dc.comb(bits)
        dc.assert_covers(layout, hs)
        met = dc.pairs_met(layout, hs)
        for i in range(dc.top_index(layout)):                      # the builder's run edges and its lone last entry, both signs
            for e in dc.run_entries(bits):
                assert (i, -e) in met and ((i, e) in met or e == 1 << (bits - 1)), (i, e)
        allh = hs + hs[::3]
        halved = np.concatenate([dc.scalars(hs, True), dc.scalars(hs[::3], True, plus_r=True)])
        plain = np.concatenate([dc.scalars(hs, False), dc.scalars(hs[::3], False, plus_r=True)])
        _COMB_WANT[bits] = (cs, allh, halved, plain, _mul_base(oracle, plain), _mul_base(oracle, halved))
    return _COMB_WANT[bits]


@pytest.mark.parametrize("form", ["encoding", "element"])
def test_generator_comb_cases_every_route(comb_ctx, oracle, form):
    """All comb cases of the context's width through scalar_mul_base (which walks k / 2 mod r: the scalars are 2 h mod r)
    and scalar_mul_base_element (which walks k: the scalars are h), on every route -- a wave per scalar, a quad per
    scalar, and the lane kernel launched narrow and wide with 1, 8 and 16 scalars per shared inversion, forced through
    the tuning keys -- against the oracle's fixed-base multiplication."""
    c = comb_ctx
    bits = c.comb_info()[0]
    cs, allh, halved, plain, want_plain, want_halved = _comb_plan(bits, oracle)
    layout = dc.comb(bits)
    if form == "encoding":                                         # what the kernel walks is h: the claimed digits
        assert all((int.from_bytes(bytes(k), "little") % R) * pow(2, -1, R) % R == h for k, h in zip(halved[::37], allh[::37]))
        for name, tune in ENC_ROUTES:
            with c.tuning(**tune):
                got = c.scalar_mul_base(halved)
            bad = np.nonzero((got != want_halved).any(1))[0]
            assert not bad.size, (bits, name, _names(cs, bad))
    else:
        assert all(int.from_bytes(bytes(k), "little") % R == h for k, h in zip(plain[::37], allh[::37]))
        for name, tune in EL_ROUTES:
            with c.tuning(**tune):
                got = c.compress(c.scalar_mul_base_element(plain))
            bad = np.nonzero((got != want_plain).any(1))[0]
            assert not bad.size, (bits, name, _names(cs, bad))
    assert c.get_tuning("small_max") is None and c.get_tuning("fb_k") is None
    assert dc.claimed_pairs(layout) <= dc.pairs_met(layout, allh)
    _healthy(c)


SWEEP_PARTS = 4


def _sweep_entries(bits, window, rng):
    """The entries of one window that the sweep visits, as signed digits: at 18 bits every entry (entry 2^17 as the digit
    -2^17); at 21 and 23 bits the first 64, the last 65 and 2^14 random ones, with both signs."""
    layout = dc.comb(bits)
    top = dc.top_index(layout)
    half = 1 << (bits - 1)
    if window == top:                                              # a scalar below r reaches 0 .. (r - 1) >> first bit, never negative
        last = (R - 1) >> layout[top][0]
        if bits == 18:
            return np.arange(0, last + 1, dtype=np.int64)
        pos = np.unique(np.concatenate([np.arange(64), np.arange(last - 64, last + 1), rng.integers(0, last + 1, 1 << 14)]))
        return pos.astype(np.int64)
    if bits == 18:
        return np.concatenate([np.arange(0, half, dtype=np.int64), [-half]])
    pos = np.unique(np.concatenate([np.arange(64), np.arange(half - 65, half), rng.integers(0, half, 1 << 14)])).astype(np.int64)
    neg = np.unique(np.concatenate([np.arange(1, 65), np.arange(half - 64, half + 1), rng.integers(1, half + 1, 1 << 14)])).astype(np.int64)
    return np.concatenate([pos, -neg])


def _generator_sweep_plan(bits, part):
    """(h per record, their bytes, [(window, records, their digits)]) of one part of the sweep, with the coverage asserted."""
    layout = dc.comb(bits)
    top = dc.top_index(layout)
    rng = np.random.default_rng(1000 * bits + part)
    hs, plan = [], []
    for i in range(part, top + 1, SWEEP_PARTS):
        d = _sweep_entries(bits, i, rng)
        fb = layout[i][0]
        up = (1 << layout[i + 1][0]) if i < top else 0
        hs += [(int(v) << fb) + (up if v < 0 else 0) for v in d]
        plan.append((i, len(d), d))
    hb = _rows(hs)
    digits = dc.recode_rows(layout, hb)
    at = 0
    for i, cnt, d in plan:                                        # each record walks the claimed entry, and only it (and the 1 above)
        assert (digits[at:at + cnt, i] == d).all(), i
        others = np.delete(digits[at:at + cnt], [i] + ([i + 1] if i < top else []), axis=1)
        assert not others.any(), i
        if bits == 18 and i < top:
            assert len(d) == (1 << 17) + 1 and set(d.tolist()) == set(range(0, 1 << 17)) | {-(1 << 17)}
        if i < top:
            assert -(1 << (bits - 1)) in d and (1 << (bits - 1)) - 1 in d
        at += cnt
    return hs, hb, plan


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_generator_comb_table_sweep(comb_ctx, oracle, torch_mod, part):
    """The table itself, entry by entry (Element form: the scalar is walked as passed): digit d in window i and nothing
    else, a negative digit with the 1 in the window above that makes the scalar positive.  At 18 bits every entry of every
    window (14 x 131 073 records; the top window as far as a scalar below r reaches), at 21 and 23 bits the first 64, the
    last 65 and 2^14 seeded random entries per window with both signs.  The windows are dealt to SWEEP_PARTS tests.
    Compared in full with scalar_mul_var_element of GENERATOR on the same scalars (eq on the records, and the
    encodings), and every 4096th record, the last entries among them, with the oracle."""
    torch = torch_mod
    c = comb_ctx
    bits = c.comb_info()[0]
    hs, hb, plan = _generator_sweep_plan(bits, part)
    dev = torch.device("cuda:0")
    k = torch.from_numpy(hb).to(dev)
    gen = torch.from_numpy(c.generator().view(np.int64)).to(dev).repeat(len(hs), 1)
    fixed = c.scalar_mul_base_element(k)
    var = c.scalar_mul_var_element(gen, k)
    assert bool(c.eq(fixed, var).all())
    fe, ve = c.compress(fixed), c.compress(var)
    bad = torch.nonzero((fe != ve).any(1)).flatten()[:8].cpu().numpy()
    assert not bad.size, (bits, [(int(b), hs[int(b)].bit_length()) for b in bad])
    ends = np.cumsum([cnt for _, cnt, _ in plan]) - 1             # the last record of a window: entry 2^(B-1) below the top
    idx = np.unique(np.concatenate([np.arange(0, len(hs), 4096), ends]))
    assert (fe[torch.from_numpy(idx).to(dev)].cpu().numpy() == oracle.scalar_mul_base(hb[idx])).all()
    _healthy(c)


# ---- caller-chosen combs --------------------------------------------------------------------------------------------------
CALLER_WIDTHS = [8, 12, 16, 18]


@pytest.fixture(scope="module")
def two_bases(oracle):
    """A random point and GENERATOR."""
    rng = np.random.default_rng(4242)
    return np.ascontiguousarray(np.stack([oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0], oracle.generator_xyzt()]),
                                dtype=np.uint64)


@pytest.mark.parametrize("bits", CALLER_WIDTHS)
def test_caller_comb_cases_dense_indexed_and_long(ctx, oracle, two_bases, bits):
    """The comb cases of the width on combs of two caller-chosen bases (every walk here halves: the scalars are 2 h mod r):
    the dense call with each base targeted in turn and a random scalar on the other, so the carry is reset where one
    base's digits end and the next one's begin with a boundary digit; indexed sums of one term and of two -- the same comb
    twice, and the target after another comb; and msm_long where its plan cuts the sum into more than one segment."""
    rng = np.random.default_rng(4300 + bits)
    layout = dc.comb(bits)
    cs = dc.comb_cases(bits)
    hs = [h for _, _, h in cs]
    dc.assert_covers(layout, hs)
    met = dc.pairs_met(layout, hs)
    assert all((i, -(1 << (bits - 1))) in met for i in range(dc.top_index(layout)))
    tk = np.concatenate([dc.scalars(hs, True), dc.scalars(hs[::3], True, plus_r=True)])
    n = len(tk)
    prod = [_mul(oracle, np.tile(two_bases[j], (n, 1)), tk) for j in range(2)]
    rk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rprod = [_mul(oracle, np.tile(two_bases[j], (n, 1)), rk) for j in range(2)]
    with ctx.fixed_bases(two_bases, comb_bits=bits) as fb:
        assert fb.info()[:2] == (2, bits)
        assert fb.long_plan(n)[0] > 1
        for pos in (0, 1):
            k = np.empty((n, 2, 32), np.uint8)
            k[:, pos], k[:, 1 - pos] = tk, rk
            k = np.ascontiguousarray(k.reshape(2 * n, 32))
            want = oracle.compress(oracle.add_xyzt(prod[pos], rprod[1 - pos]))
            for name, call in (("dense", fb.msm), ("long", fb.msm_long)):
                bad = np.nonzero((call(k) != want).any(1))[0]
                assert not bad.size, (bits, name, pos, _names(cs, bad))
        for j in (0, 1):
            got = fb.msm_indexed(np.full((n, 1), j, np.int32), tk)
            bad = np.nonzero((got != oracle.compress(prod[j])).any(1))[0]
            assert not bad.size, (bits, "indexed t=1", j, _names(cs, bad))
            got = fb.msm_indexed(np.full((n, 2), j, np.int32), np.ascontiguousarray(np.repeat(tk, 2, axis=0)))
            bad = np.nonzero((got != oracle.compress(oracle.double_xyzt(prod[j]))).any(1))[0]
            assert not bad.size, (bits, "indexed twice", j, _names(cs, bad))
            k = np.empty((n, 2, 32), np.uint8)
            k[:, 0], k[:, 1] = rk, tk
            got = fb.msm_indexed(np.tile(np.array([1 - j, j], np.int32), (n, 1)), k)
            bad = np.nonzero((got != oracle.compress(oracle.add_xyzt(prod[j], rprod[1 - j]))).any(1))[0]
            assert not bad.size, (bits, "indexed after another comb", j, _names(cs, bad))
    _healthy(ctx)


def _caller_sweep_plan(bits):
    """(h per record, the index of each window's last record) of a caller comb's full sweep, with the coverage asserted."""
    layout = dc.comb(bits)
    top = dc.top_index(layout)
    half = 1 << (bits - 1)
    hs, ends = [], []
    for i, (fb_, _) in enumerate(layout[:top + 1]):
        if i < top:
            hs += [v << fb_ for v in range(half)] + [(1 << layout[i + 1][0]) - (half << fb_)]
        else:
            hs += [v << fb_ for v in range(((R - 1) >> fb_) + 1)]
        ends.append(len(hs) - 1)
    hb = _rows(hs)
    digits = dc.recode_rows(layout, hb)
    at = 0
    for i in range(top):                                           # entries 0 .. 2^(B-1) - 1 as themselves, 2^(B-1) as the digit -2^(B-1)
        assert (digits[at:at + half, i] == np.arange(half)).all() and digits[at + half, i] == -half and digits[at + half, i + 1] == 1
        at += half + 1
    assert (digits[at:, top] == np.arange(len(hs) - at)).all()
    assert (np.count_nonzero(digits, axis=1) <= 2).all()
    return hs, ends


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_caller_comb_table_sweep(ctx, oracle, torch_mod, two_bases, bits, base):
    """Every entry of every window of a caller-chosen comb (the top window as far as a scalar below r reaches) through
    msm_indexed with one term, which walks k / 2 mod r (the scalars are 2 h mod r): the records and the encodings against
    scalar_mul_var_element of the base on the same scalars, every 4096th and each window's last against the oracle."""
    torch = torch_mod
    hs, ends = _caller_sweep_plan(bits)
    kb = _rows([(2 * h) % R for h in hs])
    n = len(hs)
    with ctx.fixed_bases(two_bases, comb_bits=bits) as fb:
        enc, el = fb.msm_indexed(np.full((n, 1), base, np.int32), kb, elements=True)
    dev = torch.device("cuda:0")
    var = ctx.scalar_mul_var_element(torch.from_numpy(two_bases[base].view(np.int64)).to(dev).repeat(n, 1), torch.from_numpy(kb).to(dev))
    el_d = torch.from_numpy(el.view(np.int64)).to(dev)
    assert bool(ctx.eq(el_d, var).all())
    ve = ctx.compress(var).cpu().numpy()
    bad = np.nonzero((enc != ve).any(1))[0]
    assert not bad.size, (bits, base, bad[:8])
    idx = np.unique(np.concatenate([np.arange(0, n, 4096), ends]))
    want = oracle.compress(oracle.scalar_mul_xyzt(np.tile(two_bases[base], (len(idx), 1)), kb[idx]))
    assert (enc[idx] == want).all()
    _healthy(ctx)


# ---- the bucket MSM -------------------------------------------------------------------------------------------------------
MSM_POINTS = 512


@pytest.fixture(scope="module")
def msm_points(oracle):
    rng = np.random.default_rng(5151)
    P = oracle.elligator_map_xyzt(rng.integers(0, 256, (MSM_POINTS, 32), dtype=np.uint8))
    assert len(set(bytes(e) for e in oracle.compress(P))) == MSM_POINTS          # distinct points
    return P, oracle.compress(P)


@pytest.mark.parametrize("c", dc.MSM_WIDTHS)
def test_msm_last_bucket_of_every_window(ctx, oracle, msm_points, c):
    """The bucket method at window width c (forced for 512 points) on four inputs, Elements and Encodings, against the
    oracle's fold: (1) the msm(c) cases on distinct points, filled with random terms; (2) every scalar the value whose
    windows below the top are all -2^(w-1) -- only last buckets hold anything, and the last super-bucket holds the whole
    batch; (3) half on that value and half on the value with every digit 1 (the first bucket); (4) every window at
    2^(w-1) - 1.  The MSM sums with k / 2 mod r: the scalars are 2 h mod r.  For c = 8, 14, 16, 17 and 18 again with the
    unpacked sort and with 1 and 128 entries per span."""
    P, E = msm_points
    layout = dc.msm(c)
    top = dc.top_index(layout)
    assert top == len(layout) - 1
    cs = dc.msm_cases(c)
    hs = [h for _, _, h in cs]
    assert len(hs) <= MSM_POINTS
    dc.assert_covers(layout, hs)
    rng = np.random.default_rng(5200 + c)
    k1 = rng.integers(0, 256, (MSM_POINTS, 32), dtype=np.uint8)
    k1[:len(hs)] = dc.scalars(hs, True)
    k1[:len(hs):5] = dc.scalars(hs[::5], True, plus_r=True)
    named = dict(dc.all_window_cases(layout))
    all_lo, all_hi = dc.from_digits(layout, named["all-lo"]), dc.from_digits(layout, named["all-hi"])
    ones = dc.from_digits(layout, [1] * len(layout))
    assert dc.recode(layout, all_lo)[:top] == [dc.lo(w) for _, w in layout[:top]]
    assert dc.recode(layout, all_hi)[:top] == [dc.hi(w) for _, w in layout[:top]]
    assert dc.lo(layout[0][1]) == -(1 << (c - 1)) and (c < 8 or (1 << (c - 1)) % 128 == 0)   # bucket 2^(c-1): alone in its super-bucket from c = 8
    inputs = [("cases", k1), ("all-lo", np.tile(dc.scalar(all_lo, True), (MSM_POINTS, 1))),
              ("lo|ones", np.concatenate([np.tile(dc.scalar(all_lo, True), (MSM_POINTS // 2, 1)), np.tile(dc.scalar(ones, True), (MSM_POINTS // 2, 1))])),
              ("all-hi", np.tile(dc.scalar(all_hi, True), (MSM_POINTS, 1)))]
    tunings = [dict()]
    if c in (8, 14, 16, 17, 18):
        tunings += [dict(msm_sort_packed=0), dict(msm_seg=1), dict(msm_seg=128)]
    for name, k in inputs:
        want = bytes(oracle.msm(P, k)[0])
        for extra in tunings:
            with ctx.tuning(msm_window=c, msm_small_max=0, **extra):
                enc, xyzt, _ = ctx.msm(P, k)
                assert bytes(enc) == want, (c, name, extra, "elements")
                assert bytes(oracle.compress(np.asarray(xyzt).reshape(1, 16))[0]) == want, (c, name, extra)
                enc, _, st = ctx.msm(E, k)
                assert bytes(enc) == want and not np.asarray(st).any(), (c, name, extra, "encodings")
    assert ctx.get_tuning("msm_window") is None
    _healthy(ctx)


# ---- the Straus chains ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 8, 9, 17])
def test_straus_chain_nibble_eight(ctx, oracle, m):
    """The w4 cases -- digit -8 (stored as nibble 8), 7, all ones plus a carry, in every window, the top digits of a scalar
    below r -- through d377_batch_msm_small (m = 1, 3, 8) and d377_batch_msm_long (m = 9, 17), the targeted scalar first in
    its sum and then last, the other terms random, against the oracle's fold.  The chains sum with k / 2 mod r: the
    scalars are 2 h mod r."""
    layout = dc.w4()
    cs = dc.w4_cases()
    hs = [h for _, _, h in cs]
    dc.assert_covers(layout, hs)
    assert {(i, -8) for i in range(62)} | {(i, 7) for i in range(62)} | {(62, 5)} <= dc.pairs_met(layout, hs)
    rng = np.random.default_rng(6100 + m)
    tk = np.concatenate([dc.scalars(hs, True), dc.scalars(hs[::3], True, plus_r=True)])
    n = len(tk)
    P = oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8))
    k = rng.integers(0, 256, (n, m, 32), dtype=np.uint8)
    k[:, 0] = tk
    k = np.ascontiguousarray(k.reshape(n * m, 32))
    prod = _mul(oracle, P, k)
    acc = np.ascontiguousarray(prod[0::m])
    for j in range(1, m):
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(prod[j::m]))
    want = oracle.compress(acc)
    call = ctx.msm_small if m <= 8 else ctx.msm_long
    order = np.arange(n * m).reshape(n, m)
    for where in ("first", "last"):
        if where == "last":                                        # the same terms, the targeted one at the end of its sum
            order = order[:, ::-1]
        o = np.ascontiguousarray(order.reshape(-1))
        got = call(np.ascontiguousarray(P[o]), np.ascontiguousarray(k[o]), m)
        bad = np.nonzero((got != want).any(1))[0]
        assert not bad.size, (m, where, _names(cs, bad))
        if m == 1:
            break
    _healthy(ctx)
