"""Every Element-taking call of the Python API on every representative of its input, on the MI355X.

An Element record is one of many representatives of its group element (any scaling l (X, Y, Z, T); the 2-torsion twin
(-X, -Y, Z, T)), the library hands such records out itself, and callers feed them straight back in.  tests/_representatives.py
builds, for a set of points, the plain records A (Z = 1) and the same group elements as the kinds affine, proj (Elligator, Z != 1),
scaled (l A), minus (-A: Z = q - 1, every limb near the top), twin (Z = 1), twin_scaled and twin_minus, and the identity class
(0, 1, 1, 0), (0, l, l, 0), (0, -1, 1, 0), (0, -l, l, 0), P + (-P), P + twin(-P).  tests/test_representatives_host.py shows that
the oracle does not tell them apart; so for every case here

  (a) the result is the oracle's on the PLAIN records, byte for byte;
  (b) the same call on the plain records gives the same bytes (a mismatch here alone: the kernel depends on the representative);
  (c) where a call returns Element records: oracle.eq_xyzt against the oracle's records is all ones, ctx.compress of them is
      (a), and the first 16 are valid extended points in integers (limbs below q, Z != 0, T Z = X Y, the curve equation).

Everything is integer arithmetic and every comparison is exact.

THE ARRAYS.  "mixed_planted": record i is kind KINDS[(i + shift) % 7] of point i, so every wave holds every kind, with
identity-class records planted at positions 0, 63, 64 and n - 1 (those that exist), each in another form; at n = 1 also the
lone ordinary record ("mixed").  At n = 257 also "all_identity_but_one" (a whole wave and more of zero denominators, one scaled
twin in the middle) and "one_identity" ((0, -l, l, 0) at position 70 among ordinary records).  n is 1, 63, 64, 65, 257 unless
stated: a lone element, a wave less one, a full wave, a wave plus one lane, a partial last wave after four full ones.

THE CALLS, the routes forced (Context.tuning) and what each array holds:

  compress, compress_to_field   routes default, four_per_wave (tiny_max = 2^20), wide_grid (tiny_max = 0) and chunked
      (decompress_chunked_min = 1 with tiny_max = 0: launch_plan.hpp asks the four-per-wave rule first, so decompress_chunked_min = 1
      alone stays on four per wave at these sizes; that setting is route "chunked_min_alone").  compress_to_field has the plain
      grid on every setting (launch_plan.hpp); it runs under the same settings.  Every n, every layout; once more on device tensors.
  eq   every layout against its plain records (all ones), against the plain records shifted by one and against their
      negation (the oracle's flags on the plain records), against right operands of the next kind; the identity class pairwise.
  is_identity, to_affine, neg, double, add, sub   one route each (the plain grid; to_affine one lane per record at these
      sizes).  Left operand: every layout.  Right operand (add, sub, eq): _representatives.right_operands -- the NEXT kind, of
      the next point, of the same point (P + twin(P); P - twin(P), the point of order 2) or of its negation (P + twin(-P)).
      neg is limb-exact against oracle.neg_xyzt of the same record.  to_affine is the oracle's to_affine of the same record (the
      twin kinds legitimately give (-x, -y)) and limb-equal to to_affine of the plain record for the kinds affine, scaled, minus.
  scalar_mul_var_element   routes lanes (small_max = 0) with chunk_per_lane 1 and 8 (the Element kernel deals uniform chunks, so
      the two settings must agree), quads (small_max = 2^20, tiny_max = 0), waves (tiny_max = 2^20).  Every n, every layout; the
      builder's scalars: 0, 1, 2, r - 1, r, r + 1, 2^256 - 1, then random ones whose halves k / 2 mod r take both parities -- asserted
      per array for the twin kinds.  Identity-class inputs with non-zero scalars give the all-zero Encoding.
  msm, sum_elements   msm on the routes buckets / quads / waves of tests/test_msm.py at n = 65 and 257, batches: z1 (affine + twin:
      the affine prepare kernel), z1_one_minus (the same with one minus record last: the flag and the shared-inversion prepare
      kernel), z1_one_scaled and z1_one_twin_scaled_inside (one scaled record last, one scaled twin at position 37: -A read
      as an affine record is twin(A), the same group element, so only another l shows a missed flag), all_kinds (planted), pair_same_scalar (every point as P and as twin(P) with one scalar: one bucket, the sum is
      2 sum k P), pair_cancelling (k and r - k: the all-zero Encoding) and all_identity (every term of the identity class).
      sum_elements at n = 1, 65, 257 on every layout, device tensors.
  msm_small   m = 1, 3, 8, n = 1, 65 sums, routes lanes (tiny_max = 0) and waves (tiny_max = 2^20).
  msm_long   m = 17 (three chains and a fold), n = 5.
  msm_buckets   (n, m, window_bits) = (3, 40, 4) and (3, 40, 12).
  msm_ragged (window_bits 4), msm_segmented (a lane and a wave context, as tests/test_segmented_sums_gpu.py makes them)
      lengths (0, 1, 8, 9, 17, 40, 0, 3).  msm_buckets and msm_ragged share msm's two prepare kernels: they also take the
      batches z1 and z1_one_scaled over the same shapes.
  msm_long_indexed   m = 9, n = 5; the pool is the planted mixed array of 64 points, the twin of every one of its records and
      the identity class; every sum names a point and its twin.
  FixedBases.msm_mixed   (v, t) = (1, 1) and (3, 2), n = 1 and 65, two random registered bases at 8 bits, the variable points the
      mixed array; planted: a variable twin of base 0 with r - k against k on base 0, an all-identity variable side, and for
      v = 3 a point and its twin with k and r - k.
  Every sums call: its terms are _representatives.sums_case -- the planted mixed array, and from three sums on one sum with a
      cancelling pair k P + (r - k) twin(P) (every other scalar 0) and one whose every term is of the identity class; the
      expected Encodings are oracle_fold / ragged_fold / indexed_fold_by_scalar_mul on the plain records.  Each also runs
      _representatives.special_sums, those two sums on their own (both the all-zero Encoding).

NOT HERE, and why.  Context.sharded("compress" / "scalar_mul_var_element") hands slices to the same launcher and kernels as the
calls above and needs the multi-GPU worker of tests/multigpu_worker.py.  msm_by_offsets only picks msm_segmented or msm_ragged.
The Element class is a thin wrapper over these calls.  Registered bases (FixedBases(points)) see a scaled record and a twin in
tests/test_fixed_bases_gpu.py and _sums_support.host_bases.  Calls that take Encodings decode to Z = 1 records themselves."""
import numpy as np
import pytest

import _representatives as rp
from _batch_msm_long_cases import oracle_fold
from _ragged_sums_cases import ragged_fold
from _sums_support import indexed_fold_by_scalar_mul, join, random_bases, var_terms

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
COUNT = 300
LENGTHS = (0, 1, 8, 9, 17, 40, 0, 3)

CODEC_ROUTES = {"default": {}, "four_per_wave": dict(tiny_max=1 << 20), "wide_grid": dict(tiny_max=0),
                "chunked": dict(decompress_chunked_min=1, tiny_max=0), "chunked_min_alone": dict(decompress_chunked_min=1)}
MUL_ROUTES = {"lanes_chunk1": dict(small_max=0, chunk_per_lane=1), "lanes_chunk8": dict(small_max=0, chunk_per_lane=8),
              "quads": dict(small_max=1 << 20, tiny_max=0), "waves": dict(tiny_max=1 << 20)}
MSM_ROUTES = {"buckets": dict(msm_small_max=0, msm_tiny_max=0), "quads": dict(msm_small_max=1000000, msm_tiny_max=0),
              "waves": dict(msm_small_max=1000000, msm_tiny_max=1000000)}
SMALL_ROUTES = {"lanes": dict(tiny_max=0), "waves": dict(tiny_max=1 << 20)}


@pytest.fixture(scope="module")
def ctxs():
    """route -> context: the library's routing, and tiny_max = 0 for the segmented sums' lane route."""
    import decaf377_amd as d
    out = {"wave": d.Context([0], comb_lazy=True), "lane": d.Context([0], comb_lazy=True)}
    out["lane"].set_tuning("tiny_max", 0)
    yield out
    for c in out.values():
        assert c.health()[0] == 0 and c.health()[2] == 0
        c.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs["wave"]


@pytest.fixture(scope="module")
def reps(oracle):
    return rp.build(oracle, 9200, COUNT)


def _layouts(reps, n):
    out = rp.layouts(reps, n, shift=n % 7)
    if n == 1:
        out["mixed"] = rp.mixed(reps, 1, shift=5, first=3)[:2]                     # the lone ordinary record: a scaled twin
    return out


def _rows(bad):
    return np.nonzero(bad.reshape(bad.shape[0], -1).any(1))[0][:8]


def _records(oracle, ctx, got, want, what):
    """(c): the records `got` are the group elements `want`, compress to the oracle's bytes and the first 16 are valid."""
    got = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 16)
    want = np.ascontiguousarray(want).reshape(-1, 16)
    eq = oracle.eq_xyzt(got, want)
    assert eq.all(), (what, np.nonzero(eq == 0)[0][:8])
    enc, want_enc = ctx.compress(got), oracle.compress(want)
    assert (enc == want_enc).all(), (what, _rows(enc != want_enc))
    rp.assert_valid(oracle, got[:16], what)


# ---- compress, compress_to_field ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(CODEC_ROUTES))
@pytest.mark.parametrize("call", ["compress", "compress_to_field"])
def test_compress(ctx, oracle, reps, call, route):
    with ctx.tuning(**CODEC_ROUTES[route]):
        for n in SIZES:
            for name, (P, PA) in _layouts(reps, n).items():
                got, want = getattr(ctx, call)(P), getattr(oracle, call)(PA)
                assert (got == want).all(), (call, route, n, name, "(a)", _rows(got != want))
                plain = getattr(ctx, call)(PA)
                assert (got == plain).all(), (call, route, n, name, "(b)", _rows(got != plain))
                ident = oracle.is_identity(PA) != 0
                assert not got[ident].any(), (call, route, n, name)


def test_compress_on_device_tensors(ctx, oracle, reps):
    import torch
    for name, (P, PA) in _layouts(reps, 257).items():
        Pd = torch.from_numpy(P.view(np.int64)).to("cuda:0")
        enc, f = ctx.compress(Pd), ctx.compress_to_field(Pd)
        torch.cuda.synchronize()
        assert (enc.cpu().numpy() == oracle.compress(PA)).all(), name
        assert (f.cpu().numpy().view(np.uint64) == oracle.compress_to_field(PA)).all(), name


# ---- eq -------------------------------------------------------------------------------------------------------------------------
def test_eq(ctx, oracle, reps):
    for n in SIZES:
        R, RA = rp.right_operands(oracle, reps, n, shift=n % 7)
        for name, (P, PA) in _layouts(reps, n).items():
            what = (n, name)
            assert ctx.eq(P, PA).all() and ctx.eq(PA, P).all(), what
            other, neg = np.roll(PA, 1, axis=0), oracle.neg_xyzt(PA)
            for Q, QA in ((other, other), (neg, neg), (R, RA), (oracle.neg_xyzt(P), neg)):
                got, want = ctx.eq(P, Q), oracle.eq_xyzt(PA, QA)
                assert (got == want).all(), (what, "(a)", np.nonzero(got != want)[0][:8])
                assert (ctx.eq(PA, QA) == got).all() and (ctx.eq(Q, P) == got).all(), (what, "(b)")
    I = reps.ident
    for a in range(6):
        assert ctx.eq(I, np.roll(I, a, axis=0)).all(), a
    assert not ctx.eq(I, reps.kinds["twin_scaled"][:I.shape[0]]).any()


# ---- is_identity, to_affine, neg, double, add, sub -------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["is_identity", "to_affine", "neg", "double", "add", "sub"])
def test_element_operations(ctx, oracle, reps, call):
    for n in SIZES:
        R, RA = rp.right_operands(oracle, reps, n, shift=n % 7)
        P0, PA0, names = rp.plant(reps, *rp.mixed(reps, n, shift=n % 7))
        for name, (P, PA) in _layouts(reps, n).items():
            what = (call, n, name)
            if call == "is_identity":
                got, want = ctx.is_identity(P), oracle.is_identity(PA)
                assert (got == want).all() and (ctx.is_identity(PA) == got).all(), (what, np.nonzero(got != want)[0][:8])
            elif call == "to_affine":
                got = ctx.to_affine(P)
                assert (got == oracle.to_affine(P)).all(), (what, _rows(got != oracle.to_affine(P)))
                if name == "mixed_planted":
                    assert (P == P0).all()
                    same = np.array([s in rp.SCALED_KINDS + ("affine",) for s in names])
                    assert (got[same] == oracle.to_affine(PA)[same]).all() and (ctx.to_affine(PA)[same] == got[same]).all(), what
            elif call == "neg":
                got = ctx.neg(P)
                assert (got == oracle.neg_xyzt(P)).all(), (what, _rows(got != oracle.neg_xyzt(P)))
                _records(oracle, ctx, got, oracle.neg_xyzt(PA), what)
            elif call == "double":
                got = ctx.double(P)
                _records(oracle, ctx, got, oracle.double_xyzt(PA), what)
                assert (ctx.compress(ctx.double(PA)) == ctx.compress(got)).all(), (what, "(b)")
            else:
                got = getattr(ctx, call)(P, R)
                _records(oracle, ctx, got, getattr(oracle, call + "_xyzt")(PA, RA), what)
                assert (ctx.compress(getattr(ctx, call)(PA, RA)) == ctx.compress(got)).all(), (what, "(b)")
                back = getattr(ctx, call)(R, P)                                    # the operands exchanged
                _records(oracle, ctx, back, getattr(oracle, call + "_xyzt")(RA, PA), what)


# ---- scalar_mul_var_element ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(MUL_ROUTES))
def test_scalar_mul_var_element(ctx, oracle, reps, route):
    with ctx.tuning(**MUL_ROUTES[route]):
        for n in SIZES:
            k = np.ascontiguousarray(np.roll(reps.scalars, 2, axis=0)[np.arange(n) % COUNT])
            if n >= 63:                                              # the twin kinds meet halves of both parities
                names = rp.mixed(reps, n, shift=n % 7)[2]
                odd = rp.half_is_odd(k)[[i for i, s in enumerate(names) if s in rp.TWIN_KINDS]]
                assert odd.any() and not odd.all(), n
            for name, (P, PA) in _layouts(reps, n).items():
                what = (route, n, name)
                got = ctx.scalar_mul_var_element(P, k)
                want = oracle.scalar_mul_xyzt(PA, k)
                enc, want_enc = ctx.compress(got), oracle.compress(want)
                assert (enc == want_enc).all(), (what, "(a)", _rows(enc != want_enc))
                plain = ctx.compress(ctx.scalar_mul_var_element(PA, k))
                assert (enc == plain).all(), (what, "(b)", _rows(enc != plain))
                _records(oracle, ctx, got, want, what)
                ident = oracle.is_identity(PA) != 0
                assert not enc[ident].any(), what


# ---- msm, sum_elements ------------------------------------------------------------------------------------------------------------
def _msm_batches(oracle, reps, n):
    """name -> (records, plain records, scalars); see the module docstring."""
    k = np.ascontiguousarray(np.roll(reps.scalars, 4, axis=0)[np.arange(n) % COUNT])
    out = {}
    P, PA, _ = rp.mixed(reps, n, kinds=("affine", "twin"))
    out["z1"] = (P, PA, k)
    P1 = P.copy()
    P1[n - 1] = reps.kinds["minus"][(n - 1) % COUNT]
    out["z1_one_minus"] = (P1, PA, k)
    # (-X, -Y, -1, -T) read as an affine record IS the twin, the same group element: a missed flag shows only with another l
    P2, P3 = P.copy(), P.copy()
    P2[n - 1] = reps.kinds["scaled"][(n - 1) % COUNT]
    out["z1_one_scaled"] = (P2, PA, k)
    P3[37] = reps.kinds["twin_scaled"][37]
    out["z1_one_twin_scaled_inside"] = (P3, PA, k)
    P, PA, names = rp.mixed(reps, n, shift=2)
    out["all_kinds"] = rp.plant(reps, P, PA, names)[:2] + (k,)
    h = n // 2
    L, LA, _ = rp.mixed(reps, h, kinds=("affine", "proj", "scaled", "minus"))
    T, TA, _ = rp.mixed(reps, h, kinds=rp.TWIN_KINDS)
    out["pair_same_scalar"] = (np.concatenate([L, T]), np.concatenate([LA, TA]), np.concatenate([k[:h], k[:h]]))
    rk = np.stack([rp.scalar_bytes((rp.R - int.from_bytes(bytes(row), "little") % rp.R) % rp.R) for row in k[:h]])
    out["pair_cancelling"] = (np.concatenate([L, T]), np.concatenate([LA, TA]), np.concatenate([k[:h], rk]))
    ni = reps.ident.shape[0]
    out["all_identity"] = (np.ascontiguousarray(reps.ident[np.arange(n) % ni]), np.tile(reps.ident[0], (n, 1)), k)
    return out


@pytest.mark.parametrize("route", sorted(MSM_ROUTES))
@pytest.mark.parametrize("n", [65, 257])
def test_msm(ctx, oracle, reps, n, route):
    with ctx.tuning(**MSM_ROUTES[route]):
        for name, (P, PA, k) in _msm_batches(oracle, reps, n).items():
            what = (route, n, name)
            enc, xyzt, _ = ctx.msm(P, k)
            want_enc, want = oracle.msm(PA, k)
            assert bytes(enc) == bytes(want_enc), (what, "(a)")
            assert bytes(ctx.msm(PA, k)[0]) == bytes(enc), (what, "(b)")
            _records(oracle, ctx, xyzt.reshape(1, 16), want.reshape(1, 16), what)
            if name in ("pair_cancelling", "all_identity"):
                assert not enc.any(), what
            if name == "pair_same_scalar":
                h = n // 2
                half = oracle.msm(PA[:h], k[:h])[1].reshape(1, 16)
                assert bytes(enc) == bytes(oracle.compress(oracle.double_xyzt(half))[0]), what


@pytest.mark.parametrize("n", [1, 65, 257])
def test_sum_elements(ctx, oracle, reps, n):
    import torch
    one = np.zeros((n, 32), np.uint8)
    one[:, 0] = 1
    for name, (P, PA) in _layouts(reps, n).items():
        enc, xyzt = ctx.sum_elements(torch.from_numpy(P.view(np.int64)).to("cuda:0"))
        plain = ctx.sum_elements(torch.from_numpy(PA.view(np.int64)).to("cuda:0"))[0]
        torch.cuda.synchronize()
        want_enc, want = oracle.msm(PA, one)
        assert bytes(enc.cpu().numpy()) == bytes(want_enc), (n, name, "(a)")
        assert bytes(plain.cpu().numpy()) == bytes(want_enc), (n, name, "(b)")
        _records(oracle, ctx, xyzt.cpu().numpy().view(np.uint64).reshape(1, 16), want.reshape(1, 16), (n, name))


# ---- the batched sums -----------------------------------------------------------------------------------------------------------
def _check_sums(oracle, ctx, call, P, PA, k, want, info, what):
    """call(points, scalars) -> (enc, xyzt): (a), (b) and (c) for one sums call; want: (encodings, records) of the oracle."""
    enc, xyzt = call(P, k)[:2]
    assert (enc == want[0]).all(), (what, "(a)", _rows(enc != want[0]))
    plain = call(PA, k)[0]
    assert (enc == plain).all(), (what, "(b)", _rows(enc != plain))
    _records(oracle, ctx, xyzt, want[1], what)
    for key in ("cancel", "identity"):
        if info.get(key) is not None:
            assert not enc[info[key]].any(), (what, key)


def _uniform(oracle, ctx, reps, call, n, m, what):
    """n sums of m terms through call(points, scalars) -> (enc, xyzt), then the two special sums on their own."""
    P, PA, k, _, info = rp.sums_case(reps, [m] * n, shift=(n + m) % 7)
    _check_sums(oracle, ctx, call, P, PA, k, oracle_fold(oracle, PA, k, m)[:2], info, what)
    P, PA, k = rp.special_sums(reps, m)
    want = oracle_fold(oracle, PA, k, m)[:2]
    assert not want[0].any()
    _check_sums(oracle, ctx, call, P, PA, k, want, {}, what + ("special",))


@pytest.mark.parametrize("route", sorted(SMALL_ROUTES))
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("m", [1, 3, 8])
def test_msm_small(ctx, oracle, reps, m, n, route):
    with ctx.tuning(**SMALL_ROUTES[route]):
        _uniform(oracle, ctx, reps, lambda P, k: ctx.msm_small(P, k, m, elements=True), n, m, ("msm_small", route, n, m))


def test_msm_long(ctx, oracle, reps):
    _uniform(oracle, ctx, reps, lambda P, k: ctx.msm_long(P, k, 17, elements=True), 5, 17, ("msm_long",))


def _z1_batches(reps, total):
    """The bucket pipeline's two prepare kernels (msm.hip): Z = 1 throughout (affine + twin) keeps the affine one; one scaled record
    last raises the flag for the shared-inversion one -> name -> (records, plain records, scalars)."""
    P, PA, _ = rp.mixed(reps, total, kinds=("affine", "twin"))
    P2 = P.copy()
    P2[total - 1] = reps.kinds["scaled"][(total - 1) % COUNT]
    k = np.ascontiguousarray(np.roll(reps.scalars, 4, axis=0)[np.arange(total) % COUNT])
    return {"z1": (P, PA, k), "z1_one_scaled": (P2, PA, k)}


@pytest.mark.parametrize("window_bits", [4, 12])
def test_msm_buckets(ctx, oracle, reps, window_bits):
    call = lambda P, k: ctx.msm_buckets(P, k, 40, elements=True, window_bits=window_bits)
    _uniform(oracle, ctx, reps, call, 3, 40, ("msm_buckets", window_bits))
    for name, (P, PA, k) in _z1_batches(reps, 120).items():
        _check_sums(oracle, ctx, call, P, PA, k, oracle_fold(oracle, PA, k, 40)[:2], {}, ("msm_buckets", window_bits, name))


def _by_offsets(oracle, ctx, reps, call, what):
    P, PA, k, off, info = rp.sums_case(reps, LENGTHS, shift=3)
    assert info == {"cancel": 2, "identity": 3}
    want = ragged_fold(oracle, PA, k, off)[:2]
    assert not want[0][[0, 6]].any()                                  # the empty sums
    _check_sums(oracle, ctx, lambda a, b: call(a, b, off), P, PA, k, want, info, what)
    for m in (2, 9):
        P, PA, k = rp.special_sums(reps, m)
        off2 = np.array([0, m, 2 * m], np.uint64)
        _check_sums(oracle, ctx, lambda a, b: call(a, b, off2), P, PA, k, ragged_fold(oracle, PA, k, off2)[:2], {"cancel": 0, "identity": 1},
                    what + ("special", m))


def test_msm_ragged(ctx, oracle, reps):
    call = lambda P, k, off: ctx.msm_ragged(P, k, off, elements=True, window_bits=4)
    _by_offsets(oracle, ctx, reps, call, ("msm_ragged",))
    off = rp.sums_case(reps, LENGTHS)[3]
    for name, (P, PA, k) in _z1_batches(reps, sum(LENGTHS)).items():
        _check_sums(oracle, ctx, lambda a, b: call(a, b, off), P, PA, k, ragged_fold(oracle, PA, k, off)[:2], {}, ("msm_ragged", name))


@pytest.mark.parametrize("route", ["lane", "wave"])
def test_msm_segmented(ctxs, oracle, reps, route):
    c = ctxs[route]
    _by_offsets(oracle, c, reps, lambda P, k, off: c.msm_segmented(P, k, off, elements=True), ("msm_segmented", route))


def test_msm_long_indexed(ctx, oracle, reps):
    m, n, pts = 9, 5, 64
    P, PA, names = rp.mixed(reps, pts, shift=1)
    P, PA, _ = rp.plant(reps, P, PA, names)
    ni = reps.ident.shape[0]
    pool = np.ascontiguousarray(np.concatenate([P, rp.twin(oracle, P), reps.ident]))
    plain = np.ascontiguousarray(np.concatenate([PA, PA, np.tile(reps.ident[0], (ni, 1))]))
    rp.assert_valid(oracle, pool[pts:pts + 16])
    assert oracle.eq_xyzt(pool, plain).all()
    rng = np.random.default_rng(9201)
    idx = rng.integers(0, 2 * pts, (n, m)).astype(np.int32)
    k = np.ascontiguousarray(np.roll(reps.scalars, 6, axis=0)[np.arange(n * m) % COUNT]).copy()
    for i in range(n):                                               # every sum names a point and its twin
        idx[i, 0], idx[i, 1] = 7 * i + 2, pts + 7 * i + 2
    idx[0, 5] = -1                                                   # an absent term
    idx[3, 2:5] = (0, 63, pts + 63)                                  # the planted identity-class records and a twin of one
    k[1 * m], k[1 * m + 1] = rp.cancelling_scalars(reps, 1)          # sum 1: k P + (r - k) twin(P), every other scalar 0
    k[1 * m + 2:2 * m] = 0
    idx[2] = 2 * pts + (np.arange(m) % ni)                           # sum 2: every term of the identity class
    want = indexed_fold_by_scalar_mul(oracle, plain, idx, k)
    assert not want[0][1].any() and not want[0][2].any()
    what = ("msm_long_indexed",)
    enc, xyzt = ctx.msm_long_indexed(pool, idx, k, m, elements=True)
    assert (enc == want[0]).all(), (what, "(a)", _rows(enc != want[0]))
    assert (ctx.msm_long_indexed(plain, idx, k, m) == enc).all(), (what, "(b)")
    _records(oracle, ctx, xyzt, want[1], what)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("v,t", [(1, 1), (3, 2)])
def test_msm_mixed(ctx, oracle, reps, v, t, n):
    rng = np.random.default_rng(9300 + 10 * v + t)
    bases = random_bases(oracle, rng, 2)
    P, PA, names = rp.mixed(reps, n * v, shift=(v + n) % 7)
    P, PA, _ = rp.plant(reps, P, PA, names)
    vk = np.ascontiguousarray(np.roll(reps.scalars, 1, axis=0)[np.arange(n * v) % COUNT]).copy()
    fk = np.ascontiguousarray(np.roll(reps.scalars, 9, axis=0)[np.arange(n * t) % COUNT]).copy()
    idx = rng.integers(0, 2, (n, t)).astype(np.int32)
    zero = []
    if n > 4:
        a, b = rp.cancelling_scalars(reps, 2)
        idx[1], idx[1, t - 1] = -1, 0                                # sum 1: k B_0 + (r - k) twin(B_0) as a scaled variable point
        fk[1 * t + t - 1], vk[1 * v:2 * v], vk[1 * v] = a, 0, b
        lam = rp.random_lambda(oracle, rng, 1)
        P[1 * v], PA[1 * v] = rp.scale(oracle, rp.twin(oracle, bases[0]), lam)[0], bases[0]
        rp.plant_identity_sum(reps, P, PA, vk, 2 * v, v)             # sum 2: the variable side all of the identity class
        zero = [1]
        if v >= 2:                                                   # sum 3: no fixed term, k P + (r - k) twin(P), the rest 0
            idx[3] = -1
            rp.plant_cancelling_pair(reps, P, PA, vk, 3 * v, v, which=3)
            zero.append(3)
    rp.assert_valid(oracle, P[:16])
    fixed = indexed_fold_by_scalar_mul(oracle, bases, idx, fk)[1]
    want = join(oracle, fixed, var_terms(oracle, PA, vk, n, v))
    assert not want[0][zero].any()
    what = ("msm_mixed", v, t, n)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        enc, xyzt = fb.msm_mixed(idx, fk, P, vk, elements=True)
        plain = fb.msm_mixed(idx, fk, PA, vk)
    assert (enc == want[0]).all(), (what, "(a)", _rows(enc != want[0]))
    assert (enc == plain).all(), (what, "(b)", _rows(enc != plain))
    _records(oracle, ctx, xyzt, want[1], what)
