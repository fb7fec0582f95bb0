"""The one long sum over 8- and 16-byte scalars on the MI355X (d377_msm_short, include/decaf377_amd_short_msm.h).

Every result is compared byte for byte with the oracle's fold on the scalars zero-extended to 32 bytes and with ctx.msm on the
same.  The short forms take the bucket route at every n (no wave route was kept for them); the comparisons run under the tuning
override that sends ctx.msm down the bucket route too.  Every case is a few thousand terms at the most, except one growth step
of 2^16."""
import ctypes

import numpy as np
import pytest

from _msm_short_cases import BITS, edge_scalars, extended, pick_window, py_shape, records
from _sums_support import Side, build_and_run_cpp

pytestmark = pytest.mark.gpu

ERR_ARG = -2
SIZES = [0, 1, 2, 5, 63, 64, 65, 257, 4097, 5000]               # what splits a wave, a workgroup and d377_msm's small-route boundary unevenly


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    c.set_tuning("msm_small_max", 0)                             # ctx.msm on the bucket route as well
    yield c
    assert c.health()[0] == 0 and c.health()[2] == 0
    c.close()


@pytest.fixture(scope="module")
def side(torch, ctx):
    return Side(torch, ctx)


@pytest.fixture(scope="module")
def pool(oracle):
    """5000 points once: projective records (Elligator outputs), their Encodings and the affine records those decode to."""
    rng = np.random.default_rng(377)
    proj = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (5000, 32), dtype=np.uint8)), dtype=np.uint64)
    enc = oracle.compress(proj)
    aff, st = oracle.decompress(enc)
    assert not st.any()
    return {"proj": proj, "enc": enc, "aff": np.ascontiguousarray(aff, dtype=np.uint64)}


def short_scalars(rng, n, nbytes, c=None):
    """n random records with the edge scalars of the width in use planted from the front"""
    rec = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    edges = records(edge_scalars(nbytes, c or pick_window(n)), nbytes)
    m = min(n, len(edges))
    rec[:m] = edges[:m]
    return rec


def want_of(oracle, pts, rec, keep=None):
    """The oracle's fold on the zero-extended scalars, over the terms `keep` marks."""
    k = extended(rec)
    if keep is not None:
        pts, k = pts[keep], k[keep]
    return oracle.msm(np.ascontiguousarray(pts), np.ascontiguousarray(k))[0]


def check_record(oracle, enc, xyzt):
    """xyzt_out compresses to enc32_out and satisfies T Z = X Y"""
    el = np.ascontiguousarray(np.asarray(xyzt).view(np.uint64).reshape(1, 16))
    assert bytes(oracle.compress(el)[0]) == bytes(enc)
    x, y, z, t = (np.ascontiguousarray(el[:, 4 * j:4 * j + 4]) for j in range(4))
    assert (oracle.fq_op(2, t, z)[0] == oracle.fq_op(2, x, y)[0]).all()


# ---- parity over n, lengths and forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 16])
@pytest.mark.parametrize("n", SIZES)
def test_short_sum_matches_oracle_and_msm(ctx, oracle, pool, n, nbytes):
    rng = np.random.default_rng(1000 * nbytes + n)
    rec = short_scalars(rng, n, nbytes)
    pts = pool["proj"][:n] if n % 2 else pool["aff"][:n]         # (odd n: Z != 1, the shared-inversion prepare; even: Z = 1)
    want = want_of(oracle, pts, rec)
    enc, xyzt, st = ctx.msm_short(pts, rec)
    assert st is None and bytes(enc) == bytes(want), (n, nbytes)
    assert bytes(ctx.msm(pts, extended(rec))[0]) == bytes(want)
    check_record(oracle, enc, xyzt)
    if n == 0:
        assert not enc.any()
    # uint64 words instead of bytes: the same records
    words = rec.view(np.uint64).reshape(n) if nbytes == 8 else rec.view(np.uint64).reshape(n, 2)
    assert bytes(ctx.msm_short(pts, words)[0]) == bytes(want)
    # Encodings, two of them invalid from 7 points on
    encs = pool["enc"][:n].copy()
    keep = np.ones(n, bool)
    if n >= 7:
        encs[3] = 0xFF
        encs[5, 31] = 0x80
        keep[[3, 5]] = False
    e2, x2, st2 = ctx.msm_short(encs, rec)
    assert list(np.nonzero(st2)[0]) == list(np.nonzero(~keep)[0])
    o_st = oracle.decompress(encs)[1] if n else np.zeros(0, np.uint8)
    assert ((st2 != 0) == (o_st != 0)).all()
    want2 = want_of(oracle, pool["aff"][:n], rec, keep)
    assert bytes(e2) == bytes(want2), (n, nbytes)
    e3, _, st3 = ctx.msm(encs, extended(rec))
    assert bytes(e3) == bytes(want2) and (st3 == st2).all()
    check_record(oracle, e2, x2)
    plan = ctx.msm_short_plan(n, nbytes)
    cw, W = py_shape(BITS[nbytes], pick_window(n))[:2]
    assert (plan["window_bits"], plan["windows"]) == (cw, W) and plan["workspace_bytes"] > 0


# ---- every window width ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 16])
def test_every_forced_window_width(ctx, oracle, pool, nbytes):
    n = 300
    for c in range(4, 17):
        rng = np.random.default_rng(100 * c + nbytes)
        rec = short_scalars(rng, n, nbytes, c)                   # the edge scalars of THIS width: +-2^(width-1) in every window
        want = want_of(oracle, pool["aff"][:n], rec)
        with ctx.tuning(msm_window=c):
            enc, xyzt, _ = ctx.msm_short(pool["aff"][:n], rec)
            plan = ctx.msm_short_plan(n, nbytes)
            full = ctx.msm(pool["aff"][:n], extended(rec))[0]
        assert bytes(enc) == bytes(want) == bytes(full), (c, nbytes)
        assert (plan["window_bits"], plan["windows"]) == py_shape(BITS[nbytes], c)[:2], (c, nbytes)
        check_record(oracle, enc, xyzt)
    with ctx.tuning(msm_window=18):                              # beyond 16 the short forms stay at 16: int16 digits
        assert ctx.msm_short_plan(n, nbytes)["windows"] == py_shape(BITS[nbytes], 16)[1]
        assert bytes(ctx.msm_short(pool["aff"][:n], rec)[0]) == bytes(want)


# ---- edge inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 16])
def test_edge_inputs(ctx, oracle, pool, nbytes):
    n = 700
    rng = np.random.default_rng(7 + nbytes)
    pts = pool["proj"][:n]
    # all scalars equal: one bucket per window holds everything, the reduction levels run
    for v in ((1 << (8 * nbytes)) - 1, int.from_bytes(rng.bytes(nbytes), "little")):
        rec = records([v] * n, nbytes)
        enc, xyzt, _ = ctx.msm_short(pts, rec)
        assert bytes(enc) == bytes(want_of(oracle, pts, rec)) == bytes(ctx.msm(pts, extended(rec))[0]), hex(v)
        check_record(oracle, enc, xyzt)
    # all scalars 0: the identity
    enc, xyzt, _ = ctx.msm_short(pts, np.zeros((n, nbytes), np.uint8))
    assert not enc.any() and oracle.is_identity(np.asarray(xyzt).view(np.uint64).reshape(1, 16)).all()
    # a third of the records with Z = 0: they count as the identity
    rec = short_scalars(rng, n, nbytes)
    dead = pts.copy()
    dead[1::3, 8:12] = 0
    keep = np.ones(n, bool)
    keep[1::3] = False
    want = want_of(oracle, pts, rec, keep)
    assert bytes(ctx.msm_short(dead, rec)[0]) == bytes(want) == bytes(ctx.msm(dead, extended(rec))[0])
    aff = pool["aff"][:n].copy()                                 # ... and among records with Z = 1
    aff[1::3, 8:12] = 0
    assert bytes(ctx.msm_short(aff, rec)[0]) == bytes(want)
    # Encodings with invalid entries, a seventh of them: statuses as the oracle's, left out of the sum
    encs = pool["enc"][:n].copy()
    encs[2::7, 31] |= 0x80
    encs[9::14] = 0xFF
    o_st = oracle.decompress(encs)[1]
    assert o_st[2::7].all() and o_st.sum() == len(o_st[2::7])
    e2, x2, st2 = ctx.msm_short(encs, rec)
    assert ((st2 != 0) == (o_st != 0)).all()
    assert bytes(e2) == bytes(want_of(oracle, pool["aff"][:n], rec, o_st == 0))
    check_record(oracle, e2, x2)


# ---- the device forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 16])
def test_dev_forms_on_a_side_stream_and_torch_tensors(ctx, oracle, pool, side, torch, nbytes):
    n = 1000
    rng = np.random.default_rng(50 + nbytes)
    rec = short_scalars(rng, n, nbytes)
    want = want_of(oracle, pool["proj"][:n], rec)
    d_pts, d_enc_in = side.dev(pool["proj"][:n]), side.dev(pool["enc"][:n])
    pad = side.dev(np.concatenate([np.zeros(nbytes // 2, np.uint8), rec.reshape(-1)]))    # the records at half their alignment
    d_rec = side.dev(rec)
    out, el, st = side.empty((32,), fill=0xA5), side.empty((16,), "u64"), side.empty((n,), fill=0xA5)
    side.ok("d377_msm_short_dev", d_pts, d_rec, nbytes, n, out, el)
    assert bytes(side.host(out)) == bytes(want)
    check_record(oracle, side.host(out), side.host(el))
    side.ok("d377_msm_short_dev", d_pts, d_rec, nbytes, n, out, None)            # without the Element record
    assert bytes(side.host(out)) == bytes(want)
    side.ok("d377_msm_short_encoded_dev", d_enc_in, d_rec, nbytes, n, out, el, st)
    assert bytes(side.host(out)) == bytes(want) and not side.host(st).any()
    # a misaligned scalars pointer is refused, and nothing is written
    out.fill_(0xA5)
    torch.cuda.synchronize()
    bad = ctypes.c_void_p(pad.data_ptr() + nbytes // 2)
    assert side.call("d377_msm_short_dev", d_pts, bad, nbytes, n, out, el) == ERR_ARG
    assert "aligned to scalar_bytes" in ctx._lib.d377_last_error().decode()
    assert side.call("d377_msm_short_encoded_dev", d_enc_in, bad, nbytes, n, out, el, st) == ERR_ARG
    assert (side.host(out) == 0xA5).all()
    if nbytes == 8:                                              # 8-byte records need no more than 8: an odd multiple of 8 is fine
        pad8 = side.dev(np.concatenate([np.zeros(8, np.uint8), rec.reshape(-1)]))
        side.ok("d377_msm_short_dev", d_pts, ctypes.c_void_p(pad8.data_ptr() + 8), nbytes, n, out, el)
        assert bytes(side.host(out)) == bytes(want)
    # the Python binding on tensors: torch's current stream, the _dev forms
    with torch.cuda.stream(side.stream):
        enc_t, xyzt_t, st_t = ctx.msm_short(d_pts, d_rec)
        words = d_rec.view(torch.int64)                          # [n, 1] or [n, 2] little-endian words
        enc_e, _, st_e = ctx.msm_short(d_enc_in, words.reshape(n) if nbytes == 8 else words)
    assert enc_t.is_cuda and st_t is None and bytes(side.host(enc_t)) == bytes(want)
    assert bytes(side.host(enc_e)) == bytes(want) and not side.host(st_e).any()
    check_record(oracle, side.host(enc_t), side.host(xyzt_t))
    with pytest.raises(ValueError, match="msm_short scalars"):
        ctx.msm_short(d_pts, rec)                                # device points with host scalars


def test_growth_and_the_workspace_shared_with_msm(oracle, pool, torch):
    """2^16 after 2^10 in one fresh context: the workspace grows between the calls; a full d377_msm_dev in between uses the same
    workspace and guard, on another stream."""
    import decaf377_amd as d
    ctx = d.Context([0], comb_lazy=True)
    try:
        side = Side(torch, ctx)
        rng = np.random.default_rng(65536)
        big = 1 << 16
        pts = np.tile(pool["aff"], (big // 5000 + 1, 1))[:big]
        rec = rng.integers(0, 256, (big, 16), dtype=np.uint8)
        mid = 1 << 12                                            # the full sum in between: past d377_msm's wave routes, on the buckets
        k32 = rng.integers(0, 256, (mid, 32), dtype=np.uint8)
        d_pts, d_rec, d_k32 = side.dev(pts), side.dev(rec), side.dev(k32)
        out = [side.empty((32,), fill=0xA5) for _ in range(3)]
        assert ctx.msm_short_plan(big, 16)["workspace_bytes"] > ctx.msm_short_plan(1 << 10, 16)["workspace_bytes"]
        side.ok("d377_msm_short_dev", d_pts, d_rec, 16, 1 << 10, out[0], None)
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):
            full = ctx.msm(d_pts[:mid], d_k32)[0]                # d377_msm_dev on a third stream: queues behind the short sum, grows
        side.ok("d377_msm_short_dev", d_pts, d_rec, 16, big, out[1], None)
        side.ok("d377_msm_short_dev", d_pts, d_rec, 16, 1 << 10, out[2], None)
        torch.cuda.synchronize()
        assert bytes(side.host(out[0])) == bytes(side.host(out[2])) == bytes(want_of(oracle, pts[:1 << 10], rec[:1 << 10]))
        assert bytes(side.host(out[1])) == bytes(want_of(oracle, pts, rec))
        assert bytes(full.cpu().numpy()) == bytes(oracle.msm(pts[:mid], k32)[0])
        assert ctx.health()[0] == 0 and ctx.health()[2] == 0
    finally:
        ctx.close()


# ---- the recipe the call exists for --------------------------------------------------------------------------------------------
def test_batch_verification_recipe(ctx, oracle, pool, side):
    """sum z_i R_i + sum w_i A_i with z short and w full: d377_msm_short_dev, d377_msm_dev, d377_batch_add_dev,
    d377_batch_compress_dev on one stream, against the oracle's fold of all 600 terms."""
    n = 300
    rng = np.random.default_rng(600)
    z = short_scalars(rng, n, 16)
    w = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    R, A = pool["proj"][:n], pool["aff"][n:2 * n]
    want = oracle.msm(np.concatenate([R, A]), np.concatenate([extended(z), w]))[0]
    d_R, d_A, d_z, d_w = side.dev(R), side.dev(A), side.dev(z), side.dev(w)
    a, b, s = side.empty((1, 16), "u64"), side.empty((1, 16), "u64"), side.empty((1, 16), "u64")
    scratch, out = side.empty((32,)), side.empty((1, 32), fill=0xA5)
    side.ok("d377_msm_short_dev", d_R, d_z, 16, n, scratch, a)
    side.ok("d377_msm_dev", d_A, d_w, n, scratch, b)
    side.ok("d377_batch_add_dev", a, b, 1, s)
    side.ok("d377_batch_compress_dev", s, 1, out)
    assert bytes(side.host(out)[0]) == bytes(want)


# ---- refusals on a live context, the C++ client ----------------------------------------------------------------------------------
def test_refusals_on_a_live_context(ctx, pool):
    import decaf377_amd as d
    rec = np.zeros((4, 16), np.uint8)
    lib = ctx._lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    enc = np.full(32, 0xA5, np.uint8)
    pts = np.ascontiguousarray(pool["aff"][:4])
    for sb in (0, 4, 12, 32):
        assert lib.d377_msm_short(ctx._h, p(pts), p(rec), sb, 4, p(enc), None) == ERR_ARG
        assert "scalar_bytes" in lib.d377_last_error().decode()
    assert lib.d377_msm_short_dev(ctx._h, 7, None, p(pts), p(rec), 16, 4, p(enc), None) == ERR_ARG
    assert "device index" in lib.d377_last_error().decode()
    assert (enc == 0xA5).all()
    with pytest.raises(d.NativeError, match="scalar_bytes"):
        ctx.msm_short_plan(4, 32)


def test_cpp_client():
    build_and_run_cpp("msm_short", "CPP_MSM_SHORT_OK", hip_headers=True)
