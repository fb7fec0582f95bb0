"""Many sums by the bucket method on the MI355X (d377_batch_bucket_msm, include/decaf377_amd_bucket_sums.h): the host forms
against the oracle's fold, Elements and Encodings with their statuses, on the shapes of the host walk (one term; one pass;
three passes; int32 keys; int16 keys whose magnitude reaches 2^15), a sum that sits in one bucket beside an ordinary one,
projective records; the library's own width at 129 and 4097 terms against d377_batch_msm_long and d377_msm; the resident forms
against the host forms; refusals on a live context; the Python routing; a captured graph that outlives the workspace it saw; a
device listed twice; the C++ mirror.  Every case is a few thousand terms at the most."""
import ctypes

import numpy as np
import pytest

from _bucket_sums_cases import WALK, assert_boundary_sums_cover, make_case, oracle_fold, passes, sums_per_pass, window_rule
from _sums_support import Side, build_and_run_cpp

pytestmark = pytest.mark.gpu

ERR_ARG = -2


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    assert c.health()[0] == 0 and c.health()[2] == 0
    c.close()


@pytest.fixture(scope="module")
def side(torch, ctx):
    return Side(torch, ctx)


def _check_host(ctx, oracle, pts, k, m, c, info=None):
    """The host form on (pts, k) against the oracle's fold -> (enc, el[, status])."""
    n = len(k) // m
    got = ctx.msm_buckets(pts, k, m, elements=True, window_bits=c)
    want_enc, want_el, want_st = oracle_fold(oracle, pts, k, m)
    tag = (n, m, c)
    assert (got[0] == want_enc).all(), (tag, np.nonzero((got[0] != want_enc).any(1))[0][:8])
    assert oracle.eq_xyzt(got[1], want_el).all(), tag
    assert (oracle.compress(np.ascontiguousarray(got[1])) == got[0]).all(), tag    # compress(xyzt_out) == enc32_out
    if want_st is not None:
        assert (got[2] == want_st).all(), tag
    plain = ctx.msm_buckets(pts, k, m, window_bits=c)            # without Element records
    assert ((plain[0] if isinstance(plain, tuple) else plain) == got[0]).all(), tag
    for s in (info or {}).get("identity", []):
        assert not got[0][s].any() and oracle.is_identity(got[1][s:s + 1]).all(), tag
    return got


@pytest.mark.parametrize("n,m,c", WALK)
def test_host_forms_match_oracle_fold(ctx, oracle, n, m, c):
    for encoded in (False, True):
        rng = np.random.default_rng(100 * n + m + encoded)
        pts, k, info = make_case(oracle, rng, n, m, c, encoded=encoded)
        if m >= 3:
            assert_boundary_sums_cover(k, info, m, c)
        got = _check_host(ctx, oracle, pts, k, m, c, info)
        if encoded and n * m >= 9:
            assert got[2].any()                                  # an invalid Encoding was there to report
    plan = ctx.msm_buckets_plan(n, m, c)
    assert plan["passes"] == len(passes(n, m, c)) and plan["window_bits"] == c


def test_one_bucket_holds_a_whole_sum_beside_an_ordinary_one(ctx, oracle):
    """(2, 700, 0): every scalar of sum 0 equal, so each window of sum 0 is one bucket of 700 points and the reduction levels
    run, beside sum 1 with random scalars."""
    n, m = 2, 700
    rng = np.random.default_rng(700)
    enc = oracle.compress(oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8)))
    pts = np.ascontiguousarray(oracle.decompress(enc)[0], dtype=np.uint64)
    assert (pts[:, 8:12] == pts[0, 8:12]).all()                  # every record has Z = 1 and none is dead: the affine prepare alone
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    k[:m] = k[0]
    _check_host(ctx, oracle, pts, k, m, 0)
    enc[5::11, 31] |= 0x40
    _check_host(ctx, oracle, enc, k, m, 0)


def test_projective_records_in_a_single_sum(ctx, oracle):
    n, m, c = 3, 40, 8
    pts, k, info = make_case(oracle, np.random.default_rng(340), n, m, c, projective=True)
    _check_host(ctx, oracle, pts, k, m, c, info)


def test_the_librarys_width_against_the_long_sums_and_msm(ctx, oracle):
    rng = np.random.default_rng(4097)
    for n, m in ((5, 129), (3, 4097)):                           # 4097: the first length d377_batch_msm_long refuses
        pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8)), dtype=np.uint64)
        k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
        pts.reshape(n * m, 4, 4)[7::13, 2] = 0
        enc, el = ctx.msm_buckets(pts, k, m, elements=True)
        plan = ctx.msm_buckets_plan(n, m)
        assert plan == {"window_bits": window_rule(m), "sums_per_pass": sums_per_pass(n, m, window_rule(m)), "passes": 1,
                        "workspace_bytes": plan["workspace_bytes"]} and plan["workspace_bytes"] > n * m * 128
        assert (oracle.compress(np.ascontiguousarray(el)) == enc).all()
        if m == 129:
            assert (enc == ctx.msm_long(pts, k, m)).all()
            assert (enc == oracle_fold(oracle, pts, k, m)[0]).all()
        else:
            import decaf377_amd as d
            with pytest.raises(d.NativeError, match="m = 4097"):
                ctx.msm_long(pts, k, m)
            for s in range(n):
                one = ctx.msm(pts[s * m:(s + 1) * m], k[s * m:(s + 1) * m])
                one_enc = one[0] if isinstance(one, tuple) else one
                assert (np.asarray(one_enc).reshape(-1) == enc[s]).all(), s


def _resident_equals_host(ctx, side, oracle, n, m, c, seed):
    for encoded in (False, True):
        pts, k, _ = make_case(oracle, np.random.default_rng(seed + encoded), n, m, c, encoded=encoded)
        want = ctx.msm_buckets(pts, k, m, elements=True, window_bits=c)
        enc, el = side.empty((n, 32), fill=0xA5), side.empty((n, 16), "u64", fill=0x5A5A)
        if encoded:
            st = side.empty((n * m,), fill=0xEE)
            side.ok("d377_batch_bucket_msm_encoded_resident", side.dev(pts), side.dev(k), m, n, c, enc, el, st)
            assert (side.host(st) == want[2]).all(), (n, m, c)
        else:
            side.ok("d377_batch_bucket_msm_resident", side.dev(pts), side.dev(k), m, n, c, enc, el)
        assert (side.host(enc) == want[0]).all(), (n, m, c, encoded)
        assert oracle.eq_xyzt(side.host(el), want[1]).all(), (n, m, c, encoded)
        enc2 = side.empty((n, 32), fill=0xA5)                    # without Element records
        if encoded:
            side.ok("d377_batch_bucket_msm_encoded_resident", side.dev(pts), side.dev(k), m, n, c, enc2, None, st)
        else:
            side.ok("d377_batch_bucket_msm_resident", side.dev(pts), side.dev(k), m, n, c, enc2, None)
        assert (side.host(enc2) == want[0]).all(), (n, m, c, encoded)


@pytest.mark.parametrize("n,m,c", [(3, 5, 4), (9, 33, 16), (17, 40, 12), (5, 129, 0)])
def test_resident_forms_equal_the_host_forms(ctx, side, oracle, n, m, c):
    _resident_equals_host(ctx, side, oracle, n, m, c if c else window_rule(m), 900 + m)
    if c == 0:
        pts, k, _ = make_case(oracle, np.random.default_rng(5), n, m, window_rule(m))
        enc = side.empty((n, 32), fill=0xA5)
        side.ok("d377_batch_bucket_msm_resident", side.dev(pts), side.dev(k), m, n, 0, enc, None)
        assert (side.host(enc) == ctx.msm_buckets(pts, k, m)).all()


def test_refusals_on_a_live_context(ctx, side, oracle):
    n, m = 3, 17
    pts, k, _ = make_case(oracle, np.random.default_rng(17), n, m, window_rule(m))
    lib = ctx._lib
    dp, dk = side.dev(pts), side.dev(k)
    enc, el = side.empty((n, 32), fill=0x5A), side.empty((n, 16), "u64", fill=0x5A5A)
    off = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)       # noqa: E731
    msg = lambda: lib.d377_last_error().decode()                  # noqa: E731
    name = "d377_batch_bucket_msm_resident"
    assert side.call(name, off(dp, 8), dk, m, n, 0, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, off(dk, 8), m, n, 0, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, m, n, 0, off(enc, 8), el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, m, n, 0, enc, off(el, 8)) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, m, n, 3, enc, el) == ERR_ARG and "window_bits = 3" in msg()
    assert side.call(name, dp, dk, 0, n, 0, enc, el) == ERR_ARG and "m = 0" in msg()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    for bad_dev in (-1, 1):
        args = (ctx._h, bad_dev, ctypes.c_void_p(side.stream.cuda_stream))
        assert lib.d377_batch_bucket_msm_resident(*args, p(dp), p(dk), m, n, 0, p(enc), p(el)) == ERR_ARG and "dev" in msg()
        assert lib.d377_bucket_msm_plan(ctx._h, bad_dev, n, m, 0, None, None, None, None) == ERR_ARG and "dev" in msg()
    assert side.call(name, None, None, m, 0, 0, None, None) == 0                    # n == 0 with good arguments
    assert side.call("d377_batch_bucket_msm_encoded_resident", None, None, m, 0, 0, None, None, None) == 0
    assert (side.host(enc) == 0x5A).all() and (side.host(el) == 0x5A5A).all()
    assert ctx.msm_buckets_plan(0, m)["passes"] == 0


def test_python_routes_by_device(torch, oracle, monkeypatch):
    import decaf377_amd as d
    n, m = 3, 17
    pts, k, _ = make_case(oracle, np.random.default_rng(31), n, m, window_rule(m))
    raw, _, _ = make_case(oracle, np.random.default_rng(31), n, m, window_rule(m), encoded=True)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")   # noqa: E731
    c = d.Context([0], comb_lazy=True)
    try:
        want = c.msm_buckets(pts, k, m, elements=True)
        enc, el = c.msm_buckets(T(pts), T(k), m, elements=True)
        assert str(enc.device) == "cuda:0" and str(el.device) == "cuda:0"
        assert (enc.cpu().numpy() == want[0]).all() and oracle.eq_xyzt(el.cpu().numpy().view(np.uint64), want[1]).all()
        outs = [torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda:0")]
        assert c.msm_buckets(T(pts), T(k), m, outs=outs, window_bits=9) is outs[0] and (outs[0].cpu().numpy() == want[0]).all()
        w_enc, w_st = c.msm_buckets(raw, k, m)
        r_enc, r_st = c.msm_buckets(T(raw), T(k), m)
        assert (r_enc.cpu().numpy() == w_enc).all() and (r_st.cpu().numpy() == w_st).all() and w_st.any()
        with pytest.raises(d.NativeError, match="no CPU path"):  # as msm_long: a tensor lives on a GPU
            c.msm_buckets(torch.from_numpy(pts.view(np.int64)), torch.from_numpy(k), m)
        monkeypatch.setattr(c, "device_ids", [7])                # a GPU the context does not own: staged through the host
        got = c.msm_buckets(T(pts), T(k), m)
        monkeypatch.undo()
        assert str(got.device) == "cuda:0" and (got.cpu().numpy() == want[0]).all()
        with pytest.raises(d.NativeError, match="window_bits = 17"):
            c.msm_buckets(T(pts), T(k), m, window_bits=17)
    finally:
        c.close()


def test_graph_replays_and_outlives_the_workspace_it_saw(torch, oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(99)
    n, m, wb = 3, 17, 6
    pts, k, _ = make_case(oracle, rng, n, m, wb)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no workspace has grown yet
    try:
        s = Side(torch, c)
        dpts, dk, out = s.dev(pts), s.dev(k), s.empty((n, 32))

        def enqueue(stream):
            s.ok("d377_batch_bucket_msm_resident", dpts, dk, m, n, wb, out, None, stream=stream)

        def expect(what):
            torch.cuda.synchronize()
            hk = dk.cpu().numpy()
            assert (out.cpu().numpy() == oracle_fold(oracle, pts, hk, m)[0]).all(), what

        enqueue(None)                                            # one eager call of the shape: the workspace grows here
        expect("eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                # one stream, a linear graph
            enqueue(torch.cuda.current_stream().cuda_stream)

        def overwrite():
            dk.copy_(torch.from_numpy(rng.integers(0, 256, tuple(dk.shape), dtype=np.uint8)))
            out.zero_()
            torch.cuda.synchronize()

        overwrite()
        g.replay()
        expect("replay")
        small = c.msm_buckets_plan(n, m, wb)["workspace_bytes"]
        bn, bm = 5, 600                                          # a larger eager call that outgrows the workspace the graph saw
        assert c.msm_buckets_plan(bn, bm, wb)["workspace_bytes"] > 2 * small
        bp, bk, _ = make_case(oracle, rng, bn, bm, wb)
        assert (c.msm_buckets(bp, bk, bm, window_bits=wb) == oracle_fold(oracle, bp, bk, bm)[0]).all()
        overwrite()
        g.replay()                                               # the old graph, into the workspace it was captured with
        expect("replay after the workspace was outgrown")
        claimed, _, gave_up = c.health()
        assert (claimed, gave_up) == (0, 0)
    finally:
        c.close()


def test_device_listed_twice_slices_the_sums(oracle):
    import decaf377_amd as d
    n, m, c = 5, 33, 7
    pts, k, _ = make_case(oracle, np.random.default_rng(533), n, m, c)
    raw, _, _ = make_case(oracle, np.random.default_rng(533), n, m, c, encoded=True)
    c2 = d.Context([0, 0], comb_lazy=True)
    try:
        enc, el = c2.msm_buckets(pts, k, m, elements=True, window_bits=c)
        want_enc, want_el, _ = oracle_fold(oracle, pts, k, m)
        assert (enc == want_enc).all() and oracle.eq_xyzt(el, want_el).all()       # the sums in order, Element records in place
        r_enc, r_st = c2.msm_buckets(raw, k, m)
        w_enc, _, w_st = oracle_fold(oracle, raw, k, m)
        assert (r_enc == w_enc).all() and (r_st == w_st).all()
        assert c2.health(0)[0] == 0 and c2.health(1)[0] == 0
    finally:
        c2.close()


def test_cpp_mirror_bucket_sums():
    build_and_run_cpp("bucket_sums", "CPP_BUCKET_SUMS_OK", hip_headers=True)


# (n, m, window_bits): 2^20 terms each.  12 bits: one pass, 17 super-buckets, 32 points to a bucket; 16 bits: four passes of four
# sums, 1025 super-buckets (the widest level 1 the sort has), int32 keys; the library's own width.  Every window is 128 tiles of
# the sort and more, in several slices.
LARGE = [(16, 1 << 16, 12), (16, 1 << 16, 16), (256, 1 << 12, 0)]


@pytest.mark.parametrize("n,m,c", LARGE)
def test_element_records_are_reproducible_byte_for_byte_at_large_shapes(ctx, torch, n, m, c):
    """Two runs of one call on one input return the same Element record BYTES, and the ragged call with equal lengths returns
    them too, where the sort walks many tiles per workgroup, several slices per window and up to 1025 bins: the order of a
    bucket's points is a function of the inputs (msm.hip tile_scatter, ORDERED).  The sums themselves: every
    Encoding equals d377_msm's for that sum (another sort order, single-sum keys), and the records compress to them."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7700 + c)
    pts = ctx.encode_to_curve_element(torch.randint(0, 256, (n * m, 32), dtype=torch.uint8, device=dev, generator=g))
    k = torch.randint(0, 256, (n * m, 32), dtype=torch.uint8, device=dev, generator=g)
    k[::1001] = k[0]                                             # one scalar on a thousand points: long runs in one bucket of every window
    runs = [ctx.msm_buckets(pts, k, m, elements=True, window_bits=c) for _ in range(3)]
    runs.append(ctx.msm_ragged(pts, k, np.arange(n + 1, dtype=np.uint64) * m, elements=True, window_bits=c))
    torch.cuda.synchronize()
    for enc, el in runs[1:]:
        assert torch.equal(enc, runs[0][0]) and torch.equal(el, runs[0][1]), (n, m, c)
    enc, el = runs[0]
    assert torch.equal(ctx.compress(el), enc)
    for s in (0, n // 2, n - 1):
        one = ctx.msm(pts[s * m:(s + 1) * m], k[s * m:(s + 1) * m])[0]
        assert torch.equal(one, enc[s]), (n, m, c, s)
