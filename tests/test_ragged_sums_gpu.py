"""Many sums of any length each on the MI355X (d377_batch_ragged_msm, include/decaf377_amd_ragged_sums.h): the host forms against
the oracle's fold per sum, Elements and Encodings with their statuses, on the cases of tests/_ragged_sums_cases.py (passes with
and without points, empty sums at both ends, more sums than lanes in a tile, sums across tile and wave boundaries, int32 keys,
int16 keys that reach 2^15); one sum against d377_msm; the library's width against the long sums; equal lengths against
d377_batch_bucket_msm, byte for byte; the resident forms against the host forms; refusals on a live context; the Python routing;
a captured graph that outlives the workspace it saw; a device listed twice; the C++ mirror.  Every case is a few thousand terms
at the most."""
import ctypes

import numpy as np
import pytest

import _bucket_sums_cases as bc
from _ragged_sums_cases import CASES, WIDTH_CASE, assert_cover_sums_cover, device_cuts, make_case, offsets_of, passes, ragged_fold, width
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


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> encoded -> (points, scalars, offsets, info, the oracle's (enc, el, status)), made once and left unchanged."""
    out = {}
    for name, (lengths, c) in CASES.items():
        out[name] = {}
        for encoded in (False, True):
            pts, k, off, info = make_case(oracle, np.random.default_rng(len(lengths) * 1000 + c + encoded), lengths, c, encoded=encoded)
            out[name][encoded] = (pts, k, off, info, ragged_fold(oracle, pts, k, off))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_forms_match_oracle_fold(ctx, oracle, cases, name):
    c = CASES[name][1]
    for encoded in (False, True):
        pts, k, off, info, (want_enc, want_el, want_st) = cases[name][encoded]
        assert_cover_sums_cover(k, off, info, c)
        got = ctx.msm_ragged(pts, k, off, elements=True, window_bits=c)
        assert (got[0] == want_enc).all(), (name, encoded, np.nonzero((got[0] != want_enc).any(1))[0][:8])
        assert oracle.eq_xyzt(got[1], want_el).all(), (name, encoded)
        assert (oracle.compress(np.ascontiguousarray(got[1])) == got[0]).all(), (name, encoded)
        if encoded:
            assert (got[2] == want_st).all() and got[2].any(), name
        plain = ctx.msm_ragged(pts, k, off, window_bits=c)        # without Element records
        assert ((plain[0] if isinstance(plain, tuple) else plain) == got[0]).all(), name
        for s in info["empty"]:
            assert not got[0][s].any() and oracle.is_identity(got[1][s:s + 1]).all(), (name, s)
    plan = ctx.msm_ragged_plan(off, c)
    cuts = passes(off, c)
    assert plan["passes"] == len(cuts) and plan["window_bits"] == c
    assert plan["max_sums_per_pass"] == max(K for _, K, _ in cuts) and plan["max_points_per_pass"] == max(n for _, _, n in cuts)


def test_one_sum_gives_the_bytes_of_msm(ctx, oracle):
    pts, k, off, info = make_case(oracle, np.random.default_rng(300), (300,), bc.window_rule(300))
    enc, el = ctx.msm_ragged(pts, k, off, elements=True)
    one = ctx.msm(pts, k)
    assert (np.asarray(one[0]).reshape(-1) == enc[0]).all()
    assert oracle.eq_xyzt(np.asarray(one[1]).reshape(1, 16), el).all()
    assert (enc == ragged_fold(oracle, pts, k, off)[0]).all()


def test_the_librarys_width_against_the_fold_and_the_long_sums(ctx, oracle):
    lengths, _ = WIDTH_CASE
    off = offsets_of(lengths)
    rng = np.random.default_rng(6762)
    terms = int(off[-1])
    pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (terms, 32), dtype=np.uint8)), dtype=np.uint64)   # Z != 1
    k = rng.integers(0, 256, (terms, 32), dtype=np.uint8)
    pts.reshape(terms, 4, 4)[7::13, 2] = 0
    enc, el = ctx.msm_ragged(pts, k, off, elements=True)
    plan = ctx.msm_ragged_plan(off)
    assert plan["window_bits"] == width(off) == bc.window_rule(1127) and plan["passes"] == 1 and plan["workspace_bytes"] > terms * 128
    assert (plan["max_sums_per_pass"], plan["max_points_per_pass"]) == (6, terms)
    assert (oracle.compress(np.ascontiguousarray(el)) == enc).all()
    assert (enc == ragged_fold(oracle, pts, k, off)[0]).all()
    assert not enc[4].any()
    for s, m in enumerate(lengths):                              # d377_batch_msm_long per distinct length (all are at most 4096)
        if m:
            lo, hi = int(off[s]), int(off[s + 1])
            assert (ctx.msm_long(pts[lo:hi], k[lo:hi], m)[0] == enc[s]).all(), s


@pytest.mark.parametrize("n,m,c", bc.WALK)
def test_equal_lengths_give_the_bytes_of_the_bucket_form(ctx, oracle, n, m, c):
    off = offsets_of([m] * n)
    for encoded in (False, True):
        pts, k, _ = bc.make_case(oracle, np.random.default_rng(100 * n + m + encoded), n, m, c, encoded=encoded)
        want = ctx.msm_buckets(pts, k, m, elements=True, window_bits=c)
        got = ctx.msm_ragged(pts, k, off, elements=True, window_bits=c)
        assert len(got) == len(want)
        for g, w in zip(got[::2], want[::2]):                     # Encodings and statuses: byte for byte
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (n, m, c, encoded)
        assert oracle.eq_xyzt(got[1], want[1]).all(), (n, m, c, encoded)
    for wb in (c, 0):
        u, r = ctx.msm_buckets_plan(n, m, wb), ctx.msm_ragged_plan(off, wb)
        assert (r["window_bits"], r["passes"], r["workspace_bytes"], r["max_sums_per_pass"]) == \
            (u["window_bits"], u["passes"], u["workspace_bytes"], u["sums_per_pass"]), (n, m, wb)


@pytest.mark.parametrize("n,m,c", bc.WALK)
def test_equal_lengths_give_the_element_record_bytes_of_the_bucket_form(ctx, oracle, n, m, c):
    """The Element records of the two calls, byte for byte: the check the feature's specification sets, kept as it sets it.

    It used to fail at (17, 40, 12) and (16, 40, 12) whenever d377_batch_bucket_msm did not reproduce its own record bytes: the
    sort ordered the points of a bucket by the arrival of LDS atomics, and the uniform call's record of a sum differed between
    two of its own runs, in the same row in which the two calls differed.  A call that returns records now sorts in an order that
    is a function of the inputs (msm.hip tile_scatter, ORDERED), and so are the record bytes of both calls."""
    off = offsets_of([m] * n)
    for encoded in (False, True):
        pts, k, _ = bc.make_case(oracle, np.random.default_rng(100 * n + m + encoded), n, m, c, encoded=encoded)
        want = ctx.msm_buckets(pts, k, m, elements=True, window_bits=c)
        got = ctx.msm_ragged(pts, k, off, elements=True, window_bits=c)
        assert got[1].dtype == want[1].dtype and got[1].shape == want[1].shape
        assert (got[1] == want[1]).all(), (n, m, c, encoded, np.nonzero((got[1] != want[1]).any(1))[0].tolist())


@pytest.mark.parametrize("name", sorted(CASES))
def test_resident_forms_equal_the_host_forms(ctx, side, cases, oracle, name):
    c = CASES[name][1]
    for encoded in (False, True):
        pts, k, off, _, _ = cases[name][encoded]
        n = len(off) - 1
        want = ctx.msm_ragged(pts, k, off, elements=True, window_bits=c)
        enc, el = side.empty((n, 32), fill=0xA5), side.empty((n, 16), "u64", fill=0x5A5A)
        doff = side.dev(off)
        if encoded:
            st = side.empty((len(k),), fill=0xEE)
            side.ok("d377_batch_ragged_msm_encoded_resident", side.dev(pts), side.dev(k), off.ctypes.data_as(ctypes.c_void_p), doff, n, c, enc, el, st)
            assert (side.host(st) == want[2]).all(), name
        else:
            side.ok("d377_batch_ragged_msm_resident", side.dev(pts), side.dev(k), off.ctypes.data_as(ctypes.c_void_p), doff, n, c, enc, el)
        assert (side.host(enc) == want[0]).all(), (name, encoded)
        assert oracle.eq_xyzt(side.host(el), want[1]).all(), (name, encoded)
        enc2 = side.empty((n, 32), fill=0xA5)                    # without Element records
        if encoded:
            side.ok("d377_batch_ragged_msm_encoded_resident", side.dev(pts), side.dev(k), off.ctypes.data_as(ctypes.c_void_p), doff, n, c, enc2,
                    None, st)
        else:
            side.ok("d377_batch_ragged_msm_resident", side.dev(pts), side.dev(k), off.ctypes.data_as(ctypes.c_void_p), doff, n, c, enc2, None)
        assert (side.host(enc2) == want[0]).all(), (name, encoded)


def test_refusals_on_a_live_context(torch, ctx, side, oracle):
    lengths = (3, 0, 17, 5)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(17), lengths, 6)
    n = len(lengths)
    lib = ctx._lib
    dp, dk, doff = side.dev(pts), side.dev(k), side.dev(off)
    hoff = off.ctypes.data_as(ctypes.c_void_p)
    enc, el = side.empty((n, 32), fill=0x5A), side.empty((n, 16), "u64", fill=0x5A5A)
    shift = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)     # noqa: E731
    msg = lambda: lib.d377_last_error().decode()                  # noqa: E731
    name = "d377_batch_ragged_msm_resident"
    assert side.call(name, shift(dp, 8), dk, hoff, doff, n, 0, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, shift(dk, 8), hoff, doff, n, 0, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, doff, n, 0, shift(enc, 8), el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, doff, n, 0, enc, shift(el, 8)) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, shift(doff, 4), n, 0, enc, el) == ERR_ARG and "offsets_dev" in msg() and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, None, n, 0, enc, el) == ERR_ARG and "offsets_dev" in msg()
    assert side.call(name, dp, dk, hoff, doff, n, 3, enc, el) == ERR_ARG and "window_bits = 3" in msg()
    bad = np.array([0, 3, 2, 20, 25], np.uint64)
    assert side.call(name, dp, dk, bad.ctypes.data_as(ctypes.c_void_p), doff, n, 0, enc, el) == ERR_ARG and "sum 1" in msg()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    for bad_dev in (-1, 1):
        args = (ctx._h, bad_dev, ctypes.c_void_p(side.stream.cuda_stream))
        assert lib.d377_batch_ragged_msm_resident(*args, p(dp), p(dk), hoff, p(doff), n, 0, p(enc), p(el)) == ERR_ARG and "dev" in msg()
        assert lib.d377_ragged_msm_plan(ctx._h, bad_dev, hoff, n, 0, None, None, None, None, None) == ERR_ARG and "dev" in msg()
    assert side.call(name, None, None, None, None, 0, 0, None, None) == 0                    # n == 0 with good arguments
    assert side.call("d377_batch_ragged_msm_encoded_resident", None, None, None, None, 0, 0, None, None, None) == 0
    assert (side.host(enc) == 0x5A).all() and (side.host(el) == 0x5A5A).all()
    assert ctx.msm_ragged_plan([0])["passes"] == 0 and ctx.msm_ragged_plan([0, 0, 0]) == {
        "window_bits": bc.window_rule(1), "passes": 1, "max_sums_per_pass": 2, "max_points_per_pass": 0, "workspace_bytes": 0}
    # sums without a term need no term buffers
    none = np.zeros(3, np.uint64)
    assert side.call(name, None, None, none.ctypes.data_as(ctypes.c_void_p), side.dev(none), 2, 0, enc, None) == 0
    assert (side.host(enc)[:2] == 0).all() and (side.host(enc)[2:] == 0x5A).all()


def test_a_capture_of_a_shape_never_run_eagerly_is_refused(torch, oracle):
    import decaf377_amd as d
    lengths = (3, 0, 17, 5)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(18), lengths, 6)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no workspace has grown yet
    try:
        s = Side(torch, c)
        dp, dk, doff, out = s.dev(pts), s.dev(k), s.dev(off), s.empty((len(lengths), 32), fill=0x5A)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rc = s.call("d377_batch_ragged_msm_resident", dp, dk, off.ctypes.data_as(ctypes.c_void_p), doff, len(lengths), 6, out, None,
                        stream=torch.cuda.current_stream().cuda_stream)
            text = c._lib.d377_last_error().decode()
        assert rc == ERR_ARG and "capture" in text
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0x5A).all()
    finally:
        c.close()


def test_python_routes_by_device(torch, oracle, monkeypatch):
    import decaf377_amd as d
    lengths = (3, 0, 17, 5)
    n = len(lengths)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(31), lengths, 6)
    raw, _, _, _ = make_case(oracle, np.random.default_rng(31), lengths, 6, encoded=True)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")   # noqa: E731
    c = d.Context([0], comb_lazy=True)
    try:
        want = c.msm_ragged(pts, k, off, elements=True)
        assert (want[0] == c.msm_ragged(pts, k, [int(v) for v in off])).all()          # offsets as a list
        enc, el = c.msm_ragged(T(pts), T(k), off, elements=True)
        assert str(enc.device) == "cuda:0" and str(el.device) == "cuda:0"
        assert (enc.cpu().numpy() == want[0]).all() and oracle.eq_xyzt(el.cpu().numpy().view(np.uint64), want[1]).all()
        outs = [torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda:0")]
        got = c.msm_ragged(T(pts), T(k), off.astype(np.int64), outs=outs, window_bits=9, offsets_dev=T(off))
        assert got is outs[0] and (outs[0].cpu().numpy() == want[0]).all()
        with pytest.raises(ValueError, match="offsets_dev"):
            c.msm_ragged(T(pts), T(k), off, offsets_dev=T(off)[:n])
        w_enc, w_st = c.msm_ragged(raw, k, off)
        r_enc, r_st = c.msm_ragged(T(raw), T(k), off)
        assert (r_enc.cpu().numpy() == w_enc).all() and (r_st.cpu().numpy() == w_st).all() and w_st.any() and len(w_st) == int(off[-1])
        with pytest.raises(d.NativeError, match="no CPU path"):
            c.msm_ragged(torch.from_numpy(pts.view(np.int64)), torch.from_numpy(k), off)
        monkeypatch.setattr(c, "device_ids", [7])                # a GPU the context does not own: staged through the host
        got = c.msm_ragged(T(pts), T(k), off)
        monkeypatch.undo()
        assert str(got.device) == "cuda:0" and (got.cpu().numpy() == want[0]).all()
        with pytest.raises(d.NativeError, match="window_bits = 17"):
            c.msm_ragged(T(pts), T(k), off, window_bits=17)
    finally:
        c.close()


def test_graph_replays_and_outlives_the_workspace_it_saw(torch, oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(99)
    lengths, wb = (3, 0, 17, 5), 6
    n = len(lengths)
    pts, k, off, _ = make_case(oracle, rng, lengths, wb)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no workspace has grown yet
    try:
        s = Side(torch, c)
        dpts, dk, doff, out = s.dev(pts), s.dev(k), s.dev(off), s.empty((n, 32))
        hoff = off.ctypes.data_as(ctypes.c_void_p)

        def enqueue(stream):
            s.ok("d377_batch_ragged_msm_resident", dpts, dk, hoff, doff, n, wb, out, None, stream=stream)

        def expect(what):
            torch.cuda.synchronize()
            hk = dk.cpu().numpy()
            assert (out.cpu().numpy() == ragged_fold(oracle, pts, hk, off)[0]).all(), what

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
        small = c.msm_ragged_plan(off, wb)["workspace_bytes"]
        big = (600, 1, 0, 900, 1500)                             # a larger eager call that outgrows the workspace the graph saw
        bp, bk, boff, _ = make_case(oracle, rng, big, wb)
        assert c.msm_ragged_plan(boff, wb)["workspace_bytes"] > 2 * small
        assert (c.msm_ragged(bp, bk, boff, window_bits=wb) == ragged_fold(oracle, bp, bk, boff)[0]).all()
        overwrite()
        g.replay()                                               # the old graph, into the workspace it was captured with
        expect("replay after the workspace was outgrown")
        claimed, _, gave_up = c.health()
        assert (claimed, gave_up) == (0, 0)
    finally:
        c.close()


def test_device_listed_twice_slices_the_sums_by_terms(ctx, oracle):
    import decaf377_amd as d
    lengths, c = (200, 1, 0, 33, 7, 0, 60, 0), 7
    pts, k, off, _ = make_case(oracle, np.random.default_rng(533), lengths, c)
    raw, _, _, _ = make_case(oracle, np.random.default_rng(533), lengths, c, encoded=True)
    assert device_cuts(off, 2) == [0, 1, 8]                      # by terms: the long sum alone on the first device
    c2 = d.Context([0, 0], comb_lazy=True)
    try:
        enc, el = c2.msm_ragged(pts, k, off, elements=True, window_bits=c)
        one_enc, one_el = ctx.msm_ragged(pts, k, off, elements=True, window_bits=c)
        want_enc, want_el, _ = ragged_fold(oracle, pts, k, off)
        assert (enc == one_enc).all() and (enc == want_enc).all() and oracle.eq_xyzt(el, one_el).all()
        r_enc, r_st = c2.msm_ragged(raw, k, off)
        o_enc, o_st = ctx.msm_ragged(raw, k, off)
        w_enc, _, w_st = ragged_fold(oracle, raw, k, off)
        assert (r_enc == o_enc).all() and (r_st == o_st).all() and (r_enc == w_enc).all() and (r_st == w_st).all()
        assert c2.health(0)[0] == 0 and c2.health(1)[0] == 0
    finally:
        c2.close()


def test_cpp_mirror_ragged_sums():
    build_and_run_cpp("ragged_sums", "CPP_RAGGED_SUMS_OK", hip_headers=True)
