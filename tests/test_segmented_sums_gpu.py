"""Many sums of any length each by Straus chains on the MI355X (d377_batch_segmented_msm, include/decaf377_amd_segmented_sums.h):
the host forms against the oracle's fold per sum, Elements and Encodings with their statuses, on the cases of
tests/_segmented_sums_cases.py -- every case on the wave route (the module's context) and on the lane route (a second context
with tiny_max = 0); against d377_batch_ragged_msm on the same arrays and, with equal lengths, against d377_batch_msm_long byte for
byte; the resident forms against the host forms; refusals on a live context; a capture refused and a graph that outlives the
scratch it saw; a device listed twice; the Python routing and msm_by_offsets on both routes; the C++ mirror.  Every case is a
few thousand terms at the most."""
import ctypes

import numpy as np
import pytest

import _segmented_sums_cases as sc
from _ragged_sums_cases import device_cuts, make_case, offsets_of, ragged_fold
from _sums_support import Side, build_and_run_cpp

pytestmark = pytest.mark.gpu

ERR_ARG = -2
ROUTES = ("wave", "lane")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctxs():
    """route -> context: the library's routing (a wave per chain slot at these sizes), and tiny_max = 0 (a lane per slot)."""
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
def sides(torch, ctxs):
    return {r: Side(torch, c) for r, c in ctxs.items()}


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> encoded -> (points, scalars, offsets, dead, the oracle's (enc, el, status)), made once and left unchanged."""
    out = {}
    for name, lengths in sc.CASES.items():
        out[name] = {}
        for encoded in (False, True):
            pts, k, off, dead = sc.build(oracle, np.random.default_rng(len(lengths) * 1000 + encoded), lengths, encoded=encoded)
            out[name][encoded] = (pts, k, off, dead, ragged_fold(oracle, pts, k, off))
    return out


def _first(res):
    return res[0] if isinstance(res, tuple) else res


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_host_forms_match_oracle_fold(ctxs, oracle, cases, name, route):
    c = ctxs[route]
    lengths = sc.CASES[name]
    for encoded in (False, True):
        pts, k, off, dead, (want_enc, want_el, want_st) = cases[name][encoded]
        got = c.msm_segmented(pts, k, off, elements=True)
        assert (got[0] == want_enc).all(), (name, encoded, np.nonzero((got[0] != want_enc).any(1))[0][:8])
        assert oracle.eq_xyzt(got[1], want_el).all(), (name, encoded)
        assert (oracle.compress(np.ascontiguousarray(got[1])) == got[0]).all(), (name, encoded)
        if encoded:
            assert (got[2] == want_st).all() and ((got[2] != 0) == dead).all(), name
        plain = c.msm_segmented(pts, k, off)                     # without Element records
        assert (_first(plain) == got[0]).all(), name
        for s, L in enumerate(lengths):
            if L == 0:
                assert not got[0][s].any() and oracle.is_identity(got[1][s:s + 1]).all(), (name, s)
        ragged = c.msm_ragged(pts, k, off, elements=True)        # the bucket pipeline on the same arrays
        assert (ragged[0] == got[0]).all() and oracle.eq_xyzt(ragged[1], got[1]).all(), (name, encoded)
        if encoded:
            assert (ragged[2] == got[2]).all(), name
    want, plan = sc.plan(off), c.msm_segmented_plan(off)
    assert (plan["chain_slots"], plan["chains"], plan["fold_levels"], plan["max_slots_per_chain"]) == \
        (want["chain_slots"], want["chains"], want["levels"], want["bmax"]), name
    assert plan["advised_route"] == ("chains", "buckets")[want["route"]] and (want["route"] == 1) == (name in ("two_levels", "past_long_limit"))
    tables = plan["scratch_bytes"] - want["records"] * 128
    assert tables == 0 if route == "wave" or not want["terms"] else tables > 0, (name, route, plan)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(sc.EQUAL))
def test_equal_lengths_give_the_bytes_of_the_long_sums(ctxs, oracle, name, route):
    c = ctxs[route]
    lengths = sc.EQUAL[name]
    m = lengths[0]
    for encoded in (False, True):
        pts, k, off, _ = sc.build(oracle, np.random.default_rng(m + encoded), lengths, encoded=encoded)
        want = c.msm_long(pts, k, m, elements=True)
        got = c.msm_segmented(pts, k, off, elements=True)
        assert len(got) == len(want)
        for g, w in zip(got[::2], want[::2]):                    # Encodings and statuses: byte for byte
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (name, encoded)
        assert oracle.eq_xyzt(got[1], want[1]).all(), (name, encoded)
        assert (got[0] == ragged_fold(oracle, pts, k, off)[0]).all()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_resident_forms_equal_the_host_forms(ctxs, sides, cases, oracle, name, route):
    c, side = ctxs[route], sides[route]
    for encoded in (False, True):
        pts, k, off, _, _ = cases[name][encoded]
        n, terms = len(off) - 1, int(off[-1])
        want = c.msm_segmented(pts, k, off, elements=True)
        enc, el = side.empty((n + 1, 32), fill=0xA5), side.empty((n + 1, 16), "u64", fill=0x5A5A)    # one row more: nothing else is written
        doff, hoff = side.dev(off), off.ctypes.data_as(ctypes.c_void_p)
        dp, dk = (side.dev(pts), side.dev(k)) if terms else (None, None)
        if encoded:
            st = side.empty((terms + 1,), fill=0xEE)
            side.ok("d377_batch_segmented_msm_encoded_resident", dp, dk, hoff, doff, n, enc, el, st)
            assert (side.host(st)[:terms] == want[2]).all() and side.host(st)[terms] == 0xEE, name
        else:
            side.ok("d377_batch_segmented_msm_resident", dp, dk, hoff, doff, n, enc, el)
        assert (side.host(enc)[:n] == want[0]).all() and (side.host(enc)[n] == 0xA5).all(), (name, encoded)
        assert oracle.eq_xyzt(side.host(el)[:n], want[1]).all() and (side.host(el)[n] == 0x5A5A).all(), (name, encoded)
        enc2 = side.empty((n + 1, 32), fill=0xA5)                # without Element records
        if encoded:
            side.ok("d377_batch_segmented_msm_encoded_resident", dp, dk, hoff, doff, n, enc2, None, st)
        else:
            side.ok("d377_batch_segmented_msm_resident", dp, dk, hoff, doff, n, enc2, None)
        assert (side.host(enc2)[:n] == want[0]).all() and (side.host(enc2)[n] == 0xA5).all(), (name, encoded)


def test_refusals_on_a_live_context(torch, ctx, sides, oracle):
    side = sides["wave"]
    lengths = (3, 0, 17, 5)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(17), lengths, 6)
    n = len(lengths)
    lib = ctx._lib
    dp, dk, doff = side.dev(pts), side.dev(k), side.dev(off)
    hoff = off.ctypes.data_as(ctypes.c_void_p)
    enc, el = side.empty((n, 32), fill=0x5A), side.empty((n, 16), "u64", fill=0x5A5A)
    shift = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)     # noqa: E731
    msg = lambda: lib.d377_last_error().decode()                  # noqa: E731
    name = "d377_batch_segmented_msm_resident"
    assert side.call(name, shift(dp, 8), dk, hoff, doff, n, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, shift(dk, 8), hoff, doff, n, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, doff, n, shift(enc, 8), el) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, doff, n, enc, shift(el, 8)) == ERR_ARG and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, shift(doff, 4), n, enc, el) == ERR_ARG and "offsets_dev" in msg() and "aligned" in msg()
    assert side.call(name, dp, dk, hoff, None, n, enc, el) == ERR_ARG and "offsets_dev" in msg()
    bad = np.array([0, 3, 2, 20, 25], np.uint64)
    assert side.call(name, dp, dk, bad.ctypes.data_as(ctypes.c_void_p), doff, n, enc, el) == ERR_ARG and "sum 1" in msg() and "offsets" in msg()
    long = np.array([0, 3, 3, 4 + (1 << 20), 5 + (1 << 20)], np.uint64)
    assert side.call(name, dp, dk, long.ctypes.data_as(ctypes.c_void_p), doff, n, enc, el) == ERR_ARG and "sum 2" in msg() and "offsets" in msg()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    for bad_dev in (-1, 1):
        args = (ctx._h, bad_dev, ctypes.c_void_p(side.stream.cuda_stream))
        assert lib.d377_batch_segmented_msm_resident(*args, p(dp), p(dk), hoff, p(doff), n, p(enc), p(el)) == ERR_ARG and "dev" in msg()
        assert lib.d377_segmented_msm_plan(ctx._h, bad_dev, hoff, n, None, None, None, None, None, None) == ERR_ARG and "dev" in msg()
    assert side.call(name, None, None, None, None, 0, None, None) == 0                       # n == 0 with good arguments
    assert side.call("d377_batch_segmented_msm_encoded_resident", None, None, None, None, 0, None, None, None) == 0
    assert (side.host(enc) == 0x5A).all() and (side.host(el) == 0x5A5A).all()
    assert ctx.msm_segmented_plan([0]) == {"chain_slots": 0, "chains": 0, "fold_levels": 0, "max_slots_per_chain": 0, "scratch_bytes": 0,
                                           "advised_route": "chains"}
    assert ctx.msm_segmented_plan([0, 0, 0]) == {"chain_slots": 2, "chains": 0, "fold_levels": 0, "max_slots_per_chain": 0,
                                                 "scratch_bytes": 4 * 128, "advised_route": "chains"}
    assert ctx.msm_segmented_plan([0, 1024, 2048])["advised_route"] == "buckets"
    # sums without a term need no term buffers
    none = np.zeros(3, np.uint64)
    assert side.call(name, None, None, none.ctypes.data_as(ctypes.c_void_p), side.dev(none), 2, enc, None) == 0
    assert (side.host(enc)[:2] == 0).all() and (side.host(enc)[2:] == 0x5A).all()


def test_a_capture_of_a_shape_never_run_eagerly_is_refused(torch, oracle):
    import decaf377_amd as d
    lengths = (3, 0, 17, 5)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(18), lengths, 6)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no scratch has grown yet
    try:
        s = Side(torch, c)
        dp, dk, doff, out = s.dev(pts), s.dev(k), s.dev(off), s.empty((len(lengths), 32), fill=0x5A)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rc = s.call("d377_batch_segmented_msm_resident", dp, dk, off.ctypes.data_as(ctypes.c_void_p), doff, len(lengths), out, None,
                        stream=torch.cuda.current_stream().cuda_stream)
            text = c._lib.d377_last_error().decode()
        assert rc == ERR_ARG and "capture" in text
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0x5A).all()
    finally:
        c.close()


@pytest.mark.parametrize("route", ROUTES)
def test_graph_replays_and_outlives_the_scratch_it_saw(torch, oracle, route):
    import decaf377_amd as d
    rng = np.random.default_rng(99)
    lengths = (3, 0, 17, 5, 140)
    n = len(lengths)
    pts, k, off, _ = make_case(oracle, rng, lengths, 6)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no scratch has grown yet
    try:
        if route == "lane":
            c.set_tuning("tiny_max", 0)
        s = Side(torch, c)
        dpts, dk, doff, out = s.dev(pts), s.dev(k), s.dev(off), s.empty((n, 32))
        hoff = off.ctypes.data_as(ctypes.c_void_p)

        def enqueue(stream):
            s.ok("d377_batch_segmented_msm_resident", dpts, dk, hoff, doff, n, out, None, stream=stream)

        def expect(what):
            torch.cuda.synchronize()
            hk = dk.cpu().numpy()
            assert (out.cpu().numpy() == ragged_fold(oracle, pts, hk, off)[0]).all(), what

        enqueue(None)                                            # one eager call of the shape: the scratch grows here
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
        small = c.msm_segmented_plan(off)["scratch_bytes"]
        big = (600, 1, 0, 900, 1500)                             # a larger eager call that outgrows the partials area the graph saw
        bp, bk, boff, _ = make_case(oracle, rng, big, 6)
        assert sc.plan(boff)["records"] > 2 * (sc.plan(off)["records"] * 5 // 4 + 32) and c.msm_segmented_plan(boff)["scratch_bytes"] > small
        assert (_first(c.msm_segmented(bp, bk, boff)) == ragged_fold(oracle, bp, bk, boff)[0]).all()
        overwrite()
        g.replay()                                               # the old graph, into the area it was captured with
        expect("replay after the scratch was outgrown")
        claimed, _, gave_up = c.health()
        assert (claimed, gave_up) == (0, 0)
    finally:
        c.close()


def test_device_listed_twice_gives_the_single_device_bytes(ctx, oracle):
    import decaf377_amd as d
    lengths = (200, 1, 0, 33, 7, 0, 60, 0)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(533), lengths, 7)
    raw, _, _, _ = make_case(oracle, np.random.default_rng(533), lengths, 7, encoded=True)
    assert device_cuts(off, 2) == [0, 1, 8]                      # by terms: the long sum alone on the first device
    c2 = d.Context([0, 0], comb_lazy=True)
    try:
        enc, el = c2.msm_segmented(pts, k, off, elements=True)
        one_enc, one_el = ctx.msm_segmented(pts, k, off, elements=True)
        want_enc, want_el, _ = ragged_fold(oracle, pts, k, off)
        assert (enc == one_enc).all() and (enc == want_enc).all() and oracle.eq_xyzt(el, one_el).all()
        r_enc, r_st = c2.msm_segmented(raw, k, off)
        o_enc, o_st = ctx.msm_segmented(raw, k, off)
        w_enc, _, w_st = ragged_fold(oracle, raw, k, off)
        assert (r_enc == o_enc).all() and (r_st == o_st).all() and (r_enc == w_enc).all() and (r_st == w_st).all()
        off2 = offsets_of((9, 17, 40, 3, 0, 21))                 # the second device's slice begins at an offset that is no multiple of 8
        assert device_cuts(off2, 2) == [0, 2, 6] and int(off2[2]) % 8
        p2, k2, _, _ = make_case(oracle, np.random.default_rng(534), (9, 17, 40, 3, 0, 21), 7)
        assert (_first(c2.msm_segmented(p2, k2, off2)) == ragged_fold(oracle, p2, k2, off2)[0]).all()
        assert c2.health(0)[0] == 0 and c2.health(1)[0] == 0
    finally:
        c2.close()


def test_python_routes_by_device_and_by_offsets(torch, oracle, monkeypatch):
    import decaf377_amd as d
    lengths = (3, 0, 17, 5)
    n = len(lengths)
    pts, k, off, _ = make_case(oracle, np.random.default_rng(31), lengths, 6)
    raw, _, _, _ = make_case(oracle, np.random.default_rng(31), lengths, 6, encoded=True)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")   # noqa: E731
    c = d.Context([0], comb_lazy=True)
    try:
        want = c.msm_segmented(pts, k, off, elements=True)
        assert (want[0] == ragged_fold(oracle, pts, k, off)[0]).all()
        assert (want[0] == _first(c.msm_segmented(pts, k, [int(v) for v in off]))).all()       # offsets as a list
        enc, el = c.msm_segmented(T(pts), T(k), off, elements=True)
        assert str(enc.device) == "cuda:0" and str(el.device) == "cuda:0"
        assert (enc.cpu().numpy() == want[0]).all() and oracle.eq_xyzt(el.cpu().numpy().view(np.uint64), want[1]).all()
        outs = [torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda:0")]
        got = c.msm_segmented(T(pts), T(k), off.astype(np.int64), outs=outs, offsets_dev=T(off))
        assert got is outs[0] and (outs[0].cpu().numpy() == want[0]).all()
        with pytest.raises(ValueError, match="offsets_dev"):
            c.msm_segmented(T(pts), T(k), off, offsets_dev=T(off)[:n])
        w_enc, w_st = c.msm_segmented(raw, k, off)
        r_enc, r_st = c.msm_segmented(T(raw), T(k), off)
        assert (r_enc.cpu().numpy() == w_enc).all() and (r_st.cpu().numpy() == w_st).all() and w_st.any() and len(w_st) == int(off[-1])
        with pytest.raises(d.NativeError, match="no CPU path"):
            c.msm_segmented(torch.from_numpy(pts.view(np.int64)), torch.from_numpy(k), off)
        monkeypatch.setattr(c, "device_ids", [7])                # a GPU the context does not own: staged through the host
        got = c.msm_segmented(T(pts), T(k), off)
        monkeypatch.undo()
        assert str(got.device) == "cuda:0" and (got.cpu().numpy() == want[0]).all()

        # msm_by_offsets: the whole call to one of the two, by name or by the plan's advice
        taken = []
        for meth in ("msm_segmented", "msm_ragged"):
            real = getattr(c, meth)
            monkeypatch.setattr(c, meth, lambda *a, _m=meth, _r=real, **kw: (taken.append(_m), _r(*a, **kw))[1])
        for route, via in (("chains", "msm_segmented"), ("buckets", "msm_ragged"), ("auto", "msm_segmented")):
            for p, s in ((pts, k), (T(pts), T(k))):
                del taken[:]
                got = c.msm_by_offsets(p, s, off, elements=True, route=route)
                assert taken == [via], (route, taken)
                host = [g.cpu().numpy() if hasattr(g, "cpu") else g for g in got]
                assert (host[0] == want[0]).all() and oracle.eq_xyzt(host[1].view(np.uint64), want[1]).all(), route
        long_off = offsets_of((1100, 1000))                      # a mean of 1050: the plan advises the buckets
        lp, lk, _, _ = make_case(oracle, np.random.default_rng(32), (1100, 1000), 6)
        del taken[:]
        auto = c.msm_by_offsets(lp, lk, long_off)
        assert taken == ["msm_ragged"] and c.msm_segmented_plan(long_off)["advised_route"] == "buckets"
        assert (_first(auto) == _first(c.msm_by_offsets(lp, lk, long_off, route="chains"))).all() and taken == ["msm_ragged", "msm_segmented"]
        assert (_first(auto) == ragged_fold(oracle, lp, lk, long_off)[0]).all()
    finally:
        c.close()


def test_cpp_mirror_segmented_sums():
    build_and_run_cpp("segmented_sums", "CPP_SEGMENTED_SUMS_OK", hip_headers=True)
