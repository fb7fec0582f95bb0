"""The long sums on device buffers and over a pool of points on the MI355X (include/decaf377_amd_long_sums.h):
d377_batch_long_msm[_encoded]_resident against the host form byte for byte, on both routes of the chains and forwarded to the
small sums; d377_batch_long_msm_indexed[_resident] against the oracle's fold and d377_batch_msm_long on the materialised
gather; the host form's refusal of an index outside the pool and the resident form's verdict; slicing over a device listed
twice; the Python routing by device; a captured graph that outlives the scratch it saw; the C++ mirror.

The plain cases are make_case's (tests/_batch_msm_long_cases.py: planted scalars, dead records, invalid Encodings), the indexed
ones tests/_msm_long_indexed_cases.py's: a pool of 23 points with record 5 at Z = 0, indices 0 and 22, repeats, and absent
terms -- a whole group, a whole sum, the last term of a sum."""
import ctypes

import numpy as np
import pytest

from _batch_msm_long_cases import make_case, oracle_fold, plan
from _msm_long_indexed_cases import DEAD_RECORD, POOL, make_indexed, make_pool, materialise
from _sums_support import Side, build_and_run_cpp

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
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
    assert c.health()[0] == 0 and c.health()[2] == 0             # after the file's tests: no lane set claimed, nobody gave up
    c.close()


@pytest.fixture(scope="module")
def side(torch, ctx):
    return Side(torch, ctx)


def _wave_max():
    import torch
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count


# ---- the plain resident forms against the host form --------------------------------------------------------------------------
def _plain(ctx, side, oracle, n, m, seed):
    """Both forms, Elements and Encodings, on make_case's cases: the resident outputs are the host form's bytes."""
    for encoded in (False, True):
        rng = np.random.default_rng(seed + encoded)
        if m > 8:
            pts, k, _ = make_case(oracle, rng, n, m, encoded=encoded)
        else:                                                    # (make_case builds sums of more than 8 terms)
            pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8)), dtype=np.uint64)
            k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
            if encoded:
                pts = oracle.compress(pts)
                pts[4::9, 31] |= 0x40
            else:
                pts.reshape(n * m, 4, 4)[4::9, 2] = 0
        want = ctx.msm_long(pts, k, m, elements=True)
        enc, el = side.empty((n, 32), fill=0xA5), side.empty((n, 16), "u64", fill=0x5A5A)
        if encoded:
            st = side.empty((n * m,), fill=0xEE)
            side.ok("d377_batch_long_msm_encoded_resident", side.dev(pts), side.dev(k), m, n, enc, el, st)
            assert (side.host(st) == want[2]).all(), (n, m)
            assert want[2].any()                                 # an invalid Encoding was there to report
        else:
            side.ok("d377_batch_long_msm_resident", side.dev(pts), side.dev(k), m, n, enc, el)
        assert (side.host(enc) == want[0]).all(), (n, m, encoded)
        assert (side.host(el) == want[1]).all(), (n, m, encoded)
        enc2 = side.empty((n, 32), fill=0xA5)                    # without Element records
        if encoded:
            side.ok("d377_batch_long_msm_encoded_resident", side.dev(pts), side.dev(k), m, n, enc2, None, st)
        else:
            side.ok("d377_batch_long_msm_resident", side.dev(pts), side.dev(k), m, n, enc2, None)
        assert (side.host(enc2) == want[0]).all(), (n, m, encoded)


@pytest.mark.parametrize("n,m", [(3, 17), (2, 129), (1, 4096)])
def test_plain_resident_equals_host_on_the_waves(ctx, side, oracle, n, m):
    assert n * plan(m)[0] <= _wave_max()
    _plain(ctx, side, oracle, n, m, 100 * m + n)


@pytest.mark.parametrize("n,m", [(37, 9), (5, 129)])
def test_plain_resident_equals_host_on_the_lanes(ctx, side, oracle, n, m):
    with ctx.tuning(tiny_max=0):                                 # wave_max = 0: every call takes the lanes, host form and resident alike
        _plain(ctx, side, oracle, n, m, 200 * m + n)


def test_plain_resident_forwards_short_sums(ctx, side, oracle):
    _plain(ctx, side, oracle, 50, 3, 303)


# ---- the indexed forms --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(oracle):
    return make_pool(oracle, np.random.default_rng(23))


def _indexed(ctx, side, oracle, pool, n, m, seed):
    rng = np.random.default_rng(seed)
    idx, k, info = make_indexed(rng, n, m)
    flat = idx.reshape(-1)
    assert 0 in flat and POOL - 1 in flat and (n * m < 5 or DEAD_RECORD in flat)
    assert m < 5 or "repeat" in info                             # an index twice within one sum
    pts = materialise(pool, idx)
    want_enc, want_el, _ = oracle_fold(oracle, pts, k, m)
    # the host form
    enc, el = ctx.msm_long_indexed(pool, idx, k, m, elements=True)
    assert (enc == want_enc).all(), (n, m, np.nonzero((enc != want_enc).any(1))[0][:8])
    assert oracle.eq_xyzt(el, want_el).all(), (n, m)
    assert (oracle.compress(np.ascontiguousarray(el)) == enc).all(), (n, m)          # the Element records have that Encoding
    assert (ctx.msm_long(pts, k, m) == enc).all(), (n, m)                            # d377_batch_msm_long on the materialised array
    assert (ctx.msm_long_indexed(pool, idx, k, m) == enc).all()
    for s in info["identity"]:
        assert not enc[s].any()
    # the resident form, with and without Element records
    r_enc, r_el, ver = side.empty((n, 32), fill=0xA5), side.empty((n, 16), "u64", fill=0x5A5A), side.empty((2,), "u64", fill=7)
    side.ok("d377_batch_long_msm_indexed_resident", side.dev(pool), POOL, side.dev(idx), side.dev(k), m, n, r_enc, r_el, ver)
    assert (side.host(r_enc) == want_enc).all(), (n, m)
    assert (side.host(r_el) == el).all(), (n, m)                 # the same launch on the same inputs: the host form's bytes
    assert side.host(ver).tolist() == [0, NONE]
    r2 = side.empty((n, 32), fill=0xA5)
    side.ok("d377_batch_long_msm_indexed_resident", side.dev(pool), POOL, side.dev(idx), side.dev(k), m, n, r2, None, None)
    assert (side.host(r2) == want_enc).all(), (n, m)
    return idx, k, el


@pytest.mark.parametrize("n,m", [(3, 17), (2, 129), (1, 4096)])
def test_indexed_on_the_waves(ctx, side, oracle, pool, n, m):
    assert n * plan(m)[0] <= _wave_max()
    _indexed(ctx, side, oracle, pool, n, m, 300 * m + n)


def test_indexed_on_the_lanes(ctx, side, oracle, pool):
    n, m = 37, 9
    with ctx.tuning(tiny_max=0):
        idx, k, lane_el = _indexed(ctx, side, oracle, pool, n, m, 409)
    wave_el = ctx.msm_long_indexed(pool, idx, k, m, elements=True)[1]
    assert oracle.eq_xyzt(wave_el, lane_el).all()
    assert (wave_el != lane_el).any()                            # another extended representative: it was two routes that agreed


@pytest.mark.parametrize("m", [1, 5, 8])
def test_indexed_short_sums_write_their_element_records(ctx, side, oracle, pool, m):
    """m <= 8: one chain per sum and no fold level, on the waves and on the lanes."""
    _indexed(ctx, side, oracle, pool, 7, m, 500 + m)
    with ctx.tuning(tiny_max=0):
        _indexed(ctx, side, oracle, pool, 7, m, 600 + m)


def _plant(idx):
    """Index POOL and index -2 planted -> (bad, mended with the two entries absent, the first position)."""
    bad = idx.copy()
    flat = bad.reshape(-1)
    a, b = len(flat) // 3, 2 * len(flat) // 3
    flat[a], flat[b] = POOL, -2
    mended = bad.copy()
    mended.reshape(-1)[[a, b]] = -1
    return bad, mended, a


def test_host_form_refuses_an_index_outside_the_pool(ctx, oracle, pool):
    n, m = 3, 17
    idx, k, _ = make_indexed(np.random.default_rng(7), n, m)
    bad, _, first = _plant(idx)
    lib = ctx._lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for which, value in ((bad, POOL), (np.where(bad == POOL, 0, bad).astype(np.int32), -2)):
        enc, el = np.full((n, 32), 0xA5, np.uint8), np.full((n, 16), 0x5A5A, np.uint64)
        assert lib.d377_batch_long_msm_indexed(ctx._h, p(pool), POOL, p(which), p(k), m, n, p(enc), p(el)) == ERR_ARG
        msg = lib.d377_last_error().decode()
        pos = int(np.nonzero(which.reshape(-1) == value)[0][0])
        assert "point_index[%d] = %d (sum %d, term %d)" % (pos, value, pos // m, pos % m) in msg, msg
        assert (enc == 0xA5).all() and (el == 0x5A5A).all()      # no output byte written
    import decaf377_amd as d
    with pytest.raises(d.NativeError, match=r"point_index\[%d\] = %d " % (first, POOL)):
        ctx.msm_long_indexed(pool, bad, k, m)


@pytest.mark.parametrize("n,m", [(3, 17), (7, 5)])
def test_resident_form_counts_refused_indices_and_walks_them_as_absent(ctx, side, oracle, pool, n, m):
    idx, k, _ = make_indexed(np.random.default_rng(70 + m), n, m)
    bad, mended, first = _plant(idx)
    enc, el, ver = side.empty((n, 32), fill=0xA5), side.empty((n, 16), "u64"), side.empty((2,), "u64", fill=7)
    side.ok("d377_batch_long_msm_indexed_resident", side.dev(pool), POOL, side.dev(bad), side.dev(k), m, n, enc, el, ver)
    assert side.host(ver).tolist() == [2, first]
    want = ctx.msm_long_indexed(pool, mended, k, m, elements=True)
    assert (side.host(enc) == want[0]).all() and (side.host(el) == want[1]).all()
    assert (want[0] == oracle_fold(oracle, materialise(pool, mended), k, m)[0]).all()


def test_refusals_on_a_live_context(ctx, side, pool):
    n, m = 3, 17
    idx, k, _ = make_indexed(np.random.default_rng(9), n, m)
    lib = ctx._lib
    dp, di, dk = side.dev(pool), side.dev(idx), side.dev(k)
    pts = side.dev(materialise(pool, idx))
    enc, el, ver = side.empty((n, 32), fill=0x5A), side.empty((n, 16), "u64", fill=0x5A5A), side.empty((2,), "u64", fill=7)
    off = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    msg = lambda: lib.d377_last_error().decode()
    ix, pl = "d377_batch_long_msm_indexed_resident", "d377_batch_long_msm_resident"
    assert side.call(ix, off(dp, 8), POOL, di, dk, m, n, enc, el, ver) == ERR_ARG and "aligned" in msg()
    assert side.call(ix, dp, POOL, di, off(dk, 8), m, n, enc, el, ver) == ERR_ARG and "aligned" in msg()
    assert side.call(ix, dp, POOL, off(di, 2), dk, m, n, enc, el, ver) == ERR_ARG and "point_index" in msg()
    assert side.call(ix, dp, POOL, di, dk, m, n, enc, el, off(ver, 4)) == ERR_ARG and "verdict" in msg()
    assert side.call(pl, off(pts, 8), dk, m, n, enc, el) == ERR_ARG and "aligned" in msg()
    assert side.call(pl, pts, dk, m, n, off(enc, 8), el) == ERR_ARG and "aligned" in msg()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for bad_dev in (-1, 1):
        args = (ctx._h, bad_dev, ctypes.c_void_p(side.stream.cuda_stream))
        assert lib.d377_batch_long_msm_indexed_resident(*args, p(dp), POOL, p(di), p(dk), m, n, p(enc), p(el), p(ver)) == ERR_ARG and "dev" in msg()
        assert lib.d377_batch_long_msm_resident(*args, p(pts), p(dk), m, n, p(enc), p(el)) == ERR_ARG and "dev" in msg()
    # n == 0 with good arguments: D377_OK, nothing enqueued, no verdict record written
    assert side.call(ix, None, POOL, None, None, m, 0, None, None, ver) == 0
    assert side.call(pl, None, None, m, 0, None, None) == 0
    assert side.call("d377_batch_long_msm_encoded_resident", None, None, m, 0, None, None, None) == 0
    assert (side.host(enc) == 0x5A).all() and (side.host(el) == 0x5A5A).all() and (side.host(ver) == 7).all()


def test_device_listed_twice_slices_the_indexed_sums(oracle, pool):
    import decaf377_amd as d
    n, m = 5, 17
    idx, k, _ = make_indexed(np.random.default_rng(517), n, m)
    c2 = d.Context([0, 0], comb_lazy=True)
    try:
        enc, el = c2.msm_long_indexed(pool, idx, k, m, elements=True)
        want_enc, want_el, _ = oracle_fold(oracle, materialise(pool, idx), k, m)
        assert (enc == want_enc).all()
        assert oracle.eq_xyzt(el, want_el).all()                 # Element records in place
        assert c2.health(0)[0] == 0 and c2.health(1)[0] == 0
    finally:
        c2.close()


# ---- Python routing -------------------------------------------------------------------------------------------------------------
def test_python_routes_by_device(torch, oracle, pool, monkeypatch):
    """A tensor on a device of the context: the resident form, results on that device (check_indices=False shows the route: only
    the resident form has a verdict tensor).  A tensor on a GPU the context does not own -- one GPU stands in for two: the
    context is told that its device has another index -- keeps the host path, results back on the tensor's device."""
    import decaf377_amd as d
    n, m = 3, 17
    idx, k, _ = make_indexed(np.random.default_rng(31), n, m)
    pts = materialise(pool, idx)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
    c = d.Context([0], comb_lazy=True)
    try:
        want = c.msm_long_indexed(pool, idx, k, m, elements=True)
        enc, el, ver = c.msm_long_indexed(T(pool), T(idx), T(k), m, elements=True, check_indices=False)
        assert str(enc.device) == "cuda:0" and ver.cpu().tolist() == [0, -1]
        assert (enc.cpu().numpy() == want[0]).all() and (el.cpu().numpy().view(np.uint64) == want[1]).all()
        assert (c.msm_long_indexed(pool, T(idx), k, m).cpu().numpy() == want[0]).all()      # one own tensor routes the call
        outs = [torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda:0")]
        bad, _, first = _plant(idx)
        with pytest.raises(d.NativeError, match=r"point_index\[%d\]" % first):
            c.msm_long_indexed(T(pool), T(bad), T(k), m, outs=outs)
        torch.cuda.synchronize()
        assert bool((outs[0] == 0x5A).all())                     # refused before any sum was launched
        assert c.msm_long_indexed(T(pool), T(idx), T(k), m, outs=outs) is outs[0] and (outs[0].cpu().numpy() == want[0]).all()
        plain = c.msm_long(T(pts), T(k), m, elements=True)
        assert str(plain[0].device) == "cuda:0"
        host = c.msm_long(pts, k, m, elements=True)
        assert (plain[0].cpu().numpy() == host[0]).all() and (plain[1].cpu().numpy().view(np.uint64) == host[1]).all()
        cpu = c.msm_long_indexed(torch.from_numpy(pool.view(np.int64)), torch.from_numpy(idx), torch.from_numpy(k), m)
        assert cpu.device.type == "cpu" and (cpu.numpy() == want[0]).all()
        monkeypatch.setattr(c, "device_ids", [7])
        got = c.msm_long_indexed(T(pool), T(idx), T(k), m, check_indices=False), c.msm_long(T(pts), T(k), m)
        monkeypatch.undo()
        for g in got:
            assert not isinstance(g, tuple) and str(g.device) == "cuda:0" and (g.cpu().numpy() == want[0]).all()
    finally:
        c.close()


# ---- a captured graph, and scratch that a graph has seen -------------------------------------------------------------------------
def test_graph_replays_and_outlives_the_scratch_it_saw(torch, oracle, pool):
    import decaf377_amd as d
    rng = np.random.default_rng(99)
    n, m = 3, 17
    pts, pk, _ = make_case(oracle, rng, n, m)
    idx, ik, _ = make_indexed(rng, n, m)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no scratch has grown yet
    try:
        s = Side(torch, c)
        with c.tuning(tiny_max=0):                               # the lane route: the one that uses the table scratch
            dpts, dpk, dpool, didx, dik = s.dev(pts), s.dev(pk), s.dev(pool), s.dev(idx), s.dev(ik)
            e_pl, e_ix, ver = s.empty((n, 32)), s.empty((n, 32)), s.empty((2,), "u64", fill=7)

            def enqueue(stream):
                s.ok("d377_batch_long_msm_resident", dpts, dpk, m, n, e_pl, None, stream=stream)
                s.ok("d377_batch_long_msm_indexed_resident", dpool, POOL, didx, dik, m, n, e_ix, None, ver, stream=stream)

            def expect(what):
                torch.cuda.synchronize()
                hidx = didx.cpu().numpy()
                assert (e_pl.cpu().numpy() == c.msm_long(pts, dpk.cpu().numpy(), m)).all(), what
                assert (e_ix.cpu().numpy() == c.msm_long_indexed(pool, hidx, dik.cpu().numpy(), m)).all(), what
                assert ver.cpu().tolist() == [0, -1], what

            enqueue(None)                                        # one eager call of each shape: the scratch areas grow here
            expect("eager")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                            # one stream, a linear graph
                enqueue(torch.cuda.current_stream().cuda_stream)

            def overwrite():
                for buf in (dpk, dik):                           # new scalars and new indices, written in place
                    buf.copy_(torch.from_numpy(rng.integers(0, 256, tuple(buf.shape), dtype=np.uint8)))
                didx.copy_(torch.from_numpy(rng.integers(-1, POOL, (n, m)).astype(np.int32)))
                e_pl.zero_(); e_ix.zero_(); ver.fill_(7)
                torch.cuda.synchronize()

            for rep in range(2):
                overwrite()
                g.replay()
                expect("replay %d" % rep)

            # outgrow both areas the graph has seen: the table scratch (8 tables per lane instead of 6) and the partial sums
            p8 = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (5 * 8, 32), dtype=np.uint8)), dtype=np.uint64)
            k8 = rng.integers(0, 256, (5 * 8, 32), dtype=np.uint8)
            assert plan(m)[1] < 8
            assert (c.msm_small(p8, k8, 8) == oracle_fold(oracle, p8, k8, 8)[0]).all()
            bn, bm = 37, 129                                     # 37 x 17 partial sums where the graph's calls had 3 x 3
            assert bn * plan(bm)[0] > 2 * n * plan(m)[0]
            bpts, bk, _ = make_case(oracle, rng, bn, bm)
            assert (c.msm_long(bpts, bk, bm) == oracle_fold(oracle, bpts, bk, bm)[0]).all()
            overwrite()
            g.replay()                                           # the old graph, into the areas it was captured with
            expect("replay after the scratch was outgrown")
        claimed, _, gave_up = c.health()
        assert (claimed, gave_up) == (0, 0)
    finally:
        c.close()


def test_cpp_mirror_msm_long_indexed():
    build_and_run_cpp("msm_long_indexed", "CPP_MSM_LONG_INDEXED_OK", hip_headers=True)
