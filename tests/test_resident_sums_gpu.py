"""The resident forms of the sums over registered bases on the MI355X: d377_batch_fixed_msm_resident,
d377_batch_fixed_long_msm_resident, d377_batch_fixed_msm_indexed_resident, d377_batch_msm_mixed[_encoded]_resident and
d377_check_base_index_resident, called through the C ABI on torch tensors, each on a side stream.

Every resident call is compared with its host form on the same inputs -- equal Encodings and status bytes, Elements equal
under the oracle's eq_xyzt and compressing to their Encodings -- and one shape per call with the oracle's fold directly.  The
cases and the folds are those of tests/_batch_msm_long_cases.py, tests/_fixed_msm_long_cases.py and tests/_sums_support.py.
n = 257 is two workgroups of 256 lanes with one live lane in the second.

The index verdict: one record per call, (refused indices, first position or UINT64_MAX); a refused index contributes nothing.
The graph test captures the indexed, the mixed and the segmented dense call, replays with the scalars overwritten in place, outgrows the
table scratch and the partial sums' area with eager calls, and replays the old graph once more: an area that a graph has seen
is retired, not freed."""
import ctypes

import numpy as np
import pytest

import _fixed_msm_long_cases as fl
from _batch_msm_long_cases import make_case, oracle_fold, plan
from _sums_support import Fold, Side, build_and_run_cpp, join as _join, mixed_case as _case, var_terms as _var_terms

pytestmark = pytest.mark.gpu

N = 257
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
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
    c.close()


@pytest.fixture(scope="module")
def side(torch, ctx):
    return Side(torch, ctx)


def _same(oracle, what, enc, el, want_enc, want_el):
    assert (enc == want_enc).all(), (what, np.nonzero((enc != want_enc).any(1))[0][:8])
    assert oracle.eq_xyzt(el, np.ascontiguousarray(want_el)).all(), what
    assert (oracle.compress(np.ascontiguousarray(el)) == enc).all(), what


# ---- the dense sums over registered bases ---------------------------------------------------------------------------------------
def _dense_resident(side, name, fb, k, n):
    enc, el = side.empty((n, 32)), side.empty((n, 16), "u64")
    side.ok(name, fb._h, side.dev(k), n, enc, el)
    return side.host(enc), side.host(el)


def test_dense_three_bases_two_workgroups(ctx, side, oracle):
    m, n = 3, N
    rng = np.random.default_rng(3)
    bases = fl.make_bases(oracle, rng, m, m)
    k = fl.make_scalars(rng, n, m, 1, m)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        want = fb.msm(k, elements=True)
        enc, el = _dense_resident(side, "d377_batch_fixed_msm_resident", fb, k, n)
    _same(oracle, "host", enc, el, want[0], want[1])
    o_enc, o_el = fl.oracle_fold(oracle, bases, k, n, m)
    _same(oracle, "oracle", enc, el, o_enc, o_el)


def test_dense_one_base_one_sum(ctx, side, oracle):
    rng = np.random.default_rng(11)
    bases = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8)), dtype=np.uint64)
    k = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        want = fb.msm(k, elements=True)
        enc, el = _dense_resident(side, "d377_batch_fixed_msm_resident", fb, k, 1)
    _same(oracle, "host", enc, el, want[0], want[1])


def test_dense_long_handle_is_cut_into_segments(ctx, side, oracle):
    m, n = 65, 3
    rng = np.random.default_rng(65)
    with ctx.fixed_bases_long(fl.make_bases(oracle, rng, m, 1), comb_bits=8) as probe:
        g, b = probe.long_plan(n)
    assert g > 1                                                 # segments > 1: the partial sums, the fold, the chunked compressor
    bases = fl.make_bases(oracle, rng, m, b)
    k = fl.make_scalars(rng, n, m, g, b)
    o_enc, o_el = fl.oracle_fold(oracle, bases, k, n, m)
    with ctx.fixed_bases_long(bases, comb_bits=8) as fb:
        assert fb.long_plan(n) == (g, b)
        want = fb.msm_long(k, elements=True)
        for name in ("d377_batch_fixed_long_msm_resident", "d377_batch_fixed_msm_resident"):   # more than 64 bases: the same call
            enc, el = _dense_resident(side, name, fb, k, n)
            _same(oracle, name, enc, el, want[0], want[1])
            _same(oracle, name + " / oracle", enc, el, o_enc, o_el)


def test_dense_short_handle_through_the_long_call(ctx, side, oracle):
    m, n = 64, 5
    rng = np.random.default_rng(64)
    bases = fl.make_bases(oracle, rng, m, 8)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        g, b = fb.long_plan(n)
        k = fl.make_scalars(rng, n, m, g, b)
        want = fb.msm_long(k, elements=True)
        enc, el = _dense_resident(side, "d377_batch_fixed_long_msm_resident", fb, k, n)
        dense = fb.msm(k)
    _same(oracle, "host", enc, el, want[0], want[1])
    assert (enc == dense).all()


# ---- the indexed sums ----------------------------------------------------------------------------------------------------------
def _indexed_case(oracle, m=64, t=2, n=N):
    bases, idx, fk, _, _ = _case(oracle, 1, t, m, n)
    idx[3] = 0                                                   # base 0 twice in one sum; _case has m - 1, -1 and a repeat of base 1
    assert (idx == -1).any() and (idx == 0).any() and (idx == m - 1).any() and idx[2, 0] == idx[2, 1]
    return bases, np.ascontiguousarray(idx), fk


def _indexed_oracle(oracle, bases, idx, fk):
    """The oracle's indexed sums by scalar multiplications and additions: term (i, j) is fk[i t + j] * B_{idx[i, j]}, absent = 0 * B_0."""
    n, t = idx.shape
    kk = fk.copy()
    kk[(idx < 0).reshape(-1)] = 0
    terms = _var_terms(oracle, np.ascontiguousarray(bases[np.maximum(idx, 0).reshape(-1)]), kk, n, t)
    return _join(oracle, np.tile(oracle.identity_xyzt(), (n, 1)), terms)


def _indexed_resident(side, fb, idx, fk, verdict=True):
    n, t = idx.shape
    enc, el = side.empty((n, 32)), side.empty((n, 16), "u64")
    ver = side.empty((2,), "u64", fill=7) if verdict else None
    side.ok("d377_batch_fixed_msm_indexed_resident", fb._h, side.dev(idx), side.dev(fk), t, n, enc, el, ver)
    return side.host(enc), side.host(el), (tuple(int(x) for x in side.host(ver)) if verdict else None)


def test_indexed_64_bases(ctx, side, oracle):
    bases, idx, fk = _indexed_case(oracle)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        want = fb.msm_indexed(idx, fk, elements=True)
        enc, el, ver = _indexed_resident(side, fb, idx, fk)
        enc2, el2, _ = _indexed_resident(side, fb, idx, fk, verdict=False)   # verdict = NULL runs
    _same(oracle, "host", enc, el, want[0], want[1])
    assert ver == (0, NONE)
    assert (enc2 == enc).all() and (el2 == el).all()
    o_enc, o_el = _indexed_oracle(oracle, bases, idx, fk)
    _same(oracle, "oracle", enc, el, o_enc, o_el)


# ---- the mixed sums ------------------------------------------------------------------------------------------------------------
def _mixed_resident(side, fb, idx, fk, pts, vk, verdict=True):
    n, t = idx.shape
    v = pts.shape[0] // n
    enc, el = side.empty((n, 32)), side.empty((n, 16), "u64")
    ver = side.empty((2,), "u64", fill=7) if verdict else None
    if pts.shape[1] == 32:
        st = side.empty((n * v,), fill=9)
        side.ok("d377_batch_msm_mixed_encoded_resident", fb._h, side.dev(idx), side.dev(fk), t, side.dev(pts), side.dev(vk), v, n, enc, el, st, ver)
        st = side.host(st)
    else:
        st = None
        side.ok("d377_batch_msm_mixed_resident", fb._h, side.dev(idx), side.dev(fk), t, side.dev(pts), side.dev(vk), v, n, enc, el, ver)
    return side.host(enc), side.host(el), st, (tuple(int(x) for x in side.host(ver)) if verdict else None)


@pytest.fixture(scope="module")
def mixed325(oracle):
    """(v, t, bases) = (3, 2, 5) at n = 257 with the oracle's fixed sums and variable terms, made once."""
    v, t, m = 3, 2, 5
    bases, idx, fk, pts, vk = _case(oracle, v, t, m, N)
    return bases, idx, fk, pts, vk, Fold(oracle, bases).records(idx, fk), _var_terms(oracle, pts, vk, N, v)


def test_mixed_signature_shape(ctx, side, oracle):
    bases, idx, fk, pts, vk = _case(oracle, 1, 1, 1, N)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        want = fb.msm_mixed(idx, fk, pts, vk, elements=True)
        enc, el, _, ver = _mixed_resident(side, fb, idx, fk, pts, vk)
    _same(oracle, "host", enc, el, want[0], want[1])
    assert ver == (0, NONE)


def test_mixed_elements(ctx, side, oracle, mixed325):
    bases, idx, fk, pts, vk, fixed, terms = mixed325
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        want = fb.msm_mixed(idx, fk, pts, vk, elements=True)
        enc, el, _, ver = _mixed_resident(side, fb, idx, fk, pts, vk)
        enc2, el2, _, _ = _mixed_resident(side, fb, idx, fk, pts, vk, verdict=False)
    _same(oracle, "host", enc, el, want[0], want[1])
    assert ver == (0, NONE) and (enc2 == enc).all() and (el2 == el).all()
    o_enc, o_el = _join(oracle, fixed, terms)
    _same(oracle, "oracle", enc, el, o_enc, o_el)


def test_mixed_encodings_every_fifth_invalid(ctx, side, oracle, mixed325):
    bases, idx, fk, pts, vk, fixed, terms = mixed325
    v = 3
    good = pts.copy()
    good[~good[:, 8:12].any(1)] = oracle.identity_xyzt()
    encs = oracle.compress(good)
    bad = np.zeros(N * v, bool)
    bad[::5] = True
    encs[bad] = 0xFF                                             # above q: no canonical Encoding
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        want = fb.msm_mixed(idx, fk, encs, vk, elements=True)
        enc, el, st, ver = _mixed_resident(side, fb, idx, fk, encs, vk)
    _same(oracle, "host", enc, el, want[0], want[1])
    assert (st == want[2]).all() and (st == bad.astype(np.uint8)).all() and ver == (0, NONE)
    o_enc, o_el = _join(oracle, fixed, terms, ~bad.reshape(N, v))
    _same(oracle, "oracle", enc, el, o_enc, o_el)


# ---- the index verdict ---------------------------------------------------------------------------------------------------------
PLANTED = {(20, 1): None, (100, 0): -2, (255, 1): INT_MIN, (256, 0): INT_MAX}   # (sum, term) -> value; None: m, the first past the end


def _plant(idx, m):
    bad = idx.copy()
    for (i, j), val in PLANTED.items():
        bad[i, j] = m if val is None else val
    mended = bad.copy()
    for (i, j) in PLANTED:
        mended[i, j] = -1
    hit = np.zeros(idx.shape[0], bool)
    hit[[i for i, _ in PLANTED]] = True
    first = min(i * idx.shape[1] + j for i, j in PLANTED)
    return np.ascontiguousarray(bad), np.ascontiguousarray(mended), hit, first


def test_verdict_of_the_indexed_sums(ctx, side, oracle):
    import decaf377_amd as d
    bases, idx, fk = _indexed_case(oracle)
    bad, mended, hit, first = _plant(idx, 64)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        clean = fb.msm_indexed(idx, fk)
        absent = fb.msm_indexed(mended, fk)
        with pytest.raises(d.NativeError):
            fb.msm_indexed(bad, fk)                              # the host form refuses the whole call
        enc, el, ver = _indexed_resident(side, fb, bad, fk)
        # the verdict alone (the call takes no output but the record): the same record.  (The inputs stay referenced until the side stream has
        # been synchronised: a tensor dropped earlier goes back to an allocator that knows nothing of that stream.)
        dbad, didx = side.dev(bad), side.dev(idx)
        ver2, ver3, ver4 = (side.empty((2,), "u64", fill=7) for _ in range(3))
        side.ok("d377_check_base_index_resident", fb._h, dbad, bad.size, ver2)
        side.ok("d377_check_base_index_resident", fb._h, didx, idx.size, ver3)
        side.ok("d377_check_base_index_resident", fb._h, didx, 0, ver4)                # no index: (0, none)
    assert ver == (4, first)
    assert (enc[~hit] == clean[~hit]).all()                      # sums without a planted index: the host call's
    assert (enc == absent).all()                                 # sums with one: the host call with those terms absent
    assert (oracle.compress(np.ascontiguousarray(el)) == enc).all()
    assert tuple(int(x) for x in side.host(ver2)) == (4, first)
    assert tuple(int(x) for x in side.host(ver3)) == (0, NONE)
    assert tuple(int(x) for x in side.host(ver4)) == (0, NONE)


def test_verdict_of_the_mixed_sums(ctx, side, oracle, mixed325):
    bases, idx, fk, pts, vk, _, _ = mixed325
    bad, mended, hit, first = _plant(idx, 5)
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        clean = fb.msm_mixed(idx, fk, pts, vk)
        absent = fb.msm_mixed(mended, fk, pts, vk)
        enc, el, _, ver = _mixed_resident(side, fb, bad, fk, pts, vk)
    assert ver == (4, first)
    assert (enc[~hit] == clean[~hit]).all() and (enc == absent).all()
    assert (oracle.compress(np.ascontiguousarray(el)) == enc).all()


# ---- Python: resident tensors, the index policy ----------------------------------------------------------------------------------
def test_python_checks_the_indices_before_any_launch(ctx, torch, oracle, mixed325):
    import decaf377_amd as d
    bases, idx, fk, pts, vk, _, _ = mixed325
    bad, mended, hit, first = _plant(idx, 5)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        for call_host, call_dev in ((lambda: fb.msm_indexed(bad, fk), lambda: fb.msm_indexed(T(bad), T(fk))),
                                    (lambda: fb.msm_mixed(bad, fk, pts, vk), lambda: fb.msm_mixed(T(bad), T(fk), T(pts), T(vk)))):
            with pytest.raises(d.NativeError) as host:
                call_host()
            with pytest.raises(d.NativeError) as dev:
                call_dev()
            assert str(dev.value) == str(host.value) and "base_index[%d]" % first in str(dev.value)
        with pytest.raises(ValueError):
            fb.msm_indexed(T(bad.astype(np.int64) + (1 << 40)), T(fk))                  # an int64 index outside 32 bits: as today
        # check_indices=False: nothing is read, the verdict tensor is appended, a refused index contributes nothing
        enc, ver = fb.msm_indexed(T(bad), T(fk), check_indices=False)
        assert enc.device.type == "cuda" and ver.dtype == torch.int64
        assert ver.cpu().tolist() == [4, first]
        assert (enc.cpu().numpy() == fb.msm_indexed(mended, fk)).all()
        enc, el, ver = fb.msm_mixed(T(idx), T(fk), T(pts), T(vk), elements=True, check_indices=False)
        assert ver.cpu().tolist() == [0, -1]                     # UINT64_MAX as int64
        want = fb.msm_mixed(idx, fk, pts, vk, elements=True)
        assert (enc.cpu().numpy() == want[0]).all() and (el.cpu().numpy().view(np.uint64) == want[1]).all()
        # numpy arrays and CPU tensors keep the host path
        cpu = fb.msm_indexed(torch.from_numpy(idx), torch.from_numpy(fk))
        assert cpu.device.type == "cpu" and (cpu.numpy() == fb.msm_indexed(idx, fk)).all()


def test_a_refused_call_leaves_a_prefilled_output_untouched(ctx, torch, oracle, mixed325):
    """check_indices=True refuses before any sum is launched: outputs the caller passed in keep what they held."""
    import decaf377_amd as d
    bases, idx, fk, pts, vk, _, _ = mixed325
    bad, mended, _, _ = _plant(idx, 5)
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        enc = torch.full((N, 32), 0x5A, dtype=torch.uint8, device="cuda:0")
        el = torch.full((N, 16), 0x5A5A, dtype=torch.int64, device="cuda:0")
        with pytest.raises(d.NativeError):
            fb.msm_mixed(T(bad), T(fk), T(pts), T(vk), elements=True, outs=[enc, el])
        with pytest.raises(d.NativeError):
            fb.msm_indexed(T(bad), T(fk), elements=True, outs=[enc, el])
        torch.cuda.synchronize()
        assert bool((enc == 0x5A).all()) and bool((el == 0x5A5A).all())
        got = fb.msm_mixed(T(mended), T(fk), T(pts), T(vk), elements=True, outs=[enc, el])     # mended: the same tensors are written
        assert got[0] is enc and got[1] is el
        assert (enc.cpu().numpy() == fb.msm_mixed(mended, fk, pts, vk)).all()
        claimed, _, gave_up = ctx.health()
        assert (claimed, gave_up) == (0, 0)


def test_a_tensor_on_a_gpu_the_context_does_not_own_keeps_the_host_path(torch, oracle, mixed325, monkeypatch):
    """As before the resident forms: staged through host memory, the results back on the tensor's device.  One GPU stands in
    for two: the context is told that its device has another index, so cuda:0 is a GPU it does not own.  The host route
    shows in the result of check_indices=False, which carries no verdict tensor there."""
    import decaf377_amd as d
    bases, idx, fk, pts, vk, _, _ = mixed325
    T = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")
    c = d.Context([0], comb_lazy=True)
    try:
        with c.fixed_bases(bases, comb_bits=12) as fb:
            dense_k = np.ascontiguousarray(fk[:5 * 4])
            want = fb.msm(dense_k), fb.msm_indexed(idx, fk), fb.msm_mixed(idx, fk, pts, vk)
            assert isinstance(fb.msm_indexed(T(idx), T(fk), check_indices=False), tuple)      # owned: resident, with its verdict
            monkeypatch.setattr(c, "device_ids", [7])
            got = fb.msm(T(dense_k)), fb.msm_indexed(T(idx), T(fk), check_indices=False), fb.msm_mixed(T(idx), T(fk), T(pts), T(vk), check_indices=False)
            monkeypatch.undo()
        for g, w in zip(got, want):
            assert not isinstance(g, tuple) and str(g.device) == "cuda:0" and (g.cpu().numpy() == w).all()
    finally:
        c.close()


# ---- refusals on a live context ------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context(torch, oracle, mixed325):
    import decaf377_amd as d
    bases, idx, fk, pts, vk, _, _ = mixed325
    c = d.Context([0], comb_lazy=True)
    try:
        s = Side(torch, c)
        lib = c._lib
        fb = c.fixed_bases(bases, comb_bits=8)
        di, dfk, dp, dvk = s.dev(idx), s.dev(fk), s.dev(pts), s.dev(vk)
        enc, el = s.empty((N, 32), fill=0x5A), s.empty((N, 16), "u64", fill=0x5A5A)
        ver = s.empty((2,), "u64", fill=7)
        off = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
        msg = lambda: lib.d377_last_error().decode()
        # a misaligned pointer: records 16 bytes, indices 4, the verdict 8
        assert s.call("d377_batch_msm_mixed_resident", fb._h, di, off(dfk, 8), 2, dp, dvk, 3, N - 1, enc, el, ver) == ERR_ARG and "aligned" in msg()
        assert s.call("d377_batch_msm_mixed_resident", fb._h, off(di, 2), dfk, 2, dp, dvk, 3, N - 1, enc, el, ver) == ERR_ARG and "base_index" in msg()
        assert s.call("d377_batch_msm_mixed_resident", fb._h, di, dfk, 2, dp, dvk, 3, N, enc, el, off(ver, 4)) == ERR_ARG and "verdict" in msg()
        assert s.call("d377_batch_fixed_msm_indexed_resident", fb._h, di, dfk, 2, N, off(enc, 8), el, ver) == ERR_ARG and "aligned" in msg()
        assert s.call("d377_batch_fixed_msm_resident", fb._h, off(dfk, 4), 3, enc, el) == ERR_ARG and "aligned" in msg()
        assert s.call("d377_check_base_index_resident", fb._h, off(di, 1), 5, ver) == ERR_ARG and "base_index" in msg()
        # a device that is none of the context's
        for bad_dev in (-1, 1):
            args = (c._h, bad_dev, ctypes.c_void_p(s.stream.cuda_stream))
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            assert lib.d377_batch_msm_mixed_resident(*args, fb._h, p(di), p(dfk), 2, p(dp), p(dvk), 3, N, p(enc), p(el), p(ver)) == ERR_ARG and "dev" in msg()
            assert lib.d377_batch_fixed_msm_indexed_resident(*args, fb._h, p(di), p(dfk), 2, N, p(enc), p(el), p(ver)) == ERR_ARG and "dev" in msg()
            assert lib.d377_batch_fixed_msm_resident(*args, fb._h, p(dfk), 3, p(enc), p(el)) == ERR_ARG and "dev" in msg()
            assert lib.d377_batch_fixed_long_msm_resident(*args, fb._h, p(dfk), 3, p(enc), p(el)) == ERR_ARG and "dev" in msg()
            assert lib.d377_check_base_index_resident(*args, fb._h, p(di), 5, p(ver)) == ERR_ARG and "dev" in msg()
        # n == 0 with good arguments: D377_OK, nothing enqueued
        assert s.call("d377_batch_msm_mixed_resident", fb._h, None, None, 2, None, None, 3, 0, None, None, None) == 0
        assert s.call("d377_batch_fixed_msm_indexed_resident", fb._h, None, None, 2, 0, None, None, None) == 0
        assert s.call("d377_batch_fixed_msm_resident", fb._h, None, 0, None, None) == 0
        assert s.call("d377_batch_fixed_long_msm_resident", fb._h, None, 0, None, None) == 0
        # a dead handle
        handle = fb._h
        fb.close()
        assert s.call("d377_batch_msm_mixed_resident", handle, di, dfk, 2, dp, dvk, 3, N, enc, el, ver) == ERR_ARG and "handle" in msg()
        assert s.call("d377_batch_fixed_msm_indexed_resident", handle, di, dfk, 2, N, enc, el, ver) == ERR_ARG and "handle" in msg()
        assert s.call("d377_batch_fixed_msm_resident", handle, dfk, 3, enc, el) == ERR_ARG and "handle" in msg()
        assert s.call("d377_check_base_index_resident", handle, di, 5, ver) == ERR_ARG and "handle" in msg()
        # no refused call wrote anything or touched a lane set
        assert (s.host(enc) == 0x5A).all() and (s.host(el) == 0x5A5A).all() and (s.host(ver) == 7).all()
        claimed, waited, gave_up = c.health()
        assert (claimed, waited, gave_up) == (0, 0, 0)
    finally:
        c.close()


# ---- a captured graph, and scratch that a graph has seen -------------------------------------------------------------------------
def test_graph_replays_and_outlives_the_scratch_it_saw(torch, oracle, mixed325):
    import decaf377_amd as d
    bases, idx, fk, pts, vk, _, _ = mixed325
    v, t = 3, 2
    ln, lm = 3, 65                                               # three dense sums over a long handle: cut into segments
    rng = np.random.default_rng(99)
    lbases = fl.make_bases(oracle, rng, lm, 1)
    lk = rng.integers(0, 256, (ln * lm, 32), dtype=np.uint8)
    c = d.Context([0], comb_lazy=True)                           # a fresh context: no scratch has grown yet
    try:
        s = Side(torch, c)
        fb = c.fixed_bases(bases, comb_bits=8)
        fbl = c.fixed_bases_long(lbases, comb_bits=8)
        segments = fbl.long_plan(ln)[0]
        assert segments > 1                                      # ... so the call uses the partial sums' area
        di, dfk, dp, dvk, dlk = s.dev(idx), s.dev(fk), s.dev(pts), s.dev(vk), s.dev(lk)
        e_ix, e_mx, e_lg = s.empty((N, 32)), s.empty((N, 32)), s.empty((ln, 32))
        v_ix, v_mx = s.empty((2,), "u64", fill=7), s.empty((2,), "u64", fill=7)

        def enqueue(stream):
            s.ok("d377_batch_fixed_msm_indexed_resident", fb._h, di, dfk, t, N, e_ix, None, v_ix, stream=stream)
            s.ok("d377_batch_msm_mixed_resident", fb._h, di, dfk, t, dp, dvk, v, N, e_mx, None, v_mx, stream=stream)
            s.ok("d377_batch_fixed_long_msm_resident", fbl._h, dlk, ln, e_lg, None, stream=stream)

        def expect(what):
            torch.cuda.synchronize()
            hfk, hvk, hlk = dfk.cpu().numpy(), dvk.cpu().numpy(), dlk.cpu().numpy()
            assert (e_ix.cpu().numpy() == fb.msm_indexed(idx, hfk)).all(), what
            assert (e_mx.cpu().numpy() == fb.msm_mixed(idx, hfk, pts, hvk)).all(), what
            assert (e_lg.cpu().numpy() == fbl.msm_long(hlk)).all(), what
            assert v_ix.cpu().tolist() == [0, -1] and v_mx.cpu().tolist() == [0, -1], what

        enqueue(None)                                            # one eager call of each shape: the scratch areas grow here
        expect("eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                # one stream, a linear graph
            enqueue(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            for buf in (dfk, dvk, dlk):                          # new scalars, written in place
                buf.copy_(torch.from_numpy(rng.integers(0, 256, tuple(buf.shape), dtype=np.uint8)))
            for out in (e_ix, e_mx, e_lg):
                out.zero_()
            v_ix.fill_(7); v_mx.fill_(7)
            torch.cuda.synchronize()
            g.replay()
            expect("replay %d" % rep)

        # outgrow both areas the graph has seen: the table scratch (8 tables per lane instead of 3) and the partial sums
        p8 = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (5 * 8, 32), dtype=np.uint8)), dtype=np.uint64)
        k8 = rng.integers(0, 256, (5 * 8, 32), dtype=np.uint8)
        with c.tuning(tiny_max=0):                               # the lane route: the one that uses the table scratch
            got8 = c.msm_small(p8, k8, 8)
        assert (got8 == oracle_fold(oracle, p8, k8, 8)[0]).all()
        bn, bm = 37, 129                                         # 37 x 17 partial sums where the graph's call had 3 x `segments`
        assert bn * plan(bm)[0] > 2 * ln * segments
        bpts, bk, _ = make_case(oracle, rng, bn, bm)
        assert (c.msm_long(bpts, bk, bm) == oracle_fold(oracle, bpts, bk, bm)[0]).all()
        for buf in (dfk, dvk, dlk):
            buf.copy_(torch.from_numpy(rng.integers(0, 256, tuple(buf.shape), dtype=np.uint8)))
        for out in (e_ix, e_mx, e_lg):
            out.zero_()
        v_ix.fill_(7); v_mx.fill_(7)
        torch.cuda.synchronize()
        g.replay()                                               # the old graph, into the areas it was captured with
        expect("replay after the scratch was outgrown")
        claimed, _, gave_up = c.health()
        assert (claimed, gave_up) == (0, 0)
    finally:
        c.close()


def test_cpp_mirror_resident_sums():
    build_and_run_cpp("resident_sums", "CPP_RESIDENT_SUMS_OK", hip_headers=True)
