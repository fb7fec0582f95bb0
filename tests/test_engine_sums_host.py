"""The Python layer of the batched sums (decaf377_amd/engine.py) without a GPU and without the native library: Context.msm_small,
msm_long, msm_buckets, msm_long_indexed and FixedBases.msm, msm_long, msm_indexed, msm_mixed on a context whose library is a stub
that records every call.  What is pinned: the symbol each call reaches, its integer arguments, that a caller's array which is
already contiguous and of the right type is passed as it is, that the outputs returned are the arrays the call wrote, NULL where
elements=False, the shapes and types of the results, and the full text of every ValueError these methods raise."""
import ctypes
import re

import numpy as np
import pytest

import decaf377_amd as d
from decaf377_amd.engine import Context, FixedBases

M = 3                                                            # bases of the stub registration


class Lib:
    """Records (symbol, args) and returns D377_OK; the two calls FixedBases() makes get the answers it reads."""

    def __init__(self):
        self.calls = []
        self.m = 0

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in ("d377_fixed_bases_create", "d377_fixed_bases_create_long"):
                self.m = args[2].value
                args[-1]._obj.value = 5
            if name == "d377_fixed_bases_info":
                args[2]._obj.value = self.m
                args[3]._obj.value = 12
            return 0
        return call


@pytest.fixture()
def ctx():
    c = Context.__new__(Context)
    c._lib = Lib()
    c._h = ctypes.c_void_p(1)
    c.device_ids = [0]
    yield c
    c._h = ctypes.c_void_p()                                     # close() and __del__ then do nothing


@pytest.fixture()
def fb(ctx):
    f = FixedBases(np.zeros((M, 16), np.uint64), comb_bits=12, ctx=ctx)
    assert (f.m, f.comb_bits, f._h) == (M, 12, 5)
    ctx._lib.calls.clear()
    yield f
    f._h = 0


def val(a):
    """A recorded argument as a plain integer or None (NULL)."""
    return a.value if hasattr(a, "value") else a


def last(ctx, symbol, nargs):
    """The arguments of the one call recorded since the last look, which must be `symbol` with `nargs` arguments."""
    assert len(ctx._lib.calls) == 1, [c[0] for c in ctx._lib.calls]
    name, args = ctx._lib.calls.pop()
    assert name == symbol and len(args) == nargs, (name, len(args))
    return [val(a) for a in args]


def last_of(ctx, i):
    name, args = ctx._lib.calls[i]
    return name, [val(a) for a in args[:-1]]


def _index_seen(ctx, symbol, pos, shape, call):
    """The int32 index array the library is handed by `call`, copied while the call runs."""
    seen = []
    lib = ctx._lib
    record = lib.__getattr__(symbol)
    setattr(lib, symbol, lambda *args: (seen.append(np.ctypeslib.as_array(
        ctypes.cast(args[pos], ctypes.POINTER(ctypes.c_int32)), shape).copy()), record(*args))[1])
    try:
        call()
    finally:
        delattr(lib, symbol)
    return seen[0]


def addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def as_tuple(r):
    return r if isinstance(r, tuple) else (r,)


def shapes(res, *want):
    """Every result has its shape and element type: (shape, "u8" / "u64")."""
    res = as_tuple(res)
    assert len(res) == len(want)
    for a, (shape, kind) in zip(res, want):
        assert tuple(a.shape) == shape, (tuple(a.shape), shape)
        if hasattr(a, "data_ptr"):
            import torch
            assert a.dtype == (torch.uint8 if kind == "u8" else torch.int64) and a.device.type == "cpu"
        else:
            assert a.dtype == (np.uint8 if kind == "u8" else np.uint64)


def raises(text):
    return pytest.raises(ValueError, match="^" + re.escape(text) + "$")


def u8(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.uint8).reshape(shape)


def u64(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)


# ---- Context.msm_small / msm_long / msm_buckets ------------------------------------------------------------------------------
SUMS = [("msm_small", "d377_batch_msm_small", ()), ("msm_long", "d377_batch_msm_long", ()), ("msm_buckets", "d377_batch_bucket_msm", (7,))]


def _sums(ctx, method, pts, k, m, **kw):
    return getattr(ctx, method)(pts, k, m, **kw)


@pytest.mark.parametrize("method,symbol,extra", SUMS)
@pytest.mark.parametrize("elements", [False, True])
@pytest.mark.parametrize("encoded", [False, True])
@pytest.mark.parametrize("given", [False, True])
def test_sums_of_m_on_numpy(ctx, method, symbol, extra, elements, encoded, given):
    n, m = 2, 3
    pts, k = (u8(n * m, 32) if encoded else u64(n * m, 16)), u8(n * m, 32)
    specs = [((n, 32), "u8")] + ([((n, 16), "u64")] if elements else []) + ([((n * m,), "u8")] if encoded else [])
    outs = [np.zeros(s, np.uint8 if kd == "u8" else np.uint64) for s, kd in specs] if given else None
    kw = {"window_bits": extra[0]} if extra else {}
    res = _sums(ctx, method, pts, k, m, outs=outs, elements=elements, **kw)
    shapes(res, *specs)
    res = as_tuple(res)
    if given:
        assert all(r is o for r, o in zip(res, outs))
    a = last(ctx, symbol + ("_encoded" if encoded else ""), 7 + len(extra) + encoded)
    assert a[:5] == [1, addr(pts), addr(k), m, n]
    assert tuple(a[5:5 + len(extra)]) == extra
    ptrs = a[5 + len(extra):]
    want = [addr(r) for r in res]
    if not elements:
        want.insert(1, None)
    assert ptrs == want


@pytest.mark.parametrize("method,symbol,extra", SUMS)
def test_sums_of_m_defaults_copies_and_no_sums(ctx, method, symbol, extra):
    pts, k = u64(4, 16), u8(4, 32)
    res = _sums(ctx, method, pts.view(np.int64)[::-1], k[::-1], 2)      # int64 records pass; neither array is contiguous
    shapes(res, ((2, 32), "u8"))
    a = last(ctx, symbol, 7 + len(extra))
    assert a[3:5] == [2, 2] and a[1] not in (addr(pts), None) and a[2] not in (addr(k), None)
    assert tuple(a[5:5 + len(extra)]) == (0,) * len(extra)               # window_bits defaults to 0
    assert a[-2:] == [addr(res), None]
    res = _sums(ctx, method, u64(0, 16), u8(0, 32), 4, elements=True)    # n = 0
    shapes(res, ((0, 32), "u8"), ((0, 16), "u64"))
    a = last(ctx, symbol, 7 + len(extra))
    assert a[3:5] == [4, 0]
    res = _sums(ctx, method, u8(0, 32), u8(0, 32), 1)                    # n = 0, Encodings
    shapes(res, ((0, 32), "u8"), ((0,), "u8"))
    assert last(ctx, symbol + "_encoded", 8 + len(extra))[3:5] == [1, 0]


@pytest.mark.parametrize("method", ["msm_small", "msm_long", "msm_buckets"])
def test_sums_of_m_refusals(ctx, method):
    k = u8(6, 32)
    with raises(method + ": points must be [n * m, 16] Elements or [n * m, 32] Encodings"):
        _sums(ctx, method, u64(6, 8), k, 3)
    with raises(method + ": points must be [n * m, 16] Elements or [n * m, 32] Encodings"):
        _sums(ctx, method, u64(2, 3, 16), k, 3)
    with raises(method + ": the number of points must be a multiple of m"):
        _sums(ctx, method, u64(6, 16), k, 4)
    with raises(method + ": the number of points must be a multiple of m"):
        _sums(ctx, method, u64(6, 16), k, 0)
    with raises(method + " points: expected uint8 elements, got uint64"):
        _sums(ctx, method, u64(6, 32), k, 3)
    with raises(method + " points: expected uint64/int64 elements, got float64"):
        _sums(ctx, method, np.zeros((6, 16)), k, 3)
    with raises(method + " scalars: expected shape (6, 32), got (5, 32)"):
        _sums(ctx, method, u64(6, 16), u8(5, 32), 3)
    with raises(method + " scalars: expected uint8 elements, got int8"):
        _sums(ctx, method, u64(6, 16), u8(6, 32).view(np.int8), 3)
    with raises(method + ": 1 output arrays expected"):
        _sums(ctx, method, u64(6, 16), k, 3, outs=[u8(2, 32), u64(2, 16)])
    with raises(method + ": 3 output arrays expected"):
        _sums(ctx, method, u8(6, 32), k, 3, outs=[u8(2, 32)], elements=True)
    assert not ctx._lib.calls


@pytest.mark.parametrize("method", ["msm_small", "msm_long", "msm_buckets"])
def test_sums_of_m_have_no_cpu_path_for_tensors(ctx, method):
    import torch
    pts, k = torch.zeros((4, 16), dtype=torch.int64), torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(d.NativeError, match=re.escape("torch tensors must live on the GPU")):
        _sums(ctx, method, pts, k, 2)
    with pytest.raises(d.NativeError, match=re.escape("torch tensors must live on the GPU")):
        _sums(ctx, method, k, k, 2, elements=True)
    assert not ctx._lib.calls


def test_msm_buckets_plan(ctx):
    assert ctx.msm_buckets_plan(3, 4, window_bits=9, dev=0) == {"window_bits": 0, "sums_per_pass": 0, "passes": 0, "workspace_bytes": 0}
    assert last(ctx, "d377_bucket_msm_plan", 9)[:5] == [1, 0, 3, 4, 9]


# ---- Context.msm_long_indexed --------------------------------------------------------------------------------------------------
def _idx(n, t, dtype=np.int32):
    idx = (np.arange(n * t).reshape(n, t) % 3).astype(dtype)
    if idx.size:
        idx[0, 0] = -1
    return idx


@pytest.mark.parametrize("elements", [False, True])
@pytest.mark.parametrize("three_d", [False, True])
def test_msm_long_indexed_on_numpy(ctx, elements, three_d):
    n, m, pool = 2, 3, u64(4, 16)
    idx, k = _idx(n, m), (u8(n, m, 32) if three_d else u8(n * m, 32))
    res = ctx.msm_long_indexed(pool, idx, k, m, elements=elements)
    shapes(res, *([((n, 32), "u8")] + ([((n, 16), "u64")] if elements else [])))
    res = as_tuple(res)
    a = last(ctx, "d377_batch_long_msm_indexed", 9)
    assert a == [1, addr(pool), 4, addr(idx), addr(k), m, n, addr(res[0]), addr(res[1]) if elements else None]


def test_msm_long_indexed_converts_an_int64_index(ctx):
    pool, k = u64(4, 16).view(np.int64), u8(6, 32)
    for dtype in (np.int64, np.int16, np.uint8):
        idx = _idx(2, 3).astype(dtype)
        if dtype == np.uint8:
            idx[0, 0] = 0
        seen = _index_seen(ctx, "d377_batch_long_msm_indexed", 3, (2, 3), lambda: ctx.msm_long_indexed(pool, idx, k, 3))
        a = last(ctx, "d377_batch_long_msm_indexed", 9)
        assert a[1] == addr(pool) and a[3] != addr(idx)
        assert (seen == idx).all() and (dtype == np.uint8 or seen[0, 0] == -1)     # the same values as int32; -1 kept


def test_msm_long_indexed_refusals(ctx):
    pool, k = u64(4, 16), u8(6, 32)
    what = "msm_long_indexed"
    with raises(what + ": pool must be [pool_count, 16] Elements"):
        ctx.msm_long_indexed(u64(4, 8), _idx(2, 3), k, 3)
    with raises(what + ": pool must be [pool_count, 16] Elements"):
        ctx.msm_long_indexed(u64(2, 2, 16), _idx(2, 3), k, 3)
    with raises(what + " pool: expected uint64/int64 elements, got uint8"):
        ctx.msm_long_indexed(u8(4, 16), _idx(2, 3), k, 3)
    with raises(what + ": outs goes with tensors on a device of the context"):
        ctx.msm_long_indexed(pool, _idx(2, 3), k, 3, outs=[u8(2, 32)])
    with raises(what + ": point_index must be an [n, m] integer array"):
        ctx.msm_long_indexed(pool, _idx(2, 3).reshape(6), k, 3)
    with raises(what + ": point_index must be an [n, m] integer array"):
        ctx.msm_long_indexed(pool, _idx(2, 3).astype(np.float32), k, 3)
    with raises(what + ": point_index must be [n, m]"):
        ctx.msm_long_indexed(pool, _idx(2, 3), k, 2)
    for bad in (1 << 31, -(1 << 31) - 1):
        idx = _idx(2, 3, np.int64)
        idx[1, 2] = bad
        with raises(what + ": point_index does not fit 32 bits"):
            ctx.msm_long_indexed(pool, idx, k, 3)
    with raises(what + ": scalars [n, m, 32] must match point_index [n, m]"):
        ctx.msm_long_indexed(pool, _idx(2, 3), u8(3, 2, 32), 3)
    with raises(what + " scalars: expected shape (6, 32), got (5, 32)"):
        ctx.msm_long_indexed(pool, _idx(2, 3), u8(5, 32), 3)
    assert not ctx._lib.calls
    idx = _idx(2, 3, np.int64)
    idx[1, 2] = (1 << 31) - 1
    idx[1, 1] = -(1 << 31)                                       # the ends of the range pass; the library judges them
    ctx.msm_long_indexed(pool, idx, k, 3)
    last(ctx, "d377_batch_long_msm_indexed", 9)


def test_msm_long_indexed_on_cpu_tensors(ctx):
    import torch
    pool, idx, k = torch.from_numpy(u64(4, 16).view(np.int64)), torch.from_numpy(_idx(2, 3)), torch.from_numpy(u8(2, 3, 32))
    enc, el = ctx.msm_long_indexed(pool, idx, k, 3, elements=True)
    shapes((enc, el), ((2, 32), "u8"), ((2, 16), "u64"))
    a = last(ctx, "d377_batch_long_msm_indexed", 9)
    assert a == [1, addr(pool), 4, addr(idx), addr(k), 3, 2, addr(enc), addr(el)]
    enc = ctx.msm_long_indexed(pool.numpy().view(np.uint64), idx.numpy(), k, 3)      # one tensor among the arguments: tensors come back
    shapes(enc, ((2, 32), "u8"))
    assert hasattr(enc, "data_ptr") and last(ctx, "d377_batch_long_msm_indexed", 9)[-2:] == [addr(enc), None]


# ---- FixedBases ----------------------------------------------------------------------------------------------------------------
def test_fixed_bases_registration(ctx):
    pts = u64(2, 16)
    f = FixedBases(pts, comb_bits=8, ctx=ctx)
    assert last_of(ctx, 0) == ("d377_fixed_bases_create", [1, addr(pts), 2, 8])
    g = ctx.fixed_bases_long(pts.view(np.int64))
    assert last_of(ctx, 2) == ("d377_fixed_bases_create_long", [1, addr(pts), 2, 12])
    with raises("FixedBases: points must be [m, 16] u64 Element records"):
        FixedBases(u64(2, 8), ctx=ctx)
    with raises("FixedBases: points must be [m, 16] u64 Element records"):
        FixedBases(u8(2, 16), ctx=ctx)
    f._h = g._h = 0


DENSE = [("msm", "d377_batch_fixed_msm", "FixedBases.msm"), ("msm_long", "d377_batch_fixed_long_msm", "FixedBases.msm_long")]


@pytest.mark.parametrize("method,symbol,what", DENSE)
def test_dense_sums(ctx, fb, method, symbol, what):
    import torch
    k = u8(2 * M, 32)
    enc = getattr(fb, method)(k)
    shapes(enc, ((2, 32), "u8"))
    assert last(ctx, symbol, 6) == [1, 5, addr(k), 2, addr(enc), None]
    enc, el = getattr(fb, method)(k[::-1], elements=True)
    shapes((enc, el), ((2, 32), "u8"), ((2, 16), "u64"))
    a = last(ctx, symbol, 6)
    assert a[:2] + a[3:] == [1, 5, 2, addr(enc), addr(el)] and a[2] not in (addr(k), None)
    enc, el = getattr(fb, method)(u8(0, 32), elements=True)               # n = 0
    shapes((enc, el), ((0, 32), "u8"), ((0, 16), "u64"))
    assert last(ctx, symbol, 6)[3] == 0
    t = torch.from_numpy(k)                                               # a CPU tensor: the host route, tensors back
    enc, el = getattr(fb, method)(t, elements=True)
    shapes((enc, el), ((2, 32), "u8"), ((2, 16), "u64"))
    assert hasattr(enc, "data_ptr") and hasattr(el, "data_ptr")
    assert last(ctx, symbol, 6) == [1, 5, addr(k), 2, addr(enc), addr(el)]
    with raises(what + ": the number of scalars must be a multiple of m = 3"):
        getattr(fb, method)(u8(4, 32))
    with raises(what + " scalars: expected shape (6, 32), got (6, 31)"):
        getattr(fb, method)(u8(6, 31))
    with raises(what + " scalars: expected uint8 elements, got uint64"):
        getattr(fb, method)(u64(6, 32))
    assert not ctx._lib.calls


def test_vartime_multiscalar_mul_is_msm(ctx, fb):
    k = u8(2 * M, 32)
    for arg in (k, d.Fr(k, ctx)):
        enc = fb.vartime_multiscalar_mul(arg)
        assert isinstance(enc, d.Encoding) and enc.ctx is ctx
        shapes(enc.data, ((2, 32), "u8"))
        assert last(ctx, "d377_batch_fixed_msm", 6) == [1, 5, addr(k), 2, addr(enc.data), None]


@pytest.mark.parametrize("elements", [False, True])
@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("tensors", [False, True])
def test_msm_indexed_on_the_host_route(ctx, fb, elements, three_d, tensors):
    n, t = 2, 4
    idx, k = _idx(n, t), (u8(n, t, 32) if three_d else u8(n * t, 32))
    args = (idx, k)
    if tensors:
        import torch
        args = (torch.from_numpy(idx), torch.from_numpy(k))
    res = fb.msm_indexed(*args, elements=elements)
    shapes(res, *([((n, 32), "u8")] + ([((n, 16), "u64")] if elements else [])))
    res = as_tuple(res)
    assert all(hasattr(r, "data_ptr") == tensors for r in res)
    a = last(ctx, "d377_batch_fixed_msm_indexed", 8)
    assert a == [1, 5, addr(idx), addr(k), t, n, addr(res[0]), addr(res[1]) if elements else None]


def test_msm_indexed_converts_and_refuses(ctx, fb):
    import torch
    what = "FixedBases.msm_indexed"
    k = u8(8, 32)
    idx = _idx(2, 4, np.int64)
    got = _index_seen(ctx, "d377_batch_fixed_msm_indexed", 2, (2, 4), lambda: fb.msm_indexed(idx, k))
    assert (got == idx).all() and got[0, 0] == -1
    assert last(ctx, "d377_batch_fixed_msm_indexed", 8)[2] != addr(idx)
    got = _index_seen(ctx, "d377_batch_fixed_msm_indexed", 2, (2, 4), lambda: fb.msm_indexed(torch.from_numpy(idx), k))
    assert (got == idx).all()
    enc = fb.msm_indexed(_idx(0, 4), u8(0, 32))                          # n = 0
    shapes(enc, ((0, 32), "u8"))
    ctx._lib.calls.clear()
    with raises(what + ": outs goes with tensors on a device of the context"):
        fb.msm_indexed(_idx(2, 4), k, outs=[u8(2, 32)])
    with raises(what + ": base_index must be an [n, t] integer array"):
        fb.msm_indexed(_idx(2, 4).reshape(8), k)
    with raises(what + ": base_index must be an [n, t] integer array"):
        fb.msm_indexed(_idx(2, 4).astype(np.float64), k)
    for bad in (1 << 31, -(1 << 31) - 1):
        idx = _idx(2, 4, np.int64)
        idx[1, 3] = bad
        with raises(what + ": base_index does not fit 32 bits"):
            fb.msm_indexed(idx, k)
    with raises(what + ": scalars [n, t, 32] must match base_index [n, t]"):
        fb.msm_indexed(_idx(2, 4), u8(4, 2, 32))
    with raises(what + " scalars: expected shape (8, 32), got (7, 32)"):
        fb.msm_indexed(_idx(2, 4), u8(7, 32))
    assert not ctx._lib.calls


@pytest.mark.parametrize("elements", [False, True])
@pytest.mark.parametrize("encoded", [False, True])
@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("tensors", [False, True])
def test_msm_mixed_on_the_host_route(ctx, fb, elements, encoded, three_d, tensors):
    n, t, v = 2, 4, 3
    idx = _idx(n, t)
    fk, vk = u8(n * t, 32), u8(n * v, 32) + 1
    pts = u8(n * v, 32) + 2 if encoded else u64(n * v, 16)
    if three_d:
        fk, vk, pts = fk.reshape(n, t, 32), vk.reshape(n, v, 32), pts.reshape(n, v, -1)
    args = (idx, fk, pts, vk)
    if tensors:
        import torch
        args = tuple(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a) for a in args)
    res = fb.msm_mixed(*args, elements=elements)
    specs = [((n, 32), "u8")] + ([((n, 16), "u64")] if elements else []) + ([((n * v,), "u8")] if encoded else [])
    shapes(res, *specs)
    res = as_tuple(res)
    assert all(hasattr(r, "data_ptr") == tensors for r in res)
    a = last(ctx, "d377_batch_msm_mixed" + ("_encoded" if encoded else ""), 11 + encoded)
    assert a[:9] == [1, 5, addr(idx), addr(fk), t, addr(pts), addr(vk), v, n]
    assert a[9:] == [addr(res[0]), addr(res[1]) if elements else None] + ([addr(res[-1])] if encoded else [])


def test_msm_mixed_converts_and_refuses(ctx, fb):
    what = "FixedBases.msm_mixed"
    n, t, v = 2, 4, 3
    fk, vk, pts = u8(n * t, 32), u8(n * v, 32), u64(n * v, 16)
    idx = _idx(n, t, np.int64)
    got = _index_seen(ctx, "d377_batch_msm_mixed", 2, (n, t), lambda: fb.msm_mixed(idx, fk, pts, vk))
    assert (got == idx).all() and got[0, 0] == -1
    a = last(ctx, "d377_batch_msm_mixed", 11)
    assert a[2] != addr(idx) and a[3:9] == [addr(fk), t, addr(pts), addr(vk), v, n]
    res = fb.msm_mixed(_idx(0, t), u8(0, 32), u64(0, 16), u8(0, 32), elements=True)       # n = 0: v counts as 1
    shapes(res, ((0, 32), "u8"), ((0, 16), "u64"))
    assert last(ctx, "d377_batch_msm_mixed", 11)[7:9] == [1, 0]
    res = fb.msm_mixed(_idx(0, t), u8(0, t, 32), u8(0, 2, 32), u8(0, 32))                  # n = 0, Encodings
    shapes(res, ((0, 32), "u8"), ((0,), "u8"))
    assert last(ctx, "d377_batch_msm_mixed_encoded", 12)[7:9] == [1, 0]
    idx = _idx(n, t)
    with raises(what + ": outs goes with tensors on a device of the context"):
        fb.msm_mixed(idx, fk, pts, vk, outs=[u8(2, 32)])
    with raises(what + ": base_index must be an [n, t] integer array"):
        fb.msm_mixed(idx.reshape(n * t), fk, pts, vk)
    with raises(what + ": base_index must be an [n, t] integer array"):
        fb.msm_mixed(idx.astype(np.float32), fk, pts, vk)
    for bad in (1 << 31, -(1 << 31) - 1):
        wide = _idx(n, t, np.int64)
        wide[1, 1] = bad
        with raises(what + ": base_index does not fit 32 bits"):
            fb.msm_mixed(wide, fk, pts, vk)
    with raises(what + ": fixed scalars [n, t, 32] must match base_index [n, t]"):
        fb.msm_mixed(idx, fk.reshape(t, n, 32), pts, vk)
    with raises(what + " fixed scalars: expected shape (8, 32), got (7, 32)"):
        fb.msm_mixed(idx, fk[:7], pts, vk)
    with raises(what + ": points [n, v, .] must have one row per sum"):
        fb.msm_mixed(idx, fk, pts.reshape(v, n, 16), vk)
    with raises(what + ": the number of points must be a multiple of the number of sums"):
        fb.msm_mixed(idx, fk, pts[:5], vk[:5])
    with raises(what + ": the number of points must be a multiple of the number of sums"):
        fb.msm_mixed(_idx(0, t), u8(0, 32), pts, vk)
    with raises(what + " points: expected shape (6, 16), got (6, 32)"):
        fb.msm_mixed(idx, fk, u64(n * v, 32), vk)
    with raises(what + " points: expected shape (6, 32), got (6, 16)"):
        fb.msm_mixed(idx, fk, u8(n * v, 16), vk)
    with raises(what + " points: expected uint64/int64 elements, got float64"):
        fb.msm_mixed(idx, fk, np.zeros((n * v, 16)), vk)
    with raises(what + ": variable scalars [n, v, 32] must match the points [n, v, .]"):
        fb.msm_mixed(idx, fk, pts, vk.reshape(v, n, 32))
    with raises(what + " variable scalars: expected shape (6, 32), got (5, 32)"):
        fb.msm_mixed(idx, fk, pts, vk[:5])
    assert not ctx._lib.calls


def test_a_closed_handle_is_refused(ctx, fb):
    fb._h = 0
    idx, k = _idx(2, 4), u8(8, 32)
    calls = [lambda: fb.msm(u8(6, 32)), lambda: fb.msm_long(u8(6, 32)), lambda: fb.msm_indexed(idx, k),
             lambda: fb.msm_mixed(idx, k, u64(6, 16), u8(6, 32)), lambda: fb.vartime_multiscalar_mul(u8(6, 32)), fb.info,
             lambda: fb.long_plan(2)]
    for call in calls:
        with pytest.raises(d.NativeError, match=re.escape("FixedBases: the handle is closed")):
            call()
    assert not ctx._lib.calls


# ---- Context.fq_op / fq_from_bytes_checked / fq_to_bytes: outs like every other element-wise map --------------------------------
def test_fq_maps_take_outs_and_check_them(ctx):
    n = 3
    a, b, raw = u64(n, 4), u64(n, 4) + 1, u8(n, 32)
    # the caller's arrays are the ones the call writes and returns, in place included; the unary codes pass b = NULL
    out, st = u64(n, 4), u8(n)
    res = ctx.fq_op("mul", a, b, outs=[out, st])
    assert res[0] is out and res[1] is st
    assert last(ctx, "d377_batch_fq_op", 7) == [1, 2, addr(a), addr(b), n, addr(out), addr(st)]
    res = ctx.fq_op("inverse", a, outs=[a, st])
    assert res[0] is a and last(ctx, "d377_batch_fq_op", 7) == [1, 5, addr(a), None, n, addr(a), addr(st)]
    res = ctx.fq_op("add", a, b)
    shapes(tuple(res), ((n, 4), "u64"), ((n,), "u8"))
    args = last(ctx, "d377_batch_fq_op", 7)
    assert args[:5] == [1, 0, addr(a), addr(b), n] and args[5:] == [addr(res[0]), addr(res[1])]
    res = ctx.fq_from_bytes_checked(raw, outs=[out, st])
    assert res[0] is out and res[1] is st and last(ctx, "d377_batch_fq_from_bytes_checked", 5) == [1, addr(raw), n, addr(out), addr(st)]
    shapes(tuple(ctx.fq_from_bytes_checked(raw)), ((n, 4), "u64"), ((n,), "u8"))
    ctx._lib.calls.clear()
    enc = u8(n, 32)
    assert ctx.fq_to_bytes(a, outs=[enc]) is enc and last(ctx, "d377_batch_fq_to_bytes", 4) == [1, addr(a), n, addr(enc)]
    shapes(ctx.fq_to_bytes(a), ((n, 32), "u8"))
    ctx._lib.calls.clear()
    # ... and checked like the inputs, before any call
    with raises("d377_batch_fq_op: expected 2 output arrays"):
        ctx.fq_op("mul", a, b, outs=[out])
    with raises("d377_batch_fq_op output: expected shape (3, 4), got (2, 4)"):
        ctx.fq_op("mul", a, b, outs=[u64(2, 4), st])
    with raises("d377_batch_fq_op output: expected shape (3,), got (4,)"):
        ctx.fq_op("neg", a, outs=[out, u8(4)])
    with raises("d377_batch_fq_op output: expected uint64/int64 elements, got uint8"):
        ctx.fq_op("square", a, outs=[u8(n, 4), st])
    with raises("d377_batch_fq_op output must be contiguous"):
        ctx.fq_op("mul", a, b, outs=[u64(n, 8)[:, :4], st])
    with raises("fq_op mul takes two operands"):
        ctx.fq_op("mul", a, outs=[out, st])
    with raises("fq_op: operands have 3 and 2 rows"):
        ctx.fq_op("mul", a, b[:2])
    with raises("d377_batch_fq_from_bytes_checked output: expected shape (3, 4), got (3, 32)"):
        ctx.fq_from_bytes_checked(raw, outs=[u8(n, 32), st])
    with raises("d377_batch_fq_from_bytes_checked: expected 2 output arrays"):
        ctx.fq_from_bytes_checked(raw, outs=[out])
    with raises("d377_batch_fq_to_bytes output: expected uint8 elements, got uint64"):
        ctx.fq_to_bytes(a, outs=[u64(n, 32)])
    with raises("d377_batch_fq_to_bytes: expected 1 output arrays"):
        ctx.fq_to_bytes(a, outs=[enc, st])
    assert not ctx._lib.calls
