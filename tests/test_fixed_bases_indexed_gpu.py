"""Fixed-base sums whose terms name their bases on the MI355X (d377_batch_fixed_msm_indexed), against the oracle and against
the dense call (d377_batch_fixed_msm) on the same sums.

The oracle side is the byte-table fold of tests/test_fixed_bases_gpu.py (k B = sum_w (byte w of k mod r) 256^w B, the
32 x 256 multiples of each base made once by oracle additions and doublings, every term folded by oracle additions),
picking the table of base_index[i, j] for term j; an absent term adds entry 0, the identity.  One fold per (m, t), at the
largest n, serves every comb width and every smaller n."""
import ctypes
import threading

import numpy as np
import pytest

from _sums_support import R, Fold, build_and_run_cpp, planted_scalars as _scalars, random_bases as _bases, scalar_bytes as _scalar_bytes

SIZES = (1, 63, 257, 4097)

pytestmark = pytest.mark.gpu


def _rows(rng, n, t, m, k):
    """n x t index rows: random, about 10 % of the terms absent, and the planted rows in sums 0 .. 6 (kept within the first
    63 sums, so that every n > 1 sees them; sum 0 is planted for n = 1).  Writes the cancelling row's scalars into k."""
    idx = rng.integers(0, m, (n, t)).astype(np.int32)
    idx[rng.random((n, t)) < 0.1] = -1
    idx[0] = m - 1                                               # every term the last base
    idx[1] = -1                                                  # no term at all: the identity
    idx[2] = 1 % m                                               # one index repeated
    cancel = None
    if t >= 2:                                                   # a twice, with k and r - k: the identity
        cancel = 3
        idx[3] = -1
        idx[3, 0] = idx[3, t - 1] = m - 1
        kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
        k[3 * t] = _scalar_bytes(kv)
        k[3 * t + t - 1] = _scalar_bytes(R - kv)
    idx[4] = rng.integers(0, m, t)
    idx[5] = rng.integers(0, m, t)
    idx[6] = rng.integers(0, m, t)
    idx[4, 0] = -1                                               # absent first, middle, last
    idx[5, t // 2] = -1
    idx[6, t - 1] = -1
    return np.ascontiguousarray(idx), 1, cancel


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    c.close()


@pytest.mark.parametrize("m,t,widths", [(1, 1, (8, 12, 16, 18)), (3, 2, (8, 12, 16, 18)), (5, 7, (8, 12, 16, 18)),
                                        (64, 3, (8, 12)), (64, 64, (8, 12))])
def test_every_width_and_size_against_the_oracle(ctx, oracle, m, t, widths):
    rng = np.random.default_rng(100 * m + t)
    bases = _bases(oracle, rng, m)
    nmax = SIZES[-1]
    k = _scalars(rng, nmax, t)
    idx, absent, cancel = _rows(rng, nmax, t, m, k)
    want_enc, want_el = Fold(oracle, bases)(idx, k)
    assert not want_enc[absent].any()
    for bits in widths:
        with ctx.fixed_bases(bases, comb_bits=bits) as fb:
            for n in SIZES:
                enc, el = fb.msm_indexed(idx[:n], k[:n * t], elements=True)
                assert enc.shape == (n, 32) and el.shape == (n, 16)
                assert (enc == want_enc[:n]).all(), (bits, n, np.nonzero((enc != want_enc[:n]).any(1))[0][:8])
                assert oracle.eq_xyzt(el, want_el[:n]).all(), (bits, n)
                assert (oracle.compress(el) == enc).all(), (bits, n)
                if n > absent:
                    assert not enc[absent].any() and oracle.is_identity(el[absent:absent + 1]).all(), (bits, n)
                if cancel is not None and n > cancel:
                    assert not enc[cancel].any() and oracle.is_identity(el[cancel:cancel + 1]).all(), (bits, n)
            enc3 = fb.msm_indexed(idx[:63].astype(np.int64), k[:63 * t].reshape(63, t, 32))   # int64 rows, [n, t, 32] scalars
            assert (enc3 == want_enc[:63]).all(), bits


@pytest.fixture(scope="module")
def dense8(ctx, oracle):
    """m = 8 bases at 16 bits and 2^16 + 1 sums' worth of scalars for the comparisons with the dense call."""
    rng = np.random.default_rng(816)
    bases = _bases(oracle, rng, 8)
    n = (1 << 16) + 1
    fb = ctx.fixed_bases(bases, comb_bits=16)
    yield fb, rng, n
    fb.close()


def test_three_terms_equal_the_dense_call_on_scattered_scalars(dense8):
    fb, rng, n = dense8
    idx = np.ascontiguousarray(np.argsort(rng.random((n, 8)), axis=1)[:, :3].astype(np.int32))   # three distinct bases per sum
    k = rng.integers(0, 256, (n, 3, 32), dtype=np.uint8)
    dense = np.zeros((n, 8, 32), np.uint8)
    dense[np.arange(n)[:, None], idx] = k
    want = fb.msm(dense.reshape(n * 8, 32))
    got = fb.msm_indexed(idx, k)
    assert (got == want).all(), np.nonzero((got != want).any(1))[0][:8]
    # the terms of each sum in another order: the same encodings
    perm = np.argsort(rng.random((n, 3)), axis=1)
    rows = np.arange(n)[:, None]
    got2 = fb.msm_indexed(np.ascontiguousarray(idx[rows, perm]), np.ascontiguousarray(k[rows, perm]))
    assert (got2 == want).all()


def test_a_permutation_of_all_bases_equals_the_dense_call(dense8):
    fb, rng, n = dense8
    perm = np.ascontiguousarray(np.argsort(rng.random((n, 8)), axis=1).astype(np.int32))
    k = rng.integers(0, 256, (n, 8, 32), dtype=np.uint8)
    dense = np.zeros((n, 8, 32), np.uint8)
    dense[np.arange(n)[:, None], perm] = k                       # term j of the indexed sum is base perm[i, j]
    want = fb.msm(dense.reshape(n * 8, 32))
    got = fb.msm_indexed(perm, k)
    assert (got == want).all(), np.nonzero((got != want).any(1))[0][:8]


@pytest.mark.parametrize("bad", [3, -2])
def test_bad_index_is_refused_and_nothing_is_written(ctx, oracle, bad):
    import decaf377_amd as d
    rng = np.random.default_rng(33)
    bases = _bases(oracle, rng, 3)
    n, t = 1000, 2
    idx = rng.integers(-1, 3, (n, t)).astype(np.int32)
    pos = 2 * 777 + 1
    idx[777, 1] = bad
    idx[900, 0] = bad                                            # a later one: the FIRST offending position is named
    k = rng.integers(0, 256, (n * t, 32), dtype=np.uint8)
    with ctx.fixed_bases(bases, comb_bits=8) as fb:
        with pytest.raises(d.NativeError) as e:
            fb.msm_indexed(idx, k)
        assert "base_index" in str(e.value) and "[%d]" % pos in str(e.value)
        enc = np.full((n, 32), 0x5A, np.uint8)
        el = np.full((n, 16), 0x5A5A5A5A5A5A5A5A, np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = ctx._lib.d377_batch_fixed_msm_indexed(ctx._h, fb._h, p(idx), p(k), t, n, p(enc), p(el))
        assert rc == -2
        msg = ctx._lib.d377_last_error().decode()
        assert "base_index" in msg and "[%d]" % pos in msg
        assert (enc == 0x5A).all() and (el == 0x5A5A5A5A5A5A5A5A).all()
        idx[777, 1] = idx[900, 0] = -1                           # mended: the call goes through
        assert fb.msm_indexed(idx, k).shape == (n, 32)


def test_device_listed_twice_gives_the_same_bytes(oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(2)
    bases = _bases(oracle, rng, 3)
    n, t = 100003, 2
    idx = rng.integers(-1, 3, (n, t)).astype(np.int32)
    k = rng.integers(0, 256, (n * t, 32), dtype=np.uint8)
    out = []
    for ids in ([0], [0, 0]):
        c = d.Context(ids, comb_lazy=True)
        with c.fixed_bases(bases, comb_bits=12) as fb:
            out.append(fb.msm_indexed(idx, k, elements=True))
        c.close()
    assert (out[0][0] == out[1][0]).all()
    assert oracle.eq_xyzt(out[0][1][::97], out[1][1][::97]).all()
    sub = np.arange(0, n, 997)
    assert (out[0][0][sub] == Fold(oracle, bases)(idx[sub], k.reshape(n, t, 32)[sub].reshape(-1, 32))[0]).all()


def test_two_threads_alternate_dense_and_indexed_on_one_handle(ctx, oracle):
    rng = np.random.default_rng(3)
    bases = _bases(oracle, rng, 3)
    n = 20000
    kd = rng.integers(0, 256, (3 * n, 32), dtype=np.uint8)
    ki = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    idx = rng.integers(-1, 3, (n, 2)).astype(np.int32)
    with ctx.fixed_bases(bases, comb_bits=12) as fb:
        want_d, want_i = fb.msm(kd), fb.msm_indexed(idx, ki)
        errors = []

        def worker(first):
            try:
                for c in range(6):
                    if (c + first) % 2:
                        ok = (fb.msm_indexed(idx, ki) == want_i).all()
                    else:
                        ok = (fb.msm(kd) == want_d).all()
                    if not ok:
                        errors.append("mismatch in call %d" % c)
            except Exception as e:                                # noqa: BLE001 -- reported below
                errors.append(repr(e))
        ts = [threading.Thread(target=worker, args=(a,)) for a in (0, 1)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert not errors, errors
    sub = np.arange(0, n, 499)
    assert (want_i[sub] == Fold(oracle, bases)(idx[sub], ki.reshape(n, 2, 32)[sub].reshape(-1, 32))[0]).all()


def test_closed_handle_and_closed_context_raise(oracle):
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    bases = _bases(oracle, np.random.default_rng(5), 1)
    idx, k = np.zeros((1, 1), np.int32), np.zeros((1, 32), np.uint8)
    fb = c.fixed_bases(bases, comb_bits=8)
    assert not fb.msm_indexed(idx, k).any()                      # 0 * B
    fb.close()
    with pytest.raises(d.NativeError):
        fb.msm_indexed(idx, k)
    fb2 = c.fixed_bases(bases, comb_bits=8)
    c.close()                                                     # closes its handles first
    with pytest.raises(d.NativeError):
        fb2.msm_indexed(idx, k)


def test_torch_staging(oracle):
    import torch
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    rng = np.random.default_rng(6)
    bases = _bases(oracle, rng, 4)
    n, t = 4096, 2
    idx = rng.integers(-1, 4, (n, t)).astype(np.int32)
    k = rng.integers(0, 256, (n * t, 32), dtype=np.uint8)
    want = Fold(oracle, bases)(idx, k)[0]
    with d.FixedBases(d.Element(bases, c), comb_bits=12) as fb:
        t_enc, t_el = fb.msm_indexed(torch.from_numpy(idx).to("cuda:0"), torch.from_numpy(k).to("cuda:0"), elements=True)
        assert str(t_enc.device) == "cuda:0" and str(t_el.device) == "cuda:0"
        assert (t_enc.cpu().numpy() == want).all()
        assert (oracle.compress(t_el.cpu().numpy().view(np.uint64)) == want).all()
    c.close()


def test_cpp_mirror_fixed_bases_indexed():
    build_and_run_cpp("fixed_bases_indexed", "CPP_FIXED_BASES_INDEXED_OK")
