"""Fixed-base combs for caller-chosen points on the MI355X (d377_fixed_bases_create / d377_batch_fixed_msm), against the
oracle and against the library's own oracle-checked operations.

The oracle's fold for a large batch of sums over FIXED bases is computed the way a comb does it, with the oracle's own group
law: k B = sum_w (byte w of k mod r) 256^w B, the 32 x 256 multiples of each base made once by oracle additions and
doublings and every term folded by oracle additions -- the same values as scalar_mul_xyzt, 10x cheaper, and the encodings
are canonical, so they compare byte for byte."""
import threading

import numpy as np
import pytest

from _sums_support import Fold, build_and_run_cpp, planted_scalars as _scalars, random_bases as _bases

WIDTHS = [8, 12, 16, 18]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    c.close()


@pytest.mark.parametrize("m", [1, 2, 3, 8, 64])
def test_every_width_and_size_against_the_oracle(ctx, oracle, m):
    rng = np.random.default_rng(m)
    bases = _bases(oracle, rng, m)
    nmax = 1 << 16
    k = _scalars(rng, nmax, m)
    want_enc, want_el = Fold(oracle, bases).dense(k)
    for bits in WIDTHS:
        with ctx.fixed_bases(bases, comb_bits=bits) as fb:
            assert fb.info()[:2] == (m, bits)
            for n in (1, 63, 4097, nmax):
                enc, el = fb.msm(k[:n * m], elements=True)
                assert (enc == want_enc[:n]).all(), (bits, n, np.nonzero((enc != want_enc[:n]).any(1))[0][:8])
                assert oracle.eq_xyzt(el, want_el[:n]).all(), (bits, n)
                if n <= 4097:
                    assert (oracle.compress(el) == enc).all(), (bits, n)
                else:
                    assert (ctx.compress(el) == enc).all(), (bits, n)


def test_generator_base_equals_the_context_comb(oracle):
    import decaf377_amd as d
    c = d.Context([0], comb_bits=18)
    rng = np.random.default_rng(18)
    k = rng.integers(0, 256, (1 << 20, 32), dtype=np.uint8)
    with c.fixed_bases(oracle.generator_xyzt().reshape(1, 16), comb_bits=18) as fb:
        got = fb.msm(k)
    assert (got == c.scalar_mul_base(k)).all()
    assert (got[::4099] == oracle.scalar_mul_base(k[::4099])).all()
    c.close()


def test_degenerate_bases(ctx, oracle):
    """The identity, a Z = 0 record (counted as the identity), a representative with Z != 1, the same point twice, P and -P,
    and P + (0, -1) in place of P."""
    rng = np.random.default_rng(7)
    p = oracle.elligator_map_xyzt(rng.integers(0, 256, (3, 32), dtype=np.uint8))
    ident = oracle.identity_xyzt()
    zero_z = p[2].copy().reshape(4, 4)
    zero_z[2] = 0
    lam = np.tile(p[1][:4], (4, 1))
    scaled = oracle.fq_op(2, p[0].reshape(4, 4), lam)[0].reshape(16)
    tors = p[0].reshape(4, 4).copy()
    tors[:2] = oracle.fq_op(4, tors[:2])[0]
    bases = np.stack([ident, zero_z.reshape(16), scaled, p[0], p[0], oracle.neg_xyzt(p[0].reshape(1, 16))[0], tors.reshape(16), p[1]])
    as_group = bases.copy()
    as_group[1] = ident                                          # what the Z = 0 record stands for
    n = 4097
    k = _scalars(rng, n, bases.shape[0])
    want_enc, want_el = Fold(oracle, as_group).dense(k)
    for bits in (8, 16):
        with ctx.fixed_bases(bases, comb_bits=bits) as fb:
            enc, el = fb.msm(k, elements=True)
        assert (enc == want_enc).all(), bits
        assert oracle.eq_xyzt(el, want_el).all(), bits


def test_two_bases_at_4m_sums_against_the_composition(ctx, oracle):
    rng = np.random.default_rng(22)
    bases = _bases(oracle, rng, 2)
    n = 1 << 22
    k = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    with ctx.fixed_bases(bases, comb_bits=16) as fb:
        enc = fb.msm(k)
    k2 = k.reshape(n, 2, 32)
    a = ctx.scalar_mul_var_element(np.ascontiguousarray(np.broadcast_to(bases[0], (n, 16))), np.ascontiguousarray(k2[:, 0]))
    b = ctx.scalar_mul_var_element(np.ascontiguousarray(np.broadcast_to(bases[1], (n, 16))), np.ascontiguousarray(k2[:, 1]))
    want = ctx.compress(ctx.add(a, b))
    assert (enc == want).all(), np.nonzero((enc != want).any(1))[0][:8]
    idx = np.arange(0, n, 8191)
    s = oracle.add_xyzt(oracle.scalar_mul_xyzt(np.tile(bases[0], (len(idx), 1)), k2[idx, 0]),
                        oracle.scalar_mul_xyzt(np.tile(bases[1], (len(idx), 1)), k2[idx, 1]))
    assert (enc[idx] == oracle.compress(s)).all()


def test_device_listed_twice_gives_the_same_bytes(oracle):
    import decaf377_amd as d
    rng = np.random.default_rng(2)
    bases = _bases(oracle, rng, 3)
    k = rng.integers(0, 256, (3 * 100003, 32), dtype=np.uint8)
    out = []
    for ids in ([0], [0, 0]):
        c = d.Context(ids, comb_lazy=True)
        with c.fixed_bases(bases, comb_bits=12) as fb:
            out.append(fb.msm(k, elements=True))
        c.close()
    assert (out[0][0] == out[1][0]).all()
    assert oracle.eq_xyzt(out[0][1][::97], out[1][1][::97]).all()


def test_concurrent_calls_on_one_handle(ctx, oracle):
    rng = np.random.default_rng(3)
    b1, b2 = _bases(oracle, rng, 3), _bases(oracle, rng, 2)
    k1 = rng.integers(0, 256, (3 * 20000, 32), dtype=np.uint8)
    k2 = rng.integers(0, 256, (2 * 20000, 32), dtype=np.uint8)
    with ctx.fixed_bases(b1, comb_bits=12) as f1, ctx.fixed_bases(b2, comb_bits=16) as f2:
        want1, want2 = f1.msm(k1), f2.msm(k2)
        errors = []

        def worker(fb, k, want):
            try:
                for _ in range(6):
                    if not (fb.msm(k) == want).all():
                        errors.append("mismatch")
            except Exception as e:                                # noqa: BLE001 -- reported below
                errors.append(repr(e))
        ts = [threading.Thread(target=worker, args=a) for a in ((f1, k1, want1), (f1, k1, want1), (f2, k2, want2))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    idx = np.arange(0, 20000, 997)
    assert (want1[idx] == Fold(oracle, b1).dense(k1.reshape(-1, 3, 32)[idx].reshape(-1, 32))[0]).all()


def test_create_destroy_returns_device_memory(ctx, oracle):
    import torch
    bases = _bases(oracle, np.random.default_rng(4), 2)
    with ctx.fixed_bases(bases, comb_bits=16) as fb:             # first use: residency, staging
        fb.msm(np.zeros((2, 32), np.uint8))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        fb = ctx.fixed_bases(bases, comb_bits=16)
        fb.msm(np.zeros((2 * 64, 32), np.uint8))
        fb.close()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert abs(free0 - free1) <= 1 << 20, (free0, free1)


def test_closed_handle_raises(oracle):
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    bases = _bases(oracle, np.random.default_rng(5), 1)
    fb = c.fixed_bases(bases, comb_bits=8)
    fb.close()
    with pytest.raises(d.NativeError):
        fb.msm(np.zeros((1, 32), np.uint8))
    fb2 = c.fixed_bases(bases, comb_bits=8)
    c.close()                                                     # closes its handles first
    with pytest.raises(d.NativeError):
        fb2.msm(np.zeros((1, 32), np.uint8))
    fb2.close()                                                   # harmless
    with pytest.raises(d.NativeError):
        c.fixed_bases(bases, comb_bits=8)


def test_high_level_and_torch_staging(oracle):
    import torch
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    rng = np.random.default_rng(6)
    bases = _bases(oracle, rng, 2)
    k = rng.integers(0, 256, (2 * 4096, 32), dtype=np.uint8)
    fb = d.FixedBases(d.Element(bases, c), comb_bits=12)
    enc = fb.vartime_multiscalar_mul(d.Fr(k, c))
    want = Fold(oracle, bases).dense(k)[0]
    assert (enc.data == want).all()
    t_enc, t_el = fb.msm(torch.from_numpy(k).to("cuda:0"), elements=True)
    assert t_enc.device.type == "cuda" and t_el.device.type == "cuda"
    assert (t_enc.cpu().numpy() == want).all()
    fb.close()
    c.close()


def test_cpp_mirror_fixed_bases():
    build_and_run_cpp("fixed_bases", "CPP_FIXED_BASES_OK")
