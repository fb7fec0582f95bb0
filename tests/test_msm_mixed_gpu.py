"""Mixed sums, registered bases plus variable points, on the MI355X (d377_batch_msm_mixed / _encoded) against the oracle and
against the composition of the existing calls (d377_batch_msm_small, d377_batch_fixed_msm_indexed, d377_batch_add,
d377_batch_compress).

The oracle side: the variable terms by scalar_mul_xyzt, the fixed part by the byte-table fold of
tests/test_fixed_bases_indexed_gpu.py (restated here: k B = sum_w (byte w of k mod r) 256^w B), everything joined by add_xyzt.
One fold per shape, at the largest n, kept as the fixed sums and the separate variable terms, serves every smaller n and the
Encoding form (a dropped term is left out of the joining additions)."""
import numpy as np
import pytest

from _sums_support import (ABSENT, CANCEL, VZERO, Fold, _p, build_and_run_cpp, join as _join, mixed_case as _case, random_bases as _bases,
                           var_terms as _var_terms)

SIZES = (1, 63, 257, 2049)                                       # straddle one workgroup of BLOCK = 256 lanes
SHAPES = [(1, 1, 1, 16), (1, 1, 1, 18), (1, 2, 64, 12), (3, 2, 5, 8), (8, 3, 5, 12), (2, 64, 64, 8)]   # (v, t, m, bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def folds(oracle):
    """(v, t, m) -> the case at the largest n with the oracle's fixed sums and variable terms, made once."""
    made = {}

    def get(v, t, m):
        if (v, t, m) not in made:
            n = SIZES[-1]
            bases, idx, fk, pts, vk = _case(oracle, v, t, m, n)
            made[(v, t, m)] = (bases, idx, fk, pts, vk, Fold(oracle, bases).records(idx, fk), _var_terms(oracle, pts, vk, n, v))
        return made[(v, t, m)]
    return get


@pytest.mark.parametrize("v,t,m,bits", SHAPES)
def test_every_shape_and_size_against_the_oracle(ctx, oracle, folds, v, t, m, bits):
    bases, idx, fk, pts, vk, fixed, terms = folds(v, t, m)
    want_enc, want_el = _join(oracle, fixed, terms)
    assert not want_enc[CANCEL].any()
    with ctx.fixed_bases(bases, comb_bits=bits) as fb:
        for n in SIZES:
            enc, el = fb.msm_mixed(idx[:n], fk[:n * t], pts[:n * v], vk[:n * v], elements=True)
            assert enc.shape == (n, 32) and el.shape == (n, 16)
            assert (enc == want_enc[:n]).all(), (n, np.nonzero((enc != want_enc[:n]).any(1))[0][:8])
            assert oracle.eq_xyzt(el, want_el[:n]).all(), n
            assert (oracle.compress(el) == enc).all(), n
            if n > CANCEL:
                assert not enc[CANCEL].any() and oracle.is_identity(el[CANCEL:CANCEL + 1]).all(), n
                assert (enc[ABSENT] == oracle.compress(_join(oracle, np.tile(oracle.identity_xyzt(), (1, 1)),
                                                             terms[ABSENT:ABSENT + 1])[1])[0]).all()
                assert (enc[VZERO] == oracle.compress(np.ascontiguousarray(fixed[VZERO:VZERO + 1]))[0]).all()
        enc3 = fb.msm_mixed(idx[:63].astype(np.int64), fk[:63 * t].reshape(63, t, 32), pts[:63 * v].reshape(63, v, 16),
                            vk[:63 * v].reshape(63, v, 32))      # int64 rows, [n, t, 32] / [n, v, .] arrays
        assert (enc3 == want_enc[:63]).all()


def test_encoded_points_every_fifth_invalid(ctx, oracle, folds):
    v, t, m, bits = 3, 2, 5, 8
    bases, idx, fk, pts, vk, fixed, terms = folds(v, t, m)
    n = 257
    dead = ~pts[:n * v, 8:12].any(1)
    good = pts[:n * v].copy()
    good[dead] = oracle.identity_xyzt()
    encs = oracle.compress(good)
    bad = np.zeros(n * v, bool)
    bad[::5] = True
    encs[bad] = 0xFF                                             # above q: no canonical Encoding
    live = ~bad.reshape(n, v)
    want_enc, want_el = _join(oracle, fixed[:n], terms[:n], live)
    with ctx.fixed_bases(bases, comb_bits=bits) as fb:
        enc, el, status = fb.msm_mixed(idx[:n], fk[:n * t], encs, vk[:n * v], elements=True)
        assert (status == bad.astype(np.uint8)).all()
        assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
        assert oracle.eq_xyzt(el, want_el).all() and (oracle.compress(el) == enc).all()
        enc2, status2 = fb.msm_mixed(idx[:n], fk[:n * t], encs.reshape(n, v, 32), vk[:n * v])
        assert (enc2 == want_enc).all() and (status2 == status).all()


def test_smallest_multi_round_chunk(ctx, oracle):
    """n = 2 CUs 256 + 257 sums: deal_chunks gives two chunks a second round, so their lanes reuse their tables and share an
    inversion across rounds.  Every sum against the oracle."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 256 + 257
    rng = np.random.default_rng(16)
    base = _bases(oracle, rng, 1)
    fk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    vk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (n, 32), dtype=np.uint8)), dtype=np.uint64)
    idx = np.zeros((n, 1), np.int32)
    fixed = Fold(oracle, base).records(idx, fk)
    want = _join(oracle, fixed, _var_terms(oracle, pts, vk, n, 1))[0]
    with ctx.fixed_bases(base, comb_bits=16) as fb:
        enc = fb.msm_mixed(idx, fk, pts, vk)
    assert (enc == want).all(), np.nonzero((enc != want).any(1))[0][:8]


def test_equals_the_composition_of_the_existing_calls(ctx, oracle):
    v, t, m, bits, n = 3, 2, 5, 12, 2049
    bases, idx, fk, pts, vk = _case(oracle, v, t, m, n, seed=7)
    with ctx.fixed_bases(bases, comb_bits=bits) as fb:
        enc = fb.msm_mixed(idx, fk, pts, vk)
        _, var_el = ctx.msm_small(pts, vk, v, elements=True)
        _, fix_el = fb.msm_indexed(idx, fk, elements=True)
        want = ctx.compress(ctx.add(var_el, fix_el))
    assert (enc == want).all(), np.nonzero((enc != want).any(1))[0][:8]


def test_long_handle_with_its_last_base_in_use(ctx, oracle):
    v, t, m, n = 1, 2, 65, 257
    bases, idx, fk, pts, vk = _case(oracle, v, t, m, n)
    idx[:, 0] = 64                                               # past what a short registration holds
    idx[ABSENT, 0] = -1
    want = _join(oracle, Fold(oracle, bases).records(idx, fk), _var_terms(oracle, pts, vk, n, v))[0]
    with ctx.fixed_bases_long(bases, comb_bits=8) as fb:
        enc = fb.msm_mixed(idx, fk, pts, vk)
    assert (enc == want).all(), np.nonzero((enc != want).any(1))[0][:8]


def test_device_listed_twice_slices_sums_status_and_elements(oracle, folds):
    import decaf377_amd as d
    v, t, m, bits = 3, 2, 5, 8
    bases, idx, fk, pts, vk, fixed, terms = folds(v, t, m)
    n = 515
    good = pts[:n * v].copy()
    good[~good[:, 8:12].any(1)] = oracle.identity_xyzt()
    encs = oracle.compress(good)
    bad = np.zeros(n * v, bool)
    bad[3::7] = True
    encs[bad] = 0xFF
    want_enc, want_el = _join(oracle, fixed[:n], terms[:n], ~bad.reshape(n, v))
    c = d.Context([0, 0], comb_lazy=True)
    try:
        with c.fixed_bases(bases, comb_bits=bits) as fb:
            enc, el, status = fb.msm_mixed(idx[:n], fk[:n * t], encs, vk[:n * v], elements=True)
            enc_e, el_e = fb.msm_mixed(idx[:n], fk[:n * t], pts[:n * v], vk[:n * v], elements=True)
        assert (status == bad.astype(np.uint8)).all()
        assert (enc == want_enc).all(), np.nonzero((enc != want_enc).any(1))[0][:8]
        assert oracle.eq_xyzt(el, want_el).all()
        full_enc, full_el = _join(oracle, fixed[:n], terms[:n])
        assert (enc_e == full_enc).all() and oracle.eq_xyzt(el_e, full_el).all()
        for dev in (0, 1):
            assert c.health(dev)[0] == 0 and c.health(dev)[2] == 0
    finally:
        c.close()


def test_refusals_on_a_live_context(ctx, oracle):
    import decaf377_amd as d
    v, t, m, n = 2, 2, 3, 1000
    bases, idx, fk, pts, vk = _case(oracle, v, t, m, n)
    idx[idx < 0] = 0
    pos = 2 * 777 + 1
    idx[777, 1] = 3
    idx[900, 0] = -2                                             # a later one: the FIRST offending position is named
    fb = ctx.fixed_bases(bases, comb_bits=8)
    with pytest.raises(d.NativeError) as e:
        fb.msm_mixed(idx, fk, pts, vk)
    assert "base_index" in str(e.value) and "[%d]" % pos in str(e.value)
    enc = np.full((n, 32), 0x5A, np.uint8)
    el = np.full((n, 16), 0x5A5A5A5A5A5A5A5A, np.uint64)
    st = np.full((n * v,), 0x5A, np.uint8)
    lib = ctx._lib
    assert lib.d377_batch_msm_mixed(ctx._h, fb._h, _p(idx), _p(fk), t, _p(pts), _p(vk), v, n, _p(enc), _p(el)) == -2
    msg = lib.d377_last_error().decode()
    assert "base_index" in msg and "[%d]" % pos in msg
    encs = np.zeros((n * v, 32), np.uint8)
    assert lib.d377_batch_msm_mixed_encoded(ctx._h, fb._h, _p(idx), _p(fk), t, _p(encs), _p(vk), v, n, _p(enc), _p(el), _p(st)) == -2
    assert (enc == 0x5A).all() and (el == 0x5A5A5A5A5A5A5A5A).all() and (st == 0x5A).all()
    idx[777, 1] = idx[900, 0] = -1                               # mended: the call goes through
    assert fb.msm_mixed(idx, fk, pts, vk).shape == (n, 32)
    assert lib.d377_batch_msm_mixed(ctx._h, fb._h, None, None, t, None, None, v, 0, None, None) == 0     # n = 0: D377_OK
    handle = fb._h
    fb.close()                                                   # a destroyed handle is refused
    assert lib.d377_batch_msm_mixed(ctx._h, handle, _p(idx), _p(fk), t, _p(pts), _p(vk), v, n, _p(enc), _p(el)) == -2
    assert "handle" in lib.d377_last_error().decode()
    assert (enc == 0x5A).all()
    with pytest.raises(d.NativeError):
        fb.msm_mixed(idx, fk, pts, vk)


def test_torch_staging(ctx, oracle, folds):
    import torch
    v, t, m, bits = 3, 2, 5, 8
    bases, idx, fk, pts, vk, fixed, terms = folds(v, t, m)
    n = 63
    want = _join(oracle, fixed[:n], terms[:n])[0]
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    with ctx.fixed_bases(bases, comb_bits=bits) as fb:
        enc, el = fb.msm_mixed(dev(idx[:n]), dev(fk[:n * t]), dev(pts[:n * v].view(np.int64)), dev(vk[:n * v]), elements=True)
    assert str(enc.device) == "cuda:0" and str(el.device) == "cuda:0"
    assert (enc.cpu().numpy() == want).all()
    assert (oracle.compress(el.cpu().numpy().view(np.uint64)) == want).all()


def test_health_afterwards(ctx):
    claimed, _, gave_up = ctx.health()
    assert claimed == 0 and gave_up == 0


def test_cpp_mirror_msm_mixed():
    build_and_run_cpp("msm_mixed", "CPP_MSM_MIXED_OK")
