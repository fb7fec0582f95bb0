"""CPU check of the signed-limb field type (decaf377_amd/csrc/fqs29.hpp) and of the variable-base chain on it.

tests/host_sim/signed_sim.cpp (sim.cpp plus the signed chain) is compiled for the host with g++; its products are the
statements the signed instruction streams of fe_asm.inc compute (tools/gen_fe_asm.py), checked here against a Python
model of the stream (every partial column sum) and against big-integer arithmetic.  The chain on fes must give the
encodings of the chain on fe, and the -DD377_BOUNDS build walks it with every precondition asserted."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383
NL, RB, MASK = 9, 29, (1 << 29) - 1
QL = [(Q >> (RB * i)) & MASK if i < NL - 1 else Q >> (RB * (NL - 1)) for i in range(NL)]
R_INV = pow(1 << 261, -1, Q)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _build(name, flags):
    lib = os.path.join(SIM_DIR, name)
    srcs = [os.path.join(SIM_DIR, "signed_sim.cpp"), os.path.join(SIM_DIR, "sim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC] + flags +
                              [os.path.join(SIM_DIR, "signed_sim.cpp"), "-o", lib])
    return lib


@pytest.fixture(scope="module")
def ssim():
    L = ctypes.CDLL(_build("libd377_signed_sim.so", ["-O2", "-DD377_FB_BITS=12"]))
    L.sim_init.restype = ctypes.c_int
    assert L.sim_init() == 0
    return L


def _value(limbs):
    return sum(int(v) << (RB * i) for i, v in enumerate(limbs))


def _stream(a, b, kind):
    """The signed stream of tools/gen_fe_asm.py in Python: (result limbs, largest |partial column sum|)."""
    a2 = [2 * x for x in a]
    if kind == "mul":
        terms = lambda k: [a[i] * b[k - i] for i in range(NL) if 0 <= k - i < NL]
    elif kind == "sqr":
        terms = lambda k: [a2[i] * a[k - i] for i in range(NL) if 0 <= k - i < NL and 2 * i < k] + \
            ([a[k // 2] * a[k // 2]] if k % 2 == 0 else [])
    else:
        terms = lambda k: [a2[i] * a2[k - i] for i in range(NL) if 0 <= k - i < NL and 2 * i < k] + \
            ([a2[k // 2] * a[k // 2]] if k % 2 == 0 else [])
    acc, worst, m, r = 0, 0, [0] * NL, [0] * NL
    for k in range(2 * NL - 1):
        for t in terms(k) + [-m[i] * QL[k - i] for i in range(max(0, k - NL + 1), min(k, NL))]:
            acc += t
            worst = max(worst, abs(acc))
        if k < NL:
            m[k] = acc & MASK
        else:
            r[k - NL] = acc & MASK
        acc >>= RB                       # Python's >> on a negative int is the arithmetic shift
    r[NL - 1] = acc
    return r, worst


def test_q2l(ssim):
    q2 = np.zeros(9, np.uint32)
    ssim.sims_consts(_p(q2))
    assert _value(q2) == 2 * Q and all(int(v) <= MASK for v in q2[:8])


def test_generator_signed_kinds():
    """The signed kinds are 187 / 159 / 160 instructions for 153 / 117 / 117 MACs and their bodies are in fe_asm.inc."""
    spec = importlib.util.spec_from_file_location("gen_fe_asm", os.path.join(ROOT, "tools", "gen_fe_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = open(os.path.join(CSRC, "fe_asm.inc")).read()
    for kind, (n, nmac) in {"smul": (187, 153), "ssqr": (159, 117), "ssqr2x": (160, 117)}.items():
        body, got_mac, got_n, _ = g.gen(kind, False)
        assert (got_n, got_mac) == (n, nmac)
        assert '#define D377_ASM_%s "%s"' % (kind.upper(), body) in text
        assert body.count("v_mad_i64_i32") == nmac and "v_mad_u64_u32" not in body
        assert body.count("v_ashrrev_i64") == 2 * NL - 1 and body.count("v_and_b32") == 2 * NL - 1


def _operands(rng, n, wide):
    """n operand rows: random limbs up to +-wide (the top limb up to +-2^21), then extreme mixes."""
    top = 1 << 21
    rows = [[int(x) for x in rng.integers(-wide, wide + 1, NL - 1)] + [int(rng.integers(-top, top + 1))] for _ in range(n)]
    ext = [-wide, wide, 0, -1, MASK, -4, MASK + 8]
    for i in range(len(ext) ** 2):
        rows.append([ext[(i + j) % len(ext)] if j % 2 else ext[i // len(ext)] for j in range(NL - 1)] +
                    [[-top, top, 0][i % 3]])
    return rows


def _product_rows(kind):
    """The operand rows of test_signed_products (tests/test_field_streams.py runs the same rows on the GPU): 600 seeded rows
    and the 49 extreme mixes, at the widths the kind's contract allows."""
    rng = np.random.default_rng({"mul": 1, "sqr": 2, "sqr2x": 3}[kind])
    lazy = (1 << 30) + (1 << 29) + 16            # a wide (lazy) operand times a carried one; a square of limbs below
    carried = (1 << 29) + 8                      # 2^30 - 2^27 (a sum of two products); twice the square of a carried one
    a_rows = _operands(rng, 600, {"mul": lazy, "sqr": (1 << 30) - (1 << 27), "sqr2x": carried}[kind])
    b_rows = _operands(rng, len(a_rows), carried)
    rng.shuffle(b_rows)
    return a_rows, b_rows


@pytest.mark.parametrize("kind", ["mul", "sqr", "sqr2x"])
def test_signed_products(ssim, kind):
    """Signed products at the contract's extreme limbs: exactly the stream's result, congruent to (s) a b / R, limbs 0..7
    in [0, 2^29), value in (s a b / R - q, s a b / R], every partial column sum inside +-2^63."""
    a_rows, b_rows = _product_rows(kind)
    a = np.array(a_rows, np.int32)
    b = np.array(b_rows, np.int32)
    r = np.zeros_like(a)
    ssim.sims_field_op({"mul": 0, "sqr": 1, "sqr2x": 2}[kind], _p(a), _p(b), ctypes.c_size_t(len(a)), _p(r))
    scale = 2 if kind == "sqr2x" else 1
    for x, y, z in zip(a_rows, b_rows, r.tolist()):
        want, worst = _stream(x, y, kind)
        assert worst < 1 << 63
        assert z == want
        va, vb = _value(x), _value(y) if kind == "mul" else _value(x)
        t, v = scale * va * vb, _value(z)
        assert (v - t * R_INV) % Q == 0
        assert all(0 <= l <= MASK for l in z[:8])
        assert t - Q * (1 << 261) < v * (1 << 261) <= t


def _linear_rows():
    """The rows of test_signed_linear_and_conversion: (a, b) for fe_sub and fe_carry, p for fes -> fe."""
    rng = np.random.default_rng(4)
    n = 400
    a = rng.integers(-(1 << 30), 1 << 30, (n, 9)).astype(np.int32)
    b = rng.integers(-(1 << 30), 1 << 30, (n, 9)).astype(np.int32)
    # a product-form input (limbs 0..7 in [0, 2^29), signed top), value above -2q + 2^233
    p = rng.integers(0, 1 << 29, (n, 9)).astype(np.int32)
    p[:, 8] = rng.integers(-2 * QL[8] + 2, 1 << 19, n)
    p[0, :8], p[0, 8] = 0, -(2 * QL[8]) + 2
    return a, b, p


def test_signed_linear_and_conversion(ssim):
    """fe_sub without offset, the arithmetic-shift carry pass (value kept) and fes -> fe (+2q, carried, same residue)."""
    a, b, p = _linear_rows()
    n = len(a)
    r = np.zeros_like(a)
    ssim.sims_field_op(4, _p(a), _p(b), ctypes.c_size_t(n), _p(r))
    assert (r.astype(np.int64) == a.astype(np.int64) - b).all()
    ssim.sims_field_op(3, _p(a), _p(b), ctypes.c_size_t(n), _p(r))
    for x, z in zip(a.tolist(), r.tolist()):
        assert _value(z) == _value(x) and all(-2 <= l < (1 << 29) + 2 for l in z[:8])
    ssim.sims_field_op(5, _p(p), _p(b), ctypes.c_size_t(n), _p(r))
    for x, z in zip(p.tolist(), r.astype(np.uint32).tolist()):
        assert _value(z) == _value(x) + 2 * Q and all(l < (1 << 29) + 8 for l in z[:8])


def _h_to_k(h):
    return (2 * h) % R_ORDER                     # the kernel runs its window loop on k/2 mod r


def _scalar_rows(rng, n):
    special = [0, 1, 2, R_ORDER - 1, R_ORDER - 2, (R_ORDER + 1) // 2, (R_ORDER - 1) // 2,
               _h_to_k(16 ** 62 - 8 * (16 ** 62 - 1) // 15),       # window digits -8 (62 of them)
               _h_to_k(7 * (16 ** 62 - 1) // 15),                    # window digits 7
               16 ** 62 - 8 * (16 ** 62 - 1) // 15]                  # digits -8 for the chain that does not halve
    ks = [int.from_bytes(rng.bytes(32), "little") for _ in range(n - len(special))] + special
    return np.array([list(k.to_bytes(32, "little")) for k in ks], np.uint8)


def test_signed_chain_matches_unsigned(ssim, oracle):
    """The window loop on fes (k_scalar_mul_var's and k_scalar_mul_var_el's chain) gives the encodings the chain on fe
    gives: random points and scalars, special scalars, the identity and invalid encodings."""
    rng = np.random.default_rng(377)
    n = 48
    k = _scalar_rows(rng, n)
    enc = oracle.encode_to_curve(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    enc[0] = 0                                           # the identity
    enc[1] = 0xFF                                        # not a field element
    enc[2, 0] |= 1                                       # a negative s
    enc[3] = enc[4]
    enc[3, 5] ^= 0x40                                    # (almost surely) not on the curve
    k[5:15] = k[n - 10:]
    outs = []
    for f in ("sim_scalar_mul_var", "sims_scalar_mul_var", "sim_scalar_mul_var_sqrt", "sims_scalar_mul_var_sqrt"):
        out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        getattr(ssim, f)(_p(enc), _p(k), ctypes.c_size_t(n), _p(out), _p(st))
        outs.append((out, st))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()
    assert (outs[2][0] == outs[3][0]).all() and (outs[2][1] == outs[3][1]).all()
    oo, so = oracle.scalar_mul_var(enc, k)
    assert (outs[1][0] == oo).all() and (outs[1][1] == so).all()
    assert outs[1][1][1] != 0 and outs[1][1][0] == 0


def test_signed_chain_bounds():
    """The -DD377_BOUNDS build walks the headline element (decompress, [k]P with the signed window loop, compress, in
    rounds of a lane's 32 elements) with every precondition asserted, and counts bench.py's field products."""
    lib = _build("libd377_signed_sim_bounds.so", ["-O0", "-g", "-DD377_BOUNDS", "-DD377_FB_BITS=8"])
    code = r"""
import ctypes, sys, numpy as np
L = ctypes.CDLL(sys.argv[1]); L.sim_init.restype = ctypes.c_int; assert L.sim_init() == 0
p = lambda a: a.ctypes.data_as(ctypes.c_void_p); n_ = ctypes.c_size_t
rng = np.random.default_rng(1)
m = ctypes.c_ulong(); s = ctypes.c_ulong()
n = 32
r0 = rng.integers(0, 256, (n, 32), dtype=np.uint8); k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
enc = np.zeros((n, 32), np.uint8); out = np.zeros((n, 32), np.uint8); st = np.zeros(n, np.uint8)
L.sim_encode_to_curve(p(r0), n_(n), p(enc), None); L.sim_op_counts(ctypes.byref(m), ctypes.byref(s))
L.sims_scalar_mul_var(p(enc), p(k), n_(n), p(out), p(st))
L.sim_op_counts(ctypes.byref(m), ctypes.byref(s)); print(m.value / n, s.value / n)
L.sims_scalar_mul_var_sqrt(p(enc), p(k), n_(4), p(out), p(st))
"""
    res = subprocess.run([sys.executable, "-c", code, lib], capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, res.stderr[-3000:]
    spec = importlib.util.spec_from_file_location("bench_for_counts", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    mul, sqr = map(float, res.stdout.split()[:2])
    assert (mul, sqr) == bench.KERNEL_OPS["scalar_mul_var"]
