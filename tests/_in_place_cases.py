"""The in-place contract of include/decaf377_amd.h as a table, the routes every operation of the table has, and inputs that
make a late read show.  Shared by tests/test_in_place_host.py (the table against the header, the route plan against
launch_plan.hpp at 256 CUs) and tests/test_in_place_gpu.py (every row, alias, route and size on device buffers).

The header: "An output buffer may be the input buffer of the same record size (in place); until a call completes its output
records may hold intermediate values."  TABLE restates, from the prototypes, every d377_batch_*_dev export in which an output
record has the size of an input record, and which inputs that output may alias."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 13356249993388743167 | 5950279507993463550 << 64 | 10965441865914903552 << 128 | 336320092672043349 << 192

# export -> (the output parameter, the input parameters it may alias), by the parameter names of the header's prototypes
TABLE = {
    # 32 bytes -> 32 bytes
    "d377_batch_sqrt_ratio_zeta_dev": ("root32", ("num32", "den32")),
    "d377_batch_sqrt_ratio_zeta_ex_dev": ("root32", ("num32", "den32")),
    "d377_batch_roundtrip_dev": ("enc32_out", ("enc32",)),
    "d377_batch_scalar_mul_base_dev": ("enc32_out", ("scalar32",)),
    "d377_batch_scalar_mul_var_dev": ("enc32_out", ("enc32", "scalar32")),
    "d377_batch_encode_to_curve_dev": ("enc32_out", ("fq32",)),
    "d377_batch_hash_to_curve_dev": ("enc32_out", ("r1_32", "r2_32")),
    "d377_batch_fq_op_dev": ("out", ("a", "b")),
    "d377_batch_fq_from_bytes_checked_dev": ("out", ("bytes32",)),
    "d377_batch_fq_to_bytes_dev": ("bytes32", ("a",)),
    "d377_batch_fr_from_le_bytes_mod_order_dev": ("fr32_out", ("bytes32",)),
    "d377_batch_fr_from_bytes_checked_dev": ("fr32_out", ("bytes32",)),
    "d377_batch_fr_op_dev": ("out32", ("a32", "b32")),
    # 128 bytes -> 128 bytes
    "d377_batch_add_dev": ("out_xyzt", ("p_xyzt", "q_xyzt")),
    "d377_batch_sub_dev": ("out_xyzt", ("p_xyzt", "q_xyzt")),
    "d377_batch_double_dev": ("out_xyzt", ("p_xyzt",)),
    "d377_batch_neg_dev": ("out_xyzt", ("p_xyzt",)),
    "d377_batch_scalar_mul_var_element_dev": ("out_xyzt", ("p_xyzt",)),
}
# The operations d377_batch_sharded_dev takes whose export is in TABLE (decompress, compress and scalar_mul_base_element change
# the record size): SHARD_OPS name -> the export whose buffers it takes
SHARDED = {"sqrt_ratio_zeta": "d377_batch_sqrt_ratio_zeta_dev", "roundtrip": "d377_batch_roundtrip_dev",
           "scalar_mul_base": "d377_batch_scalar_mul_base_dev", "scalar_mul_var": "d377_batch_scalar_mul_var_dev",
           "encode_to_curve": "d377_batch_encode_to_curve_dev", "hash_to_curve": "d377_batch_hash_to_curve_dev",
           "scalar_mul_var_element": "d377_batch_scalar_mul_var_element_dev"}

FIELD_OPS = ("add", "sub", "mul", "square", "neg", "inverse")        # the D377_FQ_* selectors 0 .. 5; the first three are binary

# ---- sizes ----------------------------------------------------------------------------------------------------------------------
WAVE_N = (1, 2, 3, 5, 17, 63, 65, 257)        # wave, quad, four- and pair-per-wave routes: odd n, n mod 4 != 0, n mod 16 != 0 -> clamped idle lanes
LANE_N = (1, 255, 257, 1000)                  # lane-set and fixed-base routes, the default deal
CHUNK_K = (2, 3, 8)                           # ... and chunk_per_lane k at n = 2 k 256 + 77: two full chunks and a ragged third
PLAIN_N = (1, 63, 257, 1000)                  # the plain grid (and the wide grid, the same grid rule)
INVERSE_N = PLAIN_N + (65,)                   # k_fq_inv: a partial wave inside the shared inversion
FB_K = (1, 8, 16)


def chunk_n(k):
    return 2 * k * 256 + 77


def resident_lanes(cus):
    return cus * 2 * 256


def _lane_cases(route, base):
    for n in LANE_N:
        yield route, dict(base), n
    for k in CHUNK_K:
        yield route, dict(base, chunk_per_lane=k), chunk_n(k)


def route_cases(family, cus):
    """(route of launch_plan.hpp, the tuning that forces it, n) for every route an operation of `family` has."""
    if family in ("sqrt", "encode"):
        for n in WAVE_N:
            yield "four_per_wave", {}, n
        yield from _lane_cases("lane_sets", dict(tiny_max=0))
    elif family == "hash":
        for n in WAVE_N:
            yield "pair_per_wave", {}, n
        for n in WAVE_N:
            # four per wave is 2 tiny_max < n <= 4 tiny_max (below, two pairs per wave): no tiny_max gives it to n = 1 or 2
            if 2 * -(-n // 4) < n:
                yield "four_per_wave", dict(tiny_max=-(-n // 4)), n
        yield from _lane_cases("lane_sets", dict(tiny_max=0))
    elif family == "roundtrip":
        for n in WAVE_N:
            yield "four_per_wave", {}, n
        for n in PLAIN_N:
            yield "wide_grid", dict(tiny_max=0), n
        # The launcher falls back from the chunked kernels to the wide grid when their residency does not match the lane sets
        # (codec_chunked_ok: device state, an occupancy query).  Nothing outside the library can observe which of the two ran;
        # the plan says codec_chunked and both give the same bytes.
        yield from _lane_cases("codec_chunked", dict(decompress_chunked_min=1, tiny_max=0))
    elif family == "mul_var":
        for n in WAVE_N:
            yield "wave_per_element", {}, n
        for n in WAVE_N:
            yield "quad_per_element", dict(tiny_max=0), n
        yield from _lane_cases("lane_sets", dict(small_max=0))
    elif family == "mul_base":
        for n in WAVE_N:
            yield "wave_per_element", {}, n
        for n in WAVE_N:
            yield "quad_per_element", dict(tiny_max=0), n
        for wide in (0, 1):
            for fk in FB_K:
                yield from _lane_cases("fb_wide" if wide else "fb_narrow", dict(small_max=0, fb_wide=wide, fb_k=fk))
    elif family == "mul_var_el":
        for n in WAVE_N:
            yield "wave_per_element", {}, n
        for n in WAVE_N:
            yield "quad_per_element", dict(tiny_max=0), n
        for n in LANE_N:
            yield "el_uniform", dict(small_max=0), n                  # one element per lane: n <= the resident lanes
        yield "el_uniform", dict(small_max=0), resident_lanes(cus) + 257     # two per lane
    elif family == "inverse":
        for n in INVERSE_N:
            yield "plain", {}, n
    else:
        assert family == "plain", family
        for n in PLAIN_N:
            yield "plain", {}, n


def el_per_lane(n, cus):
    """k_scalar_mul_var_el's uniform chunks: two elements per lane beyond the resident lanes."""
    return 2 if n > resident_lanes(cus) else 1


# ---- the plan, asked of the host build of launch_plan.hpp (tests/host_sim: sim_launch_plan) ----------------------------------------
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")))
PLAN_OPS, PLAN_ROUTES, PLAN_OUT = GOLDEN["ops"], GOLDEN["routes"], GOLDEN["out_fields"]
PLAN_TUNE = GOLDEN["in_fields"][4:]


def plan_lib():
    """The host build of launch_plan.hpp alone (tests/host_sim/launch_plan_sim.cpp: the plan exports of sim.cpp, which build
    in a second): what a test next to a GPU run asks.  tests/test_in_place_host.py holds it against the whole host build."""
    import ctypes
    import subprocess
    sim_dir, csrc = os.path.join(ROOT, "tests", "host_sim"), os.path.join(ROOT, "decaf377_amd", "csrc")
    lib = os.path.join(sim_dir, "liblaunch_plan_sim.so")
    srcs = [os.path.join(sim_dir, f) for f in ("launch_plan_sim.cpp", "launch_plan_sim.inc")] + [os.path.join(csrc, "launch_plan.hpp")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        tmp = "%s.%d" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, srcs[0], "-o", tmp])
        os.replace(tmp, lib)
    return ctypes.CDLL(lib)


def planned(sim, plan_op, n, cus, tuning):
    """The plan of one call as a dict of launch_plan_parent.json's out_fields, `route` by name; sim: either host build."""
    import ctypes
    vec = [tuning.get(k, -1) for k in PLAN_TUNE]
    assert set(tuning) <= set(PLAN_TUNE), tuning
    out = np.zeros(len(PLAN_OUT), np.int64)
    arg = np.array([PLAN_OPS.index(plan_op), 0, n, cus] + vec, np.int64)
    sim.sim_launch_plan(arg.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    f = dict(zip(PLAN_OUT, (int(v) for v in out)))
    f["route"] = PLAN_ROUTES[f["route"]]
    return f


# ---- the operations -------------------------------------------------------------------------------------------------------------
class Op:
    """One way to drive an export of TABLE.  ins: the kinds of its inputs ("bytes": [n, 32] u8, "fq": [n, 4] u64 Montgomery
    records, "el": [n, 16] u64 Elements); out: the kind of out0; alias: the inputs out0 may be; call(ctx, ins, outs) -> the
    engine's result; want(oracle, *ins) -> (out0, status or None); pool(oracle, rng, u) -> u rows of every input, the
    adversarial ones first."""

    def __init__(self, key, export, plan_op, family, ins, out, alias, call, want, pool, status, both=False, unique=1024,
                 as_elements=False):
        self.key, self.export, self.plan_op, self.family, self.ins, self.out, self.alias = key, export, plan_op, family, ins, out, alias
        self.call, self.want, self.pool, self.status, self.both, self.unique, self.as_elements = call, want, pool, status, both, unique, as_elements
        names = TABLE[export][1]
        assert len(alias) == len(names) or (len(ins) < 2 and len(alias) == 1), key     # (the unary codes of fq_op / fr_op have no b)


def ibytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _rows(rng, u):
    return rng.integers(0, 256, (u, 32), dtype=np.uint8)


def _put(cols, specials):
    """Writes the tuples of `specials` over the first rows of the input columns -> how many."""
    for j, tup in enumerate(specials):
        for col, v in zip(cols, tup):
            col[j] = v
    return len(specials)


def pool_field_bytes(oracle, rng, u, two):
    """Byte strings read as Fq (reduced mod q): square-root operands, Elligator inputs."""
    a, b = _rows(rng, u), _rows(rng, u)
    e = [ibytes(v) for v in (0, 1, Q - 1, Q, (1 << 256) - 1)]
    sp = [(a[9], b[9]), (e[0], b[1]), (a[2], e[0]), (e[0], e[0]), (e[2], e[2]), (e[3], b[5]), (a[6], e[4]), (e[1], e[2]), (e[4], e[3])]
    if two == "hash":                                  # ... and the pairs that meet the exceptional case of the quartic's addition law
        pairs = json.load(open(os.path.join(ROOT, "tests", "golden", "hash_exceptional_pairs.json")))["pairs"]
        for p in pairs:
            r1, r2 = (np.frombuffer(bytes.fromhex(p[k]), np.uint8) for k in ("r1", "r2"))
            sp += [(r1, r2), (r2, r1)]
    ns = _put((a, b), [(x.copy(), y.copy()) for x, y in sp])
    return ([a, b] if two else [a]), ns


def pool_encodings(oracle, rng, u):
    enc = oracle.encode_to_curve(_rows(rng, u))
    sp = [enc[20].copy() for _ in range(7)]
    sp[1][31] |= 0x40                                  # top bits set
    sp[2][31] |= 0x80
    sp[3][0] |= 1                                      # negative s
    sp[4] = _rows(rng, 1)[0]                           # a raw string
    sp[5][:] = 0                                       # the all-zero Encoding: the identity
    sp[6] = ibytes(Q - 1)                              # canonical, negative
    return enc, sp


def pool_scalars(rng, u):
    return _rows(rng, u), [ibytes(v) for v in (0, 1, R_ORDER - 1, R_ORDER, (1 << 256) - 1)]


def pool_mul_var(oracle, rng, u):
    enc, es = pool_encodings(oracle, rng, u)
    k, ks = pool_scalars(rng, u)
    # (the adversarial Encodings first: batch_of puts the first specials into every wave)
    sp = [(x, k[30 + j].copy()) for j, x in enumerate(es)] + [(es[0], x) for x in ks] + [(es[5], ks[0]), (es[1], ks[3])]
    return [enc, k], _put((enc, k), sp)


def pool_roundtrip(oracle, rng, u):
    enc, es = pool_encodings(oracle, rng, u)
    return [enc], _put((enc,), [(x,) for x in es])


def pool_mul_base(oracle, rng, u):
    k, ks = pool_scalars(rng, u)
    return [k], _put((k,), [(k[40].copy(),)] + [(x,) for x in ks])


def pool_checked(oracle, rng, u):
    """Byte strings for the checked conversions: canonical ones, and values >= q and >= r."""
    a = _rows(rng, u)
    a[:, 31] &= np.where(rng.integers(0, 2, u) == 1, 0x0F, 0xFF).astype(np.uint8)      # about half below both moduli
    sp = [ibytes(v) for v in (5, 0, R_ORDER - 1, R_ORDER, R_ORDER + 1, Q - 1, Q, Q + 1, (1 << 256) - 1, 1 << 255)]
    return [a], _put((a,), [(x,) for x in sp])


def pool_fr(oracle, rng, u, two):
    a, b = _rows(rng, u), _rows(rng, u)
    e = [ibytes(v) for v in (0, 1, R_ORDER - 1, R_ORDER, (1 << 256) - 1)]
    sp = [(a[9], b[9]), (e[0], b[1]), (a[2], e[0]), (e[0], e[0]), (e[2], e[2]), (e[3], b[5]), (a[6], e[4]), (e[1], e[2]), (e[4], e[3])]
    ns = _put((a, b), [(x.copy(), y.copy()) for x, y in sp])
    return ([a, b] if two else [a]), ns


def pool_fq(oracle, rng, u, two):
    """Fq records: 0 (the inverse's status) and q - 1 among random ones."""
    a, b = (oracle.fq_from_bytes_mod_order(_rows(rng, u)) for _ in range(2))
    e = [oracle.fq_from_bytes_mod_order(ibytes(v).reshape(1, 32))[0] for v in (0, Q - 1, 1)]
    sp = [(a[9], b[9]), (e[0], b[1]), (a[2], e[0]), (e[0], e[0]), (e[1], e[1]), (e[1], b[5]), (a[6], e[1]), (e[2], e[1]), (e[0], e[1])]
    ns = _put((a, b), [(x.copy(), y.copy()) for x, y in sp])
    return ([a, b] if two else [a]), ns


def pool_elements(oracle, rng, u, two, scalars=False):
    """Elements: the identity, the generator, Z != 1 (everything the Elligator map and a doubling give)."""
    p = oracle.elligator_map_xyzt(_rows(rng, u))
    q = oracle.double_xyzt(oracle.elligator_map_xyzt(_rows(rng, u)))
    ident, gen = oracle.identity_xyzt(), oracle.generator_xyzt()
    ident2 = oracle.add_xyzt(p[3:4], oracle.neg_xyzt(p[3:4]))[0]       # the identity with Z != 1
    if scalars:
        k, ks = pool_scalars(rng, u)
        sp = [(p[9], x) for x in ks] + [(ident, k[31]), (gen, k[32]), (ident2, k[33]), (gen, ks[2]), (ident, ks[0]), (q[7], k[34])]
        return [p, k], _put((p, k), [(x.copy(), y.copy()) for x, y in sp])
    sp = [(p[9], q[9]), (ident, q[1]), (p[2], ident), (ident, ident), (gen, gen), (gen, q[5]), (p[6], oracle.neg_xyzt(p[6:7])[0]),
          (ident2, gen), (p[8], p[8]), (ident2, ident2)]
    ns = _put((p, q), [(x.copy(), y.copy()) for x, y in sp])
    return ([p, q] if two else [p]), ns


def _checked_fr(oracle, a):
    st = oracle.fr_from_bytes_checked(a)
    out = a.copy()
    out[st != 0] = 0                                   # "the record is copied through when canonical"; a rejected record is all-zero
    return out, st


def _ops():
    ops = []

    def add(*a, **kw):
        ops.append(Op(*a, **kw))

    from decaf377_amd.engine import ENC, FLAG
    # the plain export has no method of its own in the engine (sqrt_ratio_zeta always takes the _ex form)
    add("sqrt_ratio_zeta", "d377_batch_sqrt_ratio_zeta_dev", "sqrt", "sqrt", ("bytes", "bytes"), "bytes", (0, 1),
        lambda c, i, o: c._run("d377_batch_sqrt_ratio_zeta", i, [ENC, ENC], [ENC, FLAG], o),
        lambda orc, a, b: orc.sqrt_ratio_zeta(a, b), lambda orc, rng, u: pool_field_bytes(orc, rng, u, True), True, both=True)
    for root, fn in (("ark", "sqrt_ratio_zeta"), ("min_curve", "sqrt_ratio_zeta_min_curve")):
        add("sqrt_ratio_zeta_ex:" + root, "d377_batch_sqrt_ratio_zeta_ex_dev", "sqrt", "sqrt", ("bytes", "bytes"), "bytes", (0, 1),
            lambda c, i, o, root=root: c.sqrt_ratio_zeta(i[0], i[1], outs=o, root=root),
            lambda orc, a, b, fn=fn: getattr(orc, fn)(a, b), lambda orc, rng, u: pool_field_bytes(orc, rng, u, True), True, both=True)
    add("roundtrip", "d377_batch_roundtrip_dev", "roundtrip", "roundtrip", ("bytes",), "bytes", (0,),
        lambda c, i, o: c.roundtrip(i[0], outs=o), lambda orc, a: orc.roundtrip(a), pool_roundtrip, True)
    add("scalar_mul_base", "d377_batch_scalar_mul_base_dev", "mul_base", "mul_base", ("bytes",), "bytes", (0,),
        lambda c, i, o: c.scalar_mul_base(i[0], outs=o), lambda orc, k: (orc.scalar_mul_base(k), None), pool_mul_base, False)
    add("scalar_mul_var", "d377_batch_scalar_mul_var_dev", "mul_var", "mul_var", ("bytes", "bytes"), "bytes", (0, 1),
        lambda c, i, o: c.scalar_mul_var(i[0], i[1], outs=o), lambda orc, e, k: orc.scalar_mul_var(e, k), pool_mul_var, True)
    add("encode_to_curve", "d377_batch_encode_to_curve_dev", "encode", "encode", ("bytes",), "bytes", (0,),
        lambda c, i, o: c.encode_to_curve(i[0], outs=o), lambda orc, r: (orc.encode_to_curve(r), None),
        lambda orc, rng, u: pool_field_bytes(orc, rng, u, False), False)
    add("hash_to_curve", "d377_batch_hash_to_curve_dev", "hash", "hash", ("bytes", "bytes"), "bytes", (0, 1),
        lambda c, i, o: c.hash_to_curve(i[0], i[1], outs=o), lambda orc, a, b: (orc.hash_to_curve(a, b), None),
        lambda orc, rng, u: pool_field_bytes(orc, rng, u, "hash"), False, both=True)
    for code, name in enumerate(FIELD_OPS):
        two = code <= 2
        add("fq_op:" + name, "d377_batch_fq_op_dev", "fq_bin" if two else "fq_un", "inverse" if name == "inverse" else "plain",
            ("fq", "fq") if two else ("fq",), "fq", (0, 1) if two else (0,),
            lambda c, i, o, name=name: c.fq_op(name, *i, outs=o),
            lambda orc, *i, code=code: orc.fq_op(code, *i), lambda orc, rng, u, two=two: pool_fq(orc, rng, u, two), True, both=two)
        add("fr_op:" + name, "d377_batch_fr_op_dev", "fr_bin" if two else "fr_un", "plain",
            ("bytes", "bytes") if two else ("bytes",), "bytes", (0, 1) if two else (0,),
            lambda c, i, o, name=name: c.fr_op(name, *i, outs=o),
            lambda orc, *i, code=code: orc.fr_op(code, *i), lambda orc, rng, u, two=two: pool_fr(orc, rng, u, two), True, both=two,
            unique=256 if name == "inverse" else 1024)                  # (the oracle's Fr inversion takes a millisecond)
    add("fq_from_bytes_checked", "d377_batch_fq_from_bytes_checked_dev", "fq_checked", "plain", ("bytes",), "fq", (0,),
        lambda c, i, o: c.fq_from_bytes_checked(i[0], outs=o), lambda orc, a: orc.fq_from_bytes_checked(a), pool_checked, True)
    add("fq_to_bytes", "d377_batch_fq_to_bytes_dev", "fq_to_bytes", "plain", ("fq",), "bytes", (0,),
        lambda c, i, o: c.fq_to_bytes(i[0], outs=o), lambda orc, a: (orc.fq_to_bytes(a), None),
        lambda orc, rng, u: pool_fq(orc, rng, u, False), False)
    add("fr_from_le_bytes_mod_order", "d377_batch_fr_from_le_bytes_mod_order_dev", "fr_mod", "plain", ("bytes",), "bytes", (0,),
        lambda c, i, o: c.fr_from_le_bytes_mod_order(i[0], outs=o), lambda orc, a: (orc.fr_from_bytes_mod_order(a), None),
        pool_checked, False)
    add("fr_from_bytes_checked", "d377_batch_fr_from_bytes_checked_dev", "fr_checked", "plain", ("bytes",), "bytes", (0,),
        lambda c, i, o: c.fr_from_bytes_checked(i[0], outs=o), _checked_fr, pool_checked, True)
    add("add", "d377_batch_add_dev", "add", "plain", ("el", "el"), "el", (0, 1), lambda c, i, o: c.add(i[0], i[1], outs=o),
        lambda orc, p, q: (orc.add_xyzt(p, q), None), lambda orc, rng, u: pool_elements(orc, rng, u, True), False, both=True)
    add("sub", "d377_batch_sub_dev", "add", "plain", ("el", "el"), "el", (0, 1), lambda c, i, o: c.sub(i[0], i[1], outs=o),
        lambda orc, p, q: (orc.sub_xyzt(p, q), None), lambda orc, rng, u: pool_elements(orc, rng, u, True), False, both=True)
    add("double", "d377_batch_double_dev", "double", "plain", ("el",), "el", (0,), lambda c, i, o: c.double(i[0], outs=o),
        lambda orc, p: (orc.double_xyzt(p), None), lambda orc, rng, u: pool_elements(orc, rng, u, False), False)
    add("neg", "d377_batch_neg_dev", "neg", "plain", ("el",), "el", (0,), lambda c, i, o: c.neg(i[0], outs=o),
        lambda orc, p: (orc.neg_xyzt(p), None), lambda orc, rng, u: pool_elements(orc, rng, u, False), False)
    # some extended representative of the oracle's element: compared under eq_xyzt and as Encodings
    add("scalar_mul_var_element", "d377_batch_scalar_mul_var_element_dev", "mul_var_el", "mul_var_el", ("el", "bytes"), "el", (0,),
        lambda c, i, o: c.scalar_mul_var_element(i[0], i[1], outs=o), lambda orc, p, k: (orc.scalar_mul_xyzt(p, k), None),
        lambda orc, rng, u: pool_elements(orc, rng, u, True, scalars=True), False, as_elements=True)
    return ops


OPS = _ops()
BY_KEY = {op.key: op for op in OPS}
# every (operation, route) pair the GPU module claims to run
CLAIMED = sorted({(op.key, route) for op in OPS for route, _, _ in route_cases(op.family, 256)})

# ---- inputs ---------------------------------------------------------------------------------------------------------------------
# Where the adversarial records sit: the odd records 1, 3, 5, ... of every wave of 64, up to SPECIAL_SLOTS of them.  The first
# SPECIAL_FIXED adversarial records of a pool are in EVERY wave (and the first eight of them in a batch of 17); a pool that
# has more walks the rest through the remaining slots, wave after wave.  Every pool but hash_to_curve's (9 and the 24
# exceptional pairs) fits a wave whole.
SPECIAL_SLOTS, SPECIAL_FIXED = 24, 16
_pools = {}


def pool_of(op, oracle):
    """(the input columns of `unique` distinct records, how many of them are adversarial, the oracle's outputs for them): the
    oracle runs once per operation, and a batch of any size draws its records from these."""
    if op.key not in _pools:
        rng = np.random.default_rng(sum(op.key.encode()) + 7000)
        cols, ns = op.pool(oracle, rng, op.unique)
        cols = [np.ascontiguousarray(c) for c in cols]
        _pools[op.key] = (cols, ns, op.want(oracle, *cols))
    return _pools[op.key]


def batch_of(op, oracle, n):
    """Seeded inputs of n records and the oracle's outputs: every wave of 64 holds the pool's adversarial records."""
    cols, ns, (want, wst) = pool_of(op, oracle)
    rng = np.random.default_rng(n * 31 + len(op.key))
    idx = rng.integers(ns, cols[0].shape[0], n)
    i = np.arange(n)
    slots, fixed = min(ns, SPECIAL_SLOTS), min(ns, SPECIAL_FIXED)
    for j in range(slots):
        at = i[i % 64 == 2 * j + 1]
        idx[at] = j if j < fixed else fixed + ((at // 64) * (slots - fixed) + (j - fixed)) % (ns - fixed)
    return [np.ascontiguousarray(c[idx]) for c in cols], (want[idx], None if wst is None else wst[idx])
