"""The in-place contract without a GPU: tests/_in_place_cases.py's table against the prototypes of include/decaf377_amd.h, and
its route plan against the host build of launch_plan.hpp (tests/host_sim: sim_launch_plan, as tests/test_launch_plan_host.py
calls it) on 256 CUs."""
import os
import re

import _in_place_cases as cases
from decaf377_amd import _native
from test_host_sim import sim  # noqa: F401  (fixture: the host build of the device headers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Bytes per record of every pointer parameter of the `_dev` exports, by the parameter's name: written here from the header's
# "Records" section and the comments on the prototypes, independently of _in_place_cases.TABLE.  None: no fixed size (the
# `len` argument gives it).  (`a`, `b`, `out`: four Montgomery limbs; `xy`: affine x, y; flags and statuses: one byte.)
RECORD_BYTES = {
    "num32": 32, "den32": 32, "root32": 32, "was_square": 1, "enc32": 32, "enc32_out": 32, "status": 1, "xyzt": 128, "scalar32": 32,
    "fq32": 32, "r1_32": 32, "r2_32": 32, "p_xyzt": 128, "q_xyzt": 128, "out_xyzt": 128, "equal": 1, "a": 32, "b": 32, "out": 32,
    "is_identity": 1, "bytes": None, "fq32_out": 32, "xy": 64, "fq_out": 32, "bytes32": 32, "fr32_out": 32, "a32": 32, "b32": 32,
    "out32": 32, "xyzt_out": 128,
}
# `_dev` exports that are no element-wise map: the sums (their inputs and outputs differ in COUNT, n terms to one record or m
# terms to a sum), the peer-copy path (untyped buffers of the operation it names: cases.SHARDED) and a counter's address
NOT_MAPS = {"d377_msm_dev", "d377_msm_encoded_dev", "d377_sum_elements_dev", "d377_batch_msm_small_dev", "d377_batch_msm_small_encoded_dev",
            "d377_batch_sharded_dev", "d377_ctx_starved_counter_dev"}


def dev_prototypes():
    """name -> [(const?, parameter name)] of the pointer parameters behind (ctx, dev, stream) of every `_dev` prototype."""
    text = open(os.path.join(ROOT, "include", "decaf377_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(d377_[a-z0-9_]+_dev)\s*\(([^)]*)\)\s*;", text):
        params = []
        for a in m.group(2).split(",")[3:]:
            a = re.sub(r"\s+", " ", a).strip()
            if "*" in a:
                params.append((a.startswith("const "), re.search(r"([A-Za-z_0-9]+)$", a).group(1)))
        protos[m.group(1)] = params
    return protos


def test_table_is_every_dev_export_with_an_equal_sized_input_and_output():
    protos = dev_prototypes()
    dev_exports = {e for e in _native.EXPORTS if e.endswith("_dev")}
    assert set(protos) == dev_exports and NOT_MAPS <= dev_exports
    derived = {}
    for name in sorted(dev_exports - NOT_MAPS):
        ins = [p for const, p in protos[name] if const]
        outs = [p for const, p in protos[name] if not const]
        assert ins and outs, name
        pairs = {o: tuple(i for i in ins if RECORD_BYTES[i] is not None and RECORD_BYTES[i] == RECORD_BYTES[o]) for o in outs}
        pairs = {o: i for o, i in pairs.items() if i}
        if pairs:
            assert len(pairs) == 1, (name, pairs)                    # one output record that an input can be: out0
            derived[name] = next(iter(pairs.items()))
    assert derived == cases.TABLE, {k: (derived.get(k), cases.TABLE.get(k)) for k in set(derived) ^ set(cases.TABLE) | {
        k for k in set(derived) & set(cases.TABLE) if derived[k] != cases.TABLE[k]}}
    assert len(cases.TABLE) == 18
    # every row is driven, every alias of it, and every selector of the two field-operation exports
    driven = {}
    for op in cases.OPS:
        driven.setdefault(op.export, set()).update(op.alias)
    assert {e: set(range(len(i))) for e, (_, i) in cases.TABLE.items()} == driven
    for prefix, export in (("fq_op:", "d377_batch_fq_op_dev"), ("fr_op:", "d377_batch_fr_op_dev")):
        assert [op.key for op in cases.OPS if op.export == export] == [prefix + f for f in cases.FIELD_OPS]
    assert {"sqrt_ratio_zeta_ex:ark", "sqrt_ratio_zeta_ex:min_curve", "sqrt_ratio_zeta"} <= set(cases.BY_KEY)
    # the operations of the peer-copy path that the table covers
    from decaf377_amd.engine import SHARD_OPS
    assert set(cases.SHARDED) == set(SHARD_OPS) - {"decompress", "compress", "scalar_mul_base_element"}
    assert set(cases.SHARDED.values()) <= set(cases.TABLE)


# the routes launch_plan.hpp has for each family of the table
ROUTES = {
    "sqrt": {"four_per_wave", "lane_sets"}, "encode": {"four_per_wave", "lane_sets"},
    "hash": {"pair_per_wave", "four_per_wave", "lane_sets"},
    "roundtrip": {"four_per_wave", "wide_grid", "codec_chunked"},
    "mul_var": {"wave_per_element", "quad_per_element", "lane_sets"},
    "mul_base": {"wave_per_element", "quad_per_element", "fb_narrow", "fb_wide"},
    "mul_var_el": {"wave_per_element", "quad_per_element", "el_uniform"},
    "plain": {"plain"}, "inverse": {"plain"},
}


def test_route_plan_reaches_every_operation_and_route_on_256_cus(sim):  # noqa: F811
    cus = 256
    want = {(op.key, r) for op in cases.OPS for r in ROUTES[op.family]}
    assert want == set(cases.CLAIMED)
    reached, launches = set(), 0
    alone = cases.plan_lib()                                         # launch_plan.hpp built alone: what the GPU module asks
    for op in cases.OPS:
        seen = {}
        for route, tuning, n in cases.route_cases(op.family, cus):
            f = cases.planned(sim, op.plan_op, n, cus, tuning)
            assert f["route"] == route, (op.key, route, tuning, n, f)
            assert all(cases.planned(alone, op.plan_op, n, c, tuning) == cases.planned(sim, op.plan_op, n, c, tuning) for c in (cus, 304, 8))
            seen.setdefault(route, []).append((n, tuning, f))
            reached.add((op.key, route))
            launches += 1 + len(op.alias) + (1 if op.both else 0) * 2
        ns = lambda r: sorted({n for n, _, _ in seen.get(r, ())})  # noqa: E731
        for r in ("four_per_wave", "pair_per_wave", "wave_per_element", "quad_per_element"):
            if r in seen:
                # hash_to_curve on four per wave: no tuning gives that route to one or two pairs (two pairs per wave take them)
                assert ns(r) == sorted(cases.WAVE_N)[2 if (op.family, r) == ("hash", "four_per_wave") else 0:], (op.key, r)
        for r in ("lane_sets", "codec_chunked", "fb_narrow", "fb_wide"):
            if r not in seen:
                continue
            assert ns(r) == sorted(cases.LANE_N + tuple(cases.chunk_n(k) for k in cases.CHUNK_K)), (op.key, r)
            deals = {(t.get("fb_k", -1), t.get("chunk_per_lane", -1)): f for n, t, f in seen[r] if n > 1000}
            for (fk, k), f in deals.items():
                # two full chunks of k rounds and a ragged third (k clipped to the fixed-base launch's elements per inversion)
                per = min(k, fk) if fk > 0 else k
                assert f["per_lane"] == per and f["extra"] == 0 and f["grid"] == -(-(2 * k + 1) // per), (op.key, r, fk, k, f)
            assert {k for _, k in deals} == set(cases.CHUNK_K)
            if r.startswith("fb_"):
                assert {fk for fk, _ in deals} == set(cases.FB_K) and all(f["kmax"] == fk for (fk, _), f in deals.items())
        if "el_uniform" in seen:
            big = cases.resident_lanes(cus) + 257
            assert ns("el_uniform") == sorted(cases.LANE_N + (big,))
            assert [f["per_lane"] for n, _, f in seen["el_uniform"]] == [1] * len(cases.LANE_N) + [2]
        if op.family in ("plain", "inverse"):
            assert ns("plain") == sorted(cases.INVERSE_N if op.key == "fq_op:inverse" else cases.PLAIN_N), op.key
        if "wide_grid" in seen:
            assert ns("wide_grid") == sorted(cases.PLAIN_N)
    assert reached == want
    assert 1 - len(reached) / len(cases.CLAIMED) == 0                # the share of claimed (operation, route) pairs left out
    assert launches == 883                                           # what the GPU module's matrix launches, each a few milliseconds at most
