"""The batch launchers' plan (decaf377_amd/csrc/launch_plan.hpp: launch_plan, lane_deal, sums_wave_max) without a GPU.

(1) The plan equals, field for field, what the launchers computed inline before the plan existed:
tests/golden/launch_plan_parent.json was written by a throwaway host program that held those launchers' decision lines
verbatim -- grid_of, deal_chunks, lane_chunks, the batch maxima, the body of d377.hip's launch() with every kernel launch
replaced by a print of its route, grid and block, and the sums' wave-or-lane line -- between a table of inputs and a printf.
(2) The properties the launcher used to state in comments hold for every recorded input.
(3) The chunk deal is one function: the generic launcher's form, with no tuning key set, and the sums' form give the same
numbers."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_host_sim import sim  # noqa: F401  (fixture: the host build of the device headers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")
GOLDEN = json.load(open(PATH))
IN, OUT, ROUTES, OPS, TUNINGS = (GOLDEN[k] for k in ("in_fields", "out_fields", "routes", "ops", "tunings"))
TUNE_KEYS = IN[4:]
DEFAULT = TUNINGS.index([-1] * len(TUNE_KEYS))
R = {name: i for i, name in enumerate(ROUTES)}
DEALT = {R["lane_sets"], R["codec_chunked"], R["fb_narrow"], R["fb_wide"], R["el_uniform"]}
FOUR_OPS = ("sqrt", "decompress", "compress", "roundtrip", "encode", "hash")
CODEC_OPS = ("decompress", "compress", "roundtrip")
SMALL_OPS = ("mul_base", "mul_var", "mul_var_el", "mul_base_el")
LANE_OPS = FOUR_OPS + ("mul_var", "encode_wide48", "encode_wide64", "encode_el", "hash_el")


def pad(row):
    return list(row) + [0] * (len(OUT) - len(row))


def p64(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def launch_plan(sim, op, aux, n, cus, tune):  # noqa: F811
    out = np.zeros(len(OUT), np.int64)
    sim.sim_launch_plan(p64(np.array([op, aux, n, cus] + list(tune), np.int64)), p64(out))
    return [int(v) for v in out]


def sums_route(sim, np_, cus, kmax, tiny_max):  # noqa: F811
    out = np.zeros(len(OUT), np.int64)
    sim.sim_sums_route(p64(np.array([np_, cus, kmax, tiny_max], np.int64)), p64(out))
    return [int(v) for v in out]


def lane_deal(sim, count, cus, sets, kmax, chunk_per_lane=-1):  # noqa: F811
    out, consts = np.zeros(6, np.int64), np.zeros(8, np.int64)
    sim.sim_lane_deal(ctypes.c_int64(count), cus, sets, kmax, ctypes.c_int64(chunk_per_lane), p64(out), p64(consts))
    return [int(v) for v in out], dict(zip(("BLOCK", "WAVES_PER_SIMD", "DCB_K", "DCB_KMAX", "DCB_K_LONG", "FB_SETS", "FB_K", "PIPE_CHUNK"),
                                            (int(v) for v in consts)))


@pytest.fixture(scope="module")
def K(sim):  # noqa: F811
    return lane_deal(sim, 1, 1, 1, 1)[1]


def cases():
    """(op name, aux, n, cus, tuning as a dict, recorded outputs as a dict)"""
    for g in GOLDEN["cases"]:
        tune = dict(zip(TUNE_KEYS, TUNINGS[g["tune"]]))
        for n, row in zip(g["n"], g["out"]):
            yield OPS[g["op"]], g["aux"], n, g["cus"], tune, dict(zip(OUT, pad(row)))


def test_plan_equals_the_parent_launcher(sim):  # noqa: F811
    count = 0
    for g in GOLDEN["cases"]:
        for n, row in zip(g["n"], g["out"]):
            got = launch_plan(sim, g["op"], g["aux"], n, g["cus"], TUNINGS[g["tune"]])
            assert got == pad(row), (OPS[g["op"]], n, g["cus"], TUNINGS[g["tune"]], dict(zip(OUT, got)))
            count += 1
    for g in GOLDEN["sums"]:
        for np_, row in zip(g["np"], g["out"]):
            got = sums_route(sim, np_, g["cus"], g["kmax"], g["tiny_max"])
            assert got == pad(row), ("sums", np_, g["cus"], g["kmax"], g["tiny_max"], dict(zip(OUT, got)))
            count += 1
    assert count > 1500


def test_table_covers_the_ops_the_thresholds_and_the_overrides(K):
    assert os.path.getsize(PATH) < 64 * 1024
    assert len(OPS) == 33 and OUT[:4] == ["route", "grid", "block", "guard"]
    have = {}
    for op, _, n, cus, tune, _ in cases():
        have.setdefault((op, cus, tuple(tune.values())), set()).add(n)
    dflt = tuple([-1] * len(TUNE_KEYS))
    B, W, KL = K["BLOCK"], K["WAVES_PER_SIMD"], K["DCB_K_LONG"]

    def both(*ts):
        return {v for t in ts for v in (t, t + 1)}

    def deal(cus, sets, kmax):                              # a workgroup per round; one generation; two (priority); the cap of cus * 64 chunks
        places = cus * sets
        return both(places * B, places * B * kmax, 2 * places * B * kmax, (cus * 64 // places) * places * B * kmax, cus * 64 * B * kmax)

    for cus in (8, 256, 304):
        res = cus * W * B
        tiny = min(cus * 4, cus * 16 * 7)
        for op in OPS:
            ns = have[(op, cus, dflt)]
            want = {1, 5 << 18, 1 << 20, 1 << 22, 1 << 28}
            if op in FOUR_OPS:
                want |= both(4 * tiny)
            if op == "hash":
                want |= both(2 * tiny)
            if op in SMALL_OPS:
                want |= both(tiny, cus * 16 * (7 if op.endswith("_el") else 8))
            if op in LANE_OPS:
                want |= deal(cus, W, KL)
            if op in CODEC_OPS:
                want |= both(res * 2 - 1)
            if op == "mul_base":
                want |= both(res * K["DCB_K"]) | deal(cus, W, K["DCB_K"]) | deal(cus, K["FB_SETS"], K["FB_K"])
            if op == "mul_var_el":
                want |= both(res, 4 * res, cus * 64 * B * 2)
            if op == "affine":
                want |= both(cus * B, cus * B * 32 - 32, cus * B * 32)
            if op not in LANE_OPS + ("mul_base", "mul_var_el", "affine") or op in CODEC_OPS:
                want |= both(cus * 32 * B)
            assert want <= ns, (op, cus, sorted(want - ns))
    # the thresholds the issue names, on 256 CUs
    assert both(4096) <= have[("sqrt", 256, dflt)] and both(2048) <= have[("hash", 256, dflt)] and both(1024) <= have[("mul_var", 256, dflt)]
    assert both(32768) <= have[("mul_var", 256, dflt)] and both(28672) <= have[("mul_var_el", 256, dflt)]
    assert both(131072) <= have[("encode", 256, dflt)] and both(262143) <= have[("compress", 256, dflt)] and both(1 << 20) <= have[("mul_base", 256, dflt)]
    # the overrides, on the ops they touch
    def tuned(op, **kv):
        t = tuple(kv.get(k, -1) for k in TUNE_KEYS)
        return have.get((op, 256, t), set())
    for op in SMALL_OPS:
        assert tuned(op, small_max=0) and both(5000) <= tuned(op, small_max=5000), op
        assert both(64) <= tuned(op, tiny_max=64) and tuned(op, tiny_max=100000), op
    for op in FOUR_OPS:
        assert tuned(op, small_max=0) and both(256) <= tuned(op, tiny_max=64), op
    for op in CODEC_OPS:
        assert tuned(op, decompress_chunked_min=0) and both(999999) <= tuned(op, decompress_chunked_min=1000000), op
        assert tuned(op, decompress_chunked_min=1 << 62), op
    for w in (0, 1):
        assert both(1 << 20) <= tuned("mul_base", fb_wide=w)
    assert tuned("mul_base", fb_k=4) and tuned("mul_base", fb_k=16) and tuned("mul_base", fb_k=4, fb_wide=1) and tuned("mul_base", fb_k=16, fb_wide=0)
    assert tuned("affine", affine_blocks_per_cu=2) and tuned("affine", affine_blocks_per_cu=64)
    for op in LANE_OPS[:8] + ("mul_base", "mul_var_el", "encode_wide48", "encode_el"):
        for v in (1, 8):
            assert {131073, 5 << 18, 1 << 28} <= tuned(op, chunk_per_lane=v), (op, v)
    # the sums: both sides of wave_max with and without TINY_MAX, both chunk lengths
    sums = {(g["cus"], g["kmax"], g["tiny_max"]): set(g["np"]) for g in GOLDEN["sums"]}
    for cus in (8, 256, 304):
        for kmax in (K["DCB_K"], KL):
            assert both(16 * cus) | deal(cus, W, kmax) | {1, 5 << 18, 1 << 20, 1 << 22, 1 << 28} <= sums[(cus, kmax, -1)], (cus, kmax)
    for kmax in (K["DCB_K"], KL):
        assert {1} <= sums[(256, kmax, 0)] and both(256) <= sums[(256, kmax, 64)] and both(400000) <= sums[(256, kmax, 100000)]


def check_deal(tag, K, n, cus, sets, f, uniform):
    """The invariants of a dealt launch: f = its recorded outputs, `sets` lane sets per CU, uniform: chunks of per_lane, no extra."""
    B = K["BLOCK"]
    places, rounds, cap = cus * sets, -(-n // B), cus * 64
    grid, per_lane, extra, kmax = f["grid"], f["per_lane"], f["extra"], f["kmax"]
    assert f["nslots"] == places and f["block"] == B and f["guard"] == 1, tag
    assert 1 <= per_lane and per_lane + (extra > 0) <= kmax <= K["DCB_KMAX"], tag
    assert 1 <= grid <= cap and 0 <= extra < grid, tag
    even = not uniform and grid <= (cap // places) * places and (grid == rounds or grid % places == 0)
    if even and (grid < cap or per_lane * grid + extra == rounds):
        # one workgroup per chunk and every round dealt out exactly once; full generations beyond one round per place
        assert per_lane * grid + extra == rounds, tag
        assert grid == rounds if rounds <= places else grid == -(-rounds // (places * kmax)) * places, tag
    elif grid < cap:
        # uniform chunks (an override, or beyond the generations the cap admits): every round has a chunk, no chunk is empty
        assert extra == 0 and per_lane * (grid - 1) < rounds <= per_lane * grid, tag
    else:
        # at the cap the workgroups walk several chunks of per_lane
        assert extra == 0 and per_lane * grid <= rounds + per_lane - 1, tag
    return places


def test_plan_invariants(K):
    for op, aux, n, cus, tune, f in cases():
        tag = (op, n, cus, tune, f)
        route, grid = f["route"], f["grid"]
        assert grid >= 1 and f["block"] in (64, K["BLOCK"]), tag
        assert f["guard"] == (route in DEALT), tag
        if route == R["four_per_wave"]:
            assert f["block"] == 64 and 4 * (grid - 1) < n <= 4 * grid, tag
        elif route == R["pair_per_wave"]:
            assert f["block"] == 64 and 2 * (grid - 1) < n <= 2 * grid, tag
        elif route == R["wave_per_element"]:
            assert f["block"] == 64 and grid == n, tag
        elif route == R["quad_per_element"]:
            assert f["block"] == 64 and 16 * (grid - 1) < n <= 16 * grid, tag
        elif route in (R["wide_grid"], R["plain"]):
            assert grid == min(-(-n // K["BLOCK"]), cus * 32), tag
        elif route == R["affine"]:
            lanes = grid * K["BLOCK"]
            assert lanes >= min(n, cus * K["BLOCK"]) or lanes * 32 >= n, tag       # a wave per SIMD at least, unless the batch is smaller
            assert lanes * 32 + 32 * K["BLOCK"] > n or lanes <= cus * 64 * K["BLOCK"], tag
        if route not in DEALT:
            assert [f[k] for k in ("nslots", "per_lane", "extra", "prio", "kmax")] == [0] * 5, tag
            continue
        sets = K["FB_SETS"] if route == R["fb_wide"] else K["WAVES_PER_SIMD"]
        uniform = tune["chunk_per_lane"] >= 0 or route == R["el_uniform"]
        places = check_deal(tag, K, n, cus, sets, f, uniform)
        if route == R["fb_wide"]:
            # the fixed-base wide launch's own rule: priorities in ONE generation only
            assert f["prio"] == (1 if grid <= places else 0), tag
        else:
            assert f["prio"] == (1 if grid <= 2 * places else 0), tag
        if route == R["el_uniform"]:
            assert f["per_lane"] == (2 if n > places * K["BLOCK"] else 1) and f["kmax"] == 2, tag
        elif route in (R["fb_narrow"], R["fb_wide"]):
            assert f["kmax"] == (tune["fb_k"] if tune["fb_k"] >= 0 else (K["FB_K"] if route == R["fb_wide"] else K["DCB_K"])), tag
        else:
            assert f["kmax"] == K["DCB_K_LONG"], tag
        if op in CODEC_OPS:
            assert n >= f["codec_chunked_min"], tag
    for g in GOLDEN["sums"]:
        for np_, row in zip(g["np"], g["out"]):
            f = dict(zip(OUT, pad(row)))
            tag = ("sums", np_, g, f)
            wave_max = 4 * (g["tiny_max"] if g["tiny_max"] >= 0 else 4 * g["cus"])
            assert f["route"] == (R["wave_per_element"] if np_ <= wave_max else R["lane_sets"]), tag
            if f["route"] == R["wave_per_element"]:
                assert f["grid"] == np_ and f["block"] == 64, tag
                continue
            f["guard"] = 1                                   # (not the header's affair for a sum; check_deal expects a launch's)
            places = check_deal(tag, K, np_, g["cus"], K["WAVES_PER_SIMD"], f, False)
            assert f["kmax"] == g["kmax"] and f["prio"] == (1 if f["grid"] <= 2 * places else 0), tag


def test_routes_never_return_along_n():
    """Default tuning: as n grows an op moves from route to route and never back to one it has left."""
    seqs = {}
    for op, _, n, cus, tune, f in cases():
        if all(v == -1 for v in tune.values()):
            seqs.setdefault((op, cus), []).append((n, f["route"]))
    assert len(seqs) == 3 * len(OPS)
    for key, seq in seqs.items():
        routes = [r for _, r in sorted(seq)]
        order = [r for i, r in enumerate(routes) if i == 0 or r != routes[i - 1]]
        assert len(order) == len(set(order)), (key, [ROUTES[r] for r in order])
    # ... and the families every size class goes through, on 256 CUs
    names = lambda op: [ROUTES[r] for r in dict.fromkeys(r for _, r in sorted(seqs[(op, 256)]))]  # noqa: E731
    assert names("hash") == ["pair_per_wave", "four_per_wave", "lane_sets"]
    assert names("compress") == ["four_per_wave", "wide_grid", "codec_chunked"] and names("decompress") == ["four_per_wave", "wide_grid", "lane_sets"]
    assert names("mul_base") == ["wave_per_element", "quad_per_element", "fb_narrow", "fb_wide"]
    assert names("mul_var_el") == ["wave_per_element", "quad_per_element", "el_uniform"]
    assert names("mul_base_el") == ["wave_per_element", "quad_per_element", "plain"] and names("affine") == ["affine"] and names("add") == ["plain"]


def test_the_launchers_deal_is_the_sums_deal(sim, K):  # noqa: F811
    """batch_host.hpp's lane_chunks was 'as d377.hip's chunks_of': with no tuning key set they are one function of (count, cus, kmax)."""
    rng = np.random.default_rng(377)
    B, W = K["BLOCK"], K["WAVES_PER_SIMD"]
    done = 0
    for cus in (8, 256, 304):
        for kmax in (1, 4, K["DCB_K"], K["DCB_K_LONG"]):
            places = cus * W
            marks = [1, B, places * B, places * B * kmax, 2 * places * B * kmax, 32 * places * B * kmax, cus * 64 * B * kmax, 1 << 28]
            counts = {max(1, m + d) for m in marks for d in (-1, 0, 1)} | {int(v) for v in rng.integers(1, 1 << 27, 40)}
            for count in sorted(counts):
                deal, _ = lane_deal(sim, count, cus, W, kmax)
                f = dict(zip(OUT, sums_route(sim, count, cus, kmax, 0)))      # TINY_MAX 0: no sum takes the wave route
                assert f["route"] == R["lane_sets"]
                assert deal == [f[k] for k in ("grid", "nslots", "per_lane", "extra", "prio", "kmax")], (count, cus, kmax)
                done += 1
    assert done > 500
    # ... and the override is the launcher's form alone: uniform chunks of that many rounds, at most kmax, capped alike
    deal, _ = lane_deal(sim, 5 << 18, 256, W, 16, chunk_per_lane=2)
    assert deal == [2560, 512, 2, 0, 0, 16]
    deal, _ = lane_deal(sim, 1 << 28, 256, W, 4, chunk_per_lane=8)
    assert deal == [256 * 64, 512, 4, 0, 0, 4]
    assert K["PIPE_CHUNK"] == 1 << 18
