"""The bucket method's plan (decaf377_amd/csrc/msm_plan.hpp: msm_plan, span_len) without a GPU.

(1) The plan equals, field for field, what the launcher computed inline before the plan existed:
tests/golden/msm_plan_parent.json was written by a throwaway host program that held that launcher's workspace carve-up and
decision lines verbatim between the table of inputs and a printf.  The one deliberate difference: the middle level of the
tree now forces the 512-leaf block kernel, and no recorded case has a middle level without it.
(2) The safety properties the launcher used to state in comments hold for every recorded input.
(3) The lanes and partial slots of k_msm_spans stay inside what the plan reserves, for random bucket sizes with L from the
rule the device applies (span_len)."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_host_sim import sim  # noqa: F401  (fixture: the host build of the device headers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_plan_parent.json")))
OUT = GOLDEN["out_fields"]
REGIONS = GOLDEN["regions"]
CASES = GOLDEN["cases"]
IN = GOLDEN["in_fields"]
KIB = 1024


class Plan:
    def __init__(self, sim, inputs):  # noqa: F811
        a = np.array(inputs, np.int64)
        out = np.zeros(len(OUT) + 4, np.int64)
        off = np.zeros(64, np.uint64)
        sz = np.zeros(64, np.uint64)
        fold = np.zeros(3 * 16, np.int32)
        consts = np.zeros(16, np.int32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        sim.sim_msm_plan.restype = ctypes.c_int
        self.nregions = sim.sim_msm_plan(p(a), p(out), p(off), p(sz), p(fold), p(consts))
        self.inp = dict(zip(IN, inputs))
        self.out = [int(v) for v in out[:len(OUT)]]
        self.f = dict(zip(OUT, self.out))
        self.f.update(zip(("partials_bytes", "tmp_idx_bytes", "ws_depth", "nfolds"), (int(v) for v in out[len(OUT):])))
        self.off = [int(v) for v in off[:self.nregions]]
        self.sz = [int(v) for v in sz[:self.nregions]]
        self.fold = [tuple(int(v) for v in fold[3 * i:3 * i + 3]) for i in range(self.f["nfolds"])]
        self.k = dict(zip(("PT_WORDS", "FOLD", "SPAN_MIN", "NODE_STRIDE", "MID_STRIDE", "WSM_CAP", "R_PARTIALS", "R_TMP_IDX", "R_FOLD0",
                           "MSM_MAX_FOLDS"), (int(v) for v in consts)))


@pytest.fixture(scope="module")
def plans(sim):  # noqa: F811
    return [Plan(sim, c["in"]) for c in CASES]


def test_table_covers_the_grid_and_the_overrides():
    ins = [dict(zip(IN, c["in"])) for c in CASES]
    dflt = [i for i in ins if i["cus"] == 256 and i["span_blocks"] == 4 and all(i[k] == -1 for k in IN[4:])]
    for c in range(4, 19):
        assert {1, 70000, 1 << 20, (1 << 31) - 1} <= {i["n"] for i in dflt if i["c"] == c}, c
    # the widths the launcher picks by itself, at the sizes the grid leaves out to keep the record small
    assert {(257, 12), (5000, 12), (1 << 19, 14), (3 << 20, 16), (1 << 24, 16)} <= {(i["n"], i["c"]) for i in dflt}
    assert {8, 304} <= {i["cus"] for i in ins} and any(i["span_blocks"] == 1 for i in ins)
    assert {1, 4096} <= {i["slices"] for i in ins} and {1, 128} <= {i["seg"] for i in ins}
    assert any(i["red"] == 2 and i["skip"] == 1 for i in ins) and any(i["chunked_sums"] == 1 for i in ins)
    assert any(i["sort_packed"] == 0 for i in ins) and any(i["n"] == (1 << 24) + 1 for i in ins)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "msm_plan_parent.json")) < 64 * KIB


def test_plan_equals_the_parent_launcher(plans):
    assert len(REGIONS) == plans[0].nregions
    for case, p in zip(CASES, plans):
        want = dict(zip(OUT, case["out"]))
        # the deliberate difference: the middle level forces the 512-leaf block kernel -- which the CU-count rule chose anyway
        assert not (want["ws_mid"] and not want["ws8"]), case["in"]
        for name in OUT:
            assert p.f[name] == want[name], (case["in"], name)
        assert p.off == case["off"] and p.sz == case["sz"], case["in"]
        assert [v for step in p.fold for v in step] == case["fold"], case["in"]


def test_plan_invariants(plans):
    for p in plans:
        f, k, i = p.f, p.k, p.inp
        n, W, nb = i["n"], f["W"], f["nb"]
        tag = tuple(i.values())
        # the regions: aligned, inside the workspace, disjoint (they lie in order)
        end = 0
        for off, sz in zip(p.off, p.sz):
            assert off % 256 == 0 and off >= end and off + sz <= f["bytes"], tag
            end = off + sz
        # the lent region holds either of its uses
        assert k["R_PARTIALS"] == k["R_TMP_IDX"]
        assert f["partials_bytes"] == f["max_segs"] * k["PT_WORDS"] * 4 and f["tmp_idx_bytes"] == W * n * 4
        assert p.sz[k["R_PARTIALS"]] >= max(f["max_segs"] * k["PT_WORDS"] * 4, W * n * 4), tag
        # the folds: from nchunks down to one record per window, each into the buffer the one before did not write, and
        # each output inside its buffer
        m = f["nchunks"]
        assert f["nfolds"] <= k["MSM_MAX_FOLDS"]
        for j, (m_in, m_out, buf) in enumerate(p.fold):
            assert m_in == m and m_out == -(-m // k["FOLD"]) and buf == j % 2, tag
            assert W * m_out * k["PT_WORDS"] * 4 <= p.sz[k["R_FOLD0"] + buf], tag
            m = m_out
        assert m == 1, tag
        # the counting pass
        assert f["count_parts"] * f["count_nbr"] >= nb and f["count_nbr"] <= (1 << 15) + 1, tag
        assert f["hist_bytes"] == 4 * f["count_nbr"] and f["hist_bytes"] <= 160 * KIB and f["wsb_lds"] <= 160 * KIB, tag
        # the tree
        assert f["ws_m"] + 1 <= k["NODE_STRIDE"] and f["ws_nblk"] << f["ws_m"] == nb - 1, tag
        if f["ws_mid"]:
            fan = 1 << (f["mid_m"] - f["ws_m"])
            assert (fan // 2) * (f["ws_m"] + 2) <= k["WSM_CAP"], tag
            assert f["mid_m"] + 1 <= k["MID_STRIDE"] and f["top_nblk"] == 16 and f["mid_nblk"] == 16, tag
            assert (f["top_m"], f["top_stride"]) == (f["mid_m"], k["MID_STRIDE"]), tag
        elif f["tree"]:
            assert (f["top_m"], f["top_nblk"], f["top_stride"]) == (f["ws_m"], f["ws_nblk"], k["NODE_STRIDE"]), tag
        if f["tree"]:
            assert f["top_nblk"] << f["top_m"] == nb - 1 and p.sz[REGIONS.index("nodes")] > 0, tag
        else:                                                    # the chunked sums: no window level, no nodes
            assert not f["ws_mid"] and f["wsb_lds"] == 0 and p.sz[REGIONS.index("nodes")] == 0, tag
        # the sort's slices cover the chip once
        if i["slices"] == -1 and 2 * i["cus"] >= W:
            assert W * f["S"] <= 2 * i["cus"], tag
        assert f["S"] >= 1 and f["S"] * f["per"] >= n, tag
        # the span lanes.  (Without an override every window's lanes together are E / L + W at most with L >= SPAN_MIN and
        # L >= E / lanes_target; a forced L is the L, so there the bound is in terms of it.)
        if i["seg"] > 0:
            assert f["span_lanes_max"] >= n * W // i["seg"] + W, tag
        else:
            assert f["span_lanes_max"] >= min(n * W // k["SPAN_MIN"], f["lanes_target"]) + W, tag
        assert f["max_segs"] == f["span_lanes_max"] + W * nb + 1, tag
        assert f["max_g0"] == f["max_segs"], tag


def test_span_lanes_and_slots_fit_for_random_buckets(sim, plans):  # noqa: F811
    """Bucket sizes per window (some empty, one huge) that n points can produce; L from span_len as k_msm_scan2 applies it."""
    sim.sim_span_len.restype = ctypes.c_uint32
    rng = np.random.default_rng(2026)
    done = 0
    for p in plans:
        f, i = p.f, p.inp
        n, W, nb = i["n"], f["W"], f["nb"]
        if n > 1 << 22:                                          # (the sizes vectors stay small; E must fit 32 bits as on the device)
            continue
        for shape in range(3):
            lens, nonempty = [], 0
            for w in range(W):
                m = int(rng.integers(0, n + 1)) if shape else n       # points of this window with a non-zero digit
                if shape == 2:                                   # one huge bucket, the rest thin
                    sizes = np.zeros(nb, np.int64)
                    rest = min(m, nb - 2)
                    sizes[rng.choice(np.arange(1, nb), rest, replace=False)] = 1
                    sizes[int(rng.integers(1, nb))] += m - rest
                else:
                    sizes = rng.multinomial(m, np.full(nb - 1, 1.0 / (nb - 1)))
                    if shape:
                        sizes[rng.random(nb - 1) < 0.3] = 0      # some buckets empty: fewer entries (shape 0: all n W entries)
                lens.append(int(sizes.sum()))
                nonempty += int((sizes != 0).sum())
            E = sum(lens)
            L = sim.sim_span_len(E, f["lanes_target"], f["forced_L"])
            assert L >= 1
            lanes = sum(-(-ln // L) for ln in lens)
            assert lanes <= f["span_lanes_max"], (tuple(i.values()), shape, L)
            if lanes:
                assert (lanes - 1) + (nonempty - 1) < f["max_segs"], (tuple(i.values()), shape)
            done += 1
    assert done >= 100
    # the rule itself
    assert sim.sim_span_len(0, 1000, 0) == 8 and sim.sim_span_len(8001, 1000, 0) == 9 and sim.sim_span_len(10 ** 6, 1000, 0) == 1000
    assert sim.sim_span_len(10 ** 6, 1000, 1) == 1 and sim.sim_span_len(5, 1000, 128) == 128
