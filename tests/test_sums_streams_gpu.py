"""Batched sums on two streams queue on the scratch they share (include/decaf377_amd.h, "Threads and streams").

Every case has the same shape.  The expected bytes come from the oracle's fold before any launch.  A gate -- at least 200 ms
of plain torch kernels (tests/_sums_support.py: Gate) -- is enqueued on stream s1, call A behind it, call B on s2, an otherwise
idle stream.  The gate must still be running once B has been enqueued ("gate too short" otherwise: the case would prove
nothing).  Then s2 is synchronised: where A and B share a guard (GUARD_OF), A's event must have fired -- B queued behind A,
which held the area first; a launch function that skipped the hand-over would let B finish while s1 still sits in the gate.
Last, after a device synchronise, both outputs are the oracle's: Encodings and statuses byte for byte, Element records under
eq_xyzt, the index verdict (0, none), and the context's health shows no lane set claimed and no workgroup that gave up.

Two streams can land on one hardware queue, and then B runs behind A with or without a guard.  The module's fixture picks s2
with a control (pick_independent_stream) and s1 so that the context's private stream is independent of it too; if no
independent stream is found every case still checks its results and then SKIPS, saying that the ordering was not checked.

The 200 ms: each call here takes about a millisecond alone and the host enqueues A and B in well under 10 ms.

Every case first runs its calls once with nothing in flight (same bytes expected): the areas have then grown, so that in the
gated run no call drains a guard on the host -- except in the growth cases, which are about that drain and take a fresh
context.  Where B waits on the host (growth, destroy, the host forms) the gate's condition is checked in front of B.

n = 257 is two workgroups of 256 lanes with one live lane in the second; the wave routes are off (tiny_max = 0,
msm_small_max = 0), so every call takes its lane kernel and the bucket pipeline.  The segmented fixed-base case takes 29 sums
over 101 bases (2929 terms): far fewer sums than resident lanes, so every sum is cut, into single-base segments at this n --
segments of several bases need more sums than lanes / 101, hundreds of thousands of terms.

What the growth and destroy cases cannot tell apart: hipFree waits for the device by itself, so there the host has waited for A
whether through the drain or through the free.  They pin the contract (B returns after A, the bytes are right, the larger area
serves A again); the same-guard pairs and the host forms, where nothing is freed, are the cases a missing hand-over fails."""
import threading

import numpy as np
import pytest

import _batch_msm_long_cases as lc
import _bucket_sums_cases as bc
import _fixed_msm_long_cases as fl
from _batch_msm_long_cases import oracle_fold
from _msm_long_indexed_cases import POOL, make_indexed, make_pool, materialise
from _sums_support import (Gate, Side, indexed_fold_by_scalar_mul, join, mixed_case, pick_independent_stream, planted_scalars,
                           runs_beside, var_terms)

pytestmark = pytest.mark.gpu

N = 257
NONE = (1 << 64) - 1
GATE_MS = 200.0
TUNING = {"tiny_max": 0, "msm_small_max": 0}

# call (stream form) -> (guard, shape-dependent area): read off the launch functions (batch_msm.hip: batch_msm_launch,
# batch_msm_mixed.hip: mixed_launch, batch_msm_long.hip: batch_msm_long_launch, batch_msm_long_indexed.hip:
# batch_msm_long_indexed_launch, fixed_bases.hip: fixed_msm_launch / fixed_msm_long_launch, msm.hip: msm_reserve,
# msm_batch.inc: bsum_launch).  "vb" = DeviceState::vb_guard, "msm" = DeviceState::msm_guard.
GUARD_OF = {
    "d377_batch_msm_small_dev": ("vb", "table scratch (m tables per lane)"),
    "d377_batch_msm_small_encoded_dev": ("vb", "table scratch (m tables per lane)"),
    "d377_batch_msm_mixed_resident": ("vb", "table scratch (v tables)"),
    "d377_batch_msm_mixed_encoded_resident": ("vb", "table scratch (v tables)"),
    "d377_batch_long_msm_resident": ("vb", "table scratch (b tables), partials"),
    "d377_batch_long_msm_encoded_resident": ("vb", "table scratch (b tables), partials"),
    "d377_batch_long_msm_indexed_resident": ("vb", "table scratch (b tables), partials"),
    "d377_batch_fixed_long_msm_resident": ("vb", "partials (more than one segment per sum)"),
    "d377_batch_fixed_msm_resident": ("vb", "lane sets only"),
    "d377_batch_fixed_msm_indexed_resident": ("vb", "lane sets only"),
    "d377_msm_dev": ("msm", "MSM workspace"),                      # (its chunked decoding pass takes vb inside, Encoding form)
    "d377_msm_encoded_dev": ("msm", "MSM workspace"),
    "d377_batch_bucket_msm_resident": ("msm", "MSM workspace"),
    "d377_batch_bucket_msm_encoded_resident": ("msm", "MSM workspace"),   # (the same decoding pass)
}


class Call:
    """One prepared resident call: device inputs and prefilled outputs made before any gate, the oracle's bytes to compare with."""

    def __init__(self, side, symbol, ins, outs, want):
        """ins: the arguments between the stream and the outputs (tensors or integers); outs: kinds in the call's order --
        ("enc", rows), ("el", rows), ("st", rows), ("ver",); want: {kind: expected array}."""
        self.side, self.symbol, self.ins, self.want = side, symbol, ins, want
        self.kinds = [o[0] for o in outs]
        self.outs = [self._empty(*o) for o in outs]

    def _empty(self, kind, rows=None):
        s = self.side
        if kind == "enc":
            return s.empty((rows, 32), fill=0xA5)
        if kind == "el":
            return s.empty((rows, 16), "u64", fill=0x5A5A)
        if kind == "st":
            return s.empty((rows,), fill=0xEE)
        return s.empty((2,), "u64", fill=7)

    def reset(self):
        for kind, t in zip(self.kinds, self.outs):
            t.fill_({"enc": 0xA5, "el": 0x5A5A, "st": 0xEE, "ver": 7}[kind])
        self.side.torch.cuda.synchronize()

    def enqueue(self, stream):
        self.side.ok(self.symbol, *self.ins, *self.outs, stream=stream.cuda_stream)

    def got(self):
        """The outputs on the host (after a synchronise of the caller's)."""
        out = {}
        for kind, t in zip(self.kinds, self.outs):
            a = t.cpu().numpy()
            out[kind] = a.view(np.uint64) if a.dtype == np.int64 else a
        return out

    def check(self, oracle, what):
        got = self.got()
        _same(oracle, (what, self.symbol), got, self.want)
        return got


def _same(oracle, tag, got, want):
    assert (got["enc"] == want["enc"]).all(), (tag, np.nonzero((got["enc"] != want["enc"]).any(1))[0][:8])
    if "el" in got:
        assert oracle.eq_xyzt(np.ascontiguousarray(got["el"]), np.ascontiguousarray(want["el"])).all(), tag
        assert (oracle.compress(np.ascontiguousarray(got["el"])) == got["enc"]).all(), tag
    if "st" in got:
        assert (got["st"] == want["st"]).all(), tag
    if "ver" in got:
        assert got["ver"].tolist() == [0, NONE], tag


class Cases:
    """The host arrays of every case and the oracle's results, made once per module and never written again."""

    def __init__(self, oracle):
        self.o, self.memo = oracle, {}

    def get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def _points(self, rng, terms):
        return np.ascontiguousarray(self.o.elligator_map_xyzt(rng.integers(0, 256, (terms, 32), dtype=np.uint8)), dtype=np.uint64)

    def small(self, m, encoded=False):
        def make():
            rng = np.random.default_rng(8000 + 10 * m + encoded)
            pts = self._points(rng, N * m)
            k = planted_scalars(rng, N, m)
            if encoded:
                pts = self.o.compress(pts)
                pts[3::7] = 0xFF                                 # above q: no canonical Encoding
            else:
                pts[5, 8:12] = 0                                 # a record with Z = 0: the identity
            enc, el, st = oracle_fold(self.o, pts, k, m)
            return dict(pts=pts, k=k, m=m, n=N, want=dict(enc=enc, el=el, st=st))
        return self.get(("small", m, encoded), make)

    def mixed(self, v, t, encoded=False):
        def make():
            bases, idx, fk, pts, vk = mixed_case(self.o, v, t, 2, N)
            fixed = indexed_fold_by_scalar_mul(self.o, bases, idx, fk)[1]
            terms = var_terms(self.o, pts, vk, N, v)
            live = None
            st = None
            if encoded:
                good = pts.copy()
                good[~good[:, 8:12].any(1)] = self.o.identity_xyzt()
                pts = self.o.compress(good)
                bad = np.zeros(N * v, bool)
                bad[::5] = True
                pts[bad] = 0xFF
                live, st = ~bad.reshape(N, v), bad.astype(np.uint8)
            enc, el = join(self.o, fixed, terms, live)
            return dict(bases=bases, idx=idx, fk=fk, pts=pts, vk=vk, v=v, t=t, n=N, want=dict(enc=enc, el=el, st=st))
        return self.get(("mixed", v, t, encoded), make)

    def long(self, n, m, encoded=False):
        def make():
            pts, k, _ = lc.make_case(self.o, np.random.default_rng(100 * m + n + encoded), n, m, encoded=encoded)
            enc, el, st = oracle_fold(self.o, pts, k, m)
            return dict(pts=pts, k=k, m=m, n=n, want=dict(enc=enc, el=el, st=st))
        return self.get(("long", n, m, encoded), make)

    def long_indexed(self, n, m):
        def make():
            rng = np.random.default_rng(300 * m + n)
            pool = make_pool(self.o, rng)
            idx, k, info = make_indexed(rng, n, m)
            assert info["absent"].any()                          # -1 terms
            enc, el, _ = oracle_fold(self.o, materialise(pool, idx), k, m)
            return dict(pool=pool, idx=idx, k=k, m=m, n=n, want=dict(enc=enc, el=el))
        return self.get(("long_indexed", n, m), make)

    def fixed3(self):
        """Three bases; dense scalars and an indexed case of t = 2 over the same bases."""
        def make():
            rng = np.random.default_rng(3)
            bases = fl.make_bases(self.o, rng, 3, 3)
            k = fl.make_scalars(rng, N, 3, 1, 3)
            enc, el = fl.oracle_fold(self.o, bases, k, N, 3)
            idx = rng.integers(-1, 3, (N, 2)).astype(np.int32)
            idx[0], idx[1], idx[2] = (2, -1), (0, 0), (-1, -1)    # the last base and an absent term; a repeat; no term at all
            ik = planted_scalars(rng, N, 2)
            i_enc, i_el = indexed_fold_by_scalar_mul(self.o, bases, idx, ik)
            return dict(bases=bases, k=k, n=N, want=dict(enc=enc, el=el), idx=np.ascontiguousarray(idx), ik=ik,
                        i_want=dict(enc=i_enc, el=i_el))
        return self.get("fixed3", make)

    def fixed_seg(self, n, g, b):
        def make():
            rng = np.random.default_rng(101)
            bases = fl.make_bases(self.o, rng, 101, b)
            k = fl.make_scalars(rng, n, 101, g, b)
            enc, el = fl.oracle_fold(self.o, bases, k, n, 101)
            return dict(bases=bases, k=k, n=n, want=dict(enc=enc, el=el))
        return self.get(("fixed_seg", n, g, b), make)

    def buckets(self, n, m, c, encoded=False):
        def make():
            pts, k, _ = bc.make_case(self.o, np.random.default_rng(900 + 100 * n + m + encoded), n, m, c, encoded=encoded)
            enc, el, st = oracle_fold(self.o, pts, k, m)
            return dict(pts=pts, k=k, m=m, n=n, c=c, want=dict(enc=enc, el=el, st=st))
        return self.get(("buckets", n, m, c, encoded), make)

    def msm(self, n):
        def make():
            rng = np.random.default_rng(n)
            pts = self._points(rng, n)
            pts[7::501, 8:12] = 0
            k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            enc, el, _ = oracle_fold(self.o, pts, k, n)
            return dict(pts=pts, k=k, n=n, want=dict(enc=enc, el=el))
        return self.get(("msm", n), make)


SEG_SUMS = 29                                                    # 29 x 101 = 2929 terms


class Maker:
    """The calls of one context: device copies and registrations, made before any gate."""

    def __init__(self, side, cases):
        self.side, self.cases, self.ctx, self.handles, self.seg_plan = side, cases, side.ctx, {}, None

    def handle(self, key, bases, long=False):
        if key not in self.handles:
            self.handles[key] = (self.ctx.fixed_bases_long if long else self.ctx.fixed_bases)(bases, comb_bits=8)
        return self.handles[key]

    def close(self):
        for fb in self.handles.values():
            fb.close()
        self.handles = {}

    def _sums(self, symbol, c, extra=(), encoded=False):
        s, want = self.side, c["want"]
        outs = [("enc", c["n"]), ("el", c["n"])] + ([("st", c["n"] * c["m"])] if encoded else [])
        return Call(s, symbol, [s.dev(c["pts"]), s.dev(c["k"]), c["m"], c["n"], *extra], outs, want)

    def small(self, m, encoded=False):
        return self._sums("d377_batch_msm_small_encoded_dev" if encoded else "d377_batch_msm_small_dev", self.cases.small(m, encoded),
                          encoded=encoded)

    def long(self, n, m, encoded=False):
        return self._sums("d377_batch_long_msm_encoded_resident" if encoded else "d377_batch_long_msm_resident",
                          self.cases.long(n, m, encoded), encoded=encoded)

    def buckets(self, n, m, c, encoded=False):
        return self._sums("d377_batch_bucket_msm_encoded_resident" if encoded else "d377_batch_bucket_msm_resident",
                          self.cases.buckets(n, m, c, encoded), extra=(c,), encoded=encoded)

    def mixed(self, v, t, encoded=False):
        s, c = self.side, self.cases.mixed(v, t, encoded)
        fb = self.handle(("mixed", v, t), c["bases"])
        outs = [("enc", N), ("el", N)] + ([("st", N * v)] if encoded else []) + [("ver",)]
        return Call(s, "d377_batch_msm_mixed_encoded_resident" if encoded else "d377_batch_msm_mixed_resident",
                    [fb._h, s.dev(c["idx"]), s.dev(c["fk"]), t, s.dev(c["pts"]), s.dev(c["vk"]), v, N], outs, c["want"])

    def long_indexed(self, n, m):
        s, c = self.side, self.cases.long_indexed(n, m)
        return Call(s, "d377_batch_long_msm_indexed_resident", [s.dev(c["pool"]), POOL, s.dev(c["idx"]), s.dev(c["k"]), m, n],
                    [("enc", n), ("el", n), ("ver",)], c["want"])

    def fixed_dense(self):
        s, c = self.side, self.cases.fixed3()
        fb = self.handle("fixed3", c["bases"])
        return Call(s, "d377_batch_fixed_msm_resident", [fb._h, s.dev(c["k"]), N], [("enc", N), ("el", N)], c["want"])

    def fixed_indexed(self):
        s, c = self.side, self.cases.fixed3()
        fb = self.handle("fixed3", c["bases"])
        return Call(s, "d377_batch_fixed_msm_indexed_resident", [fb._h, s.dev(c["idx"]), s.dev(c["ik"]), 2, N],
                    [("enc", N), ("el", N), ("ver",)], c["i_want"])

    def fixed_seg(self):
        """101 bases at 8 bits, SEG_SUMS sums: far fewer sums than resident lanes, so every sum is cut into segments."""
        s = self.side
        if self.seg_plan is None:                                # (the cut depends on the device's lanes: asked of a probe handle)
            with self.ctx.fixed_bases_long(self.cases._points(np.random.default_rng(1), 101), comb_bits=8) as probe:
                self.seg_plan = probe.long_plan(SEG_SUMS)
        g, b = self.seg_plan
        assert g > 1                                             # more than one segment: the partials, the fold levels
        c = self.cases.fixed_seg(SEG_SUMS, g, b)
        fb = self.handle("seg", c["bases"], long=True)
        assert fb.long_plan(SEG_SUMS) == (g, b)
        return Call(s, "d377_batch_fixed_long_msm_resident", [fb._h, s.dev(c["k"]), SEG_SUMS], [("enc", SEG_SUMS), ("el", SEG_SUMS)],
                    c["want"])

    def msm(self, n):
        s, c = self.side, self.cases.msm(n)
        return Call(s, "d377_msm_dev", [s.dev(c["pts"]), s.dev(c["k"]), n], [("enc", 1), ("el", 1)], c["want"])


class Env:
    pass


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def cases(oracle):
    return Cases(oracle)


def _tuned(ctx):
    for key, v in TUNING.items():
        ctx.set_tuning(key, v)
    return ctx


@pytest.fixture(scope="module")
def env(torch, oracle, cases):
    """The module's context with the wave routes off, the gate, and the streams: s1 such that the context's private stream
    (the host forms) runs beside a gate on it, s2 independent of s1 by the control."""
    import decaf377_amd as d
    e = Env()
    e.torch, e.oracle = torch, oracle
    e.ctx = _tuned(d.Context([0], comb_lazy=True))
    e.gate = Gate(torch, GATE_MS)
    c = cases.small(1)

    def host_call():
        e.ctx.msm_small(c["pts"], c["k"], 1)

    host_call()                                                  # (the staging buffers have grown: no hipFree behind the gate)
    e.private_independent = False
    for _ in range(4):
        e.side = Side(torch, e.ctx)
        if runs_beside(torch, e.gate, e.side.stream, host_call):
            e.private_independent = True
            break
    e.s1 = e.side.stream
    s2, which = pick_independent_stream(torch, e.gate, e.s1)
    e.independent = s2 is not None
    e.side.stream2 = e.s2 = s2 if s2 is not None else torch.cuda.Stream(device="cuda:0")
    e.mk = Maker(e.side, cases)
    print("\ngate: %d kernels, %.1f ms measured (at least %.0f asked); s2 = candidate %s, independent of s1: %s; "
          "the context's private stream independent of s1: %s"
          % (e.gate.count, e.gate.measured_ms, GATE_MS, which, e.independent, e.private_independent))
    yield e
    torch.cuda.synchronize()
    e.mk.close()
    claimed, _, gave_up = e.ctx.health()
    e.ctx.close()
    assert (claimed, gave_up) == (0, 0)


def test_the_gate_is_long_enough_and_the_streams_are_independent(env):
    """What the fixture found, as a result of its own: the cases below rest on it."""
    assert env.gate.measured_ms >= GATE_MS
    if not (env.independent and env.private_independent):
        pytest.skip("no stream independent of s1: ordering not checked")


def _event(env, stream):
    ev = env.torch.cuda.Event()
    ev.record(stream)
    return ev


def _healthy(ctx):
    claimed, _, gave_up = ctx.health()
    assert (claimed, gave_up) == (0, 0)


def _warm(env, *calls):
    """Every call once with nothing in flight: the areas grow here, the results are the oracle's, the outputs are prefilled again."""
    for c in calls:
        c.enqueue(env.s1)
    env.torch.cuda.synchronize()
    for c in calls:
        c.check(env.oracle, "alone")
        c.reset()


def _pair(env, a, b):
    """Steps 2 .. 7 for A on s1 behind the gate and B on s2."""
    torch = env.torch
    same = GUARD_OF[a.symbol][0] == GUARD_OF[b.symbol][0]
    _warm(env, a, b)
    gate_end = env.gate.start(env.s1)
    a.enqueue(env.s1)
    ev_a = _event(env, env.s1)
    b.enqueue(env.s2)
    _event(env, env.s2)
    assert not gate_end.query(), "gate too short"
    if same:
        env.s2.synchronize()
        handed_over = ev_a.query()
        if env.independent:
            assert handed_over, "%s finished on s2 while %s still waits behind the gate: no hand-over" % (b.symbol, a.symbol)
    torch.cuda.synchronize()
    a.check(env.oracle, "A")
    b.check(env.oracle, "B")
    _healthy(env.ctx)
    if same and not env.independent:
        pytest.skip("no stream independent of s1: ordering not checked")


def _both_orders(order, x, y):
    return (x, y) if order == "ab" else (y, x)


# ---- same-guard pairs: the ordering and the results ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ab", "ba"])
def test_small_and_mixed_sums_lay_the_table_scratch_out_differently(env, order):
    """8 tables per lane against 1."""
    _pair(env, *_both_orders(order, env.mk.small(8), env.mk.mixed(1, 1)))


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_long_sums_and_segmented_fixed_sums_share_the_partials(env, order):
    _pair(env, *_both_orders(order, env.mk.long(5, 129), env.mk.fixed_seg()))


def test_long_indexed_sums_and_long_sums_of_another_length(env):
    _pair(env, env.mk.long_indexed(5, 65), env.mk.long(4, 33))


def test_dense_and_indexed_fixed_sums_share_the_lane_sets(env):
    _pair(env, env.mk.fixed_dense(), env.mk.fixed_indexed())


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_bucket_sums_and_one_long_sum_share_the_msm_workspace(env, order):
    assert env.ctx.get_tuning("msm_small_max") == 0              # 3000 points take the bucket pipeline
    _pair(env, *_both_orders(order, env.mk.buckets(3, 40, 8), env.mk.msm(3000)))


def test_bucket_sums_of_three_passes_and_of_one(env):
    assert env.ctx.msm_buckets_plan(9, 33, 16)["passes"] == 3
    _pair(env, env.mk.buckets(9, 33, 16), env.mk.buckets(3, 5, 4))


# ---- cross-guard pairs: they need not queue; both are right ----------------------------------------------------------------------
def test_bucket_sums_beside_small_sums(env):
    a, b = env.mk.buckets(3, 40, 8), env.mk.small(8)
    assert GUARD_OF[a.symbol][0] != GUARD_OF[b.symbol][0]
    _pair(env, a, b)


def test_bucket_sums_of_encodings_beside_mixed_sums_of_encodings(env):
    a, b = env.mk.buckets(3, 40, 8, encoded=True), env.mk.mixed(1, 1, encoded=True)
    assert a.want["st"].any() and b.want["st"].any()             # invalid Encodings were there to report
    assert GUARD_OF[a.symbol][0] != GUARD_OF[b.symbol][0]
    _pair(env, a, b)


# ---- a host form behind a resident call ------------------------------------------------------------------------------------------
def _host_behind(env, a, host_call, want):
    """A on s1 behind the gate, then the host-pointer call B (the context's private stream): it returns after A."""
    _warm(env, a)
    first = host_call()                                          # alone: the staging buffers grow here, not behind the gate
    gate_end = env.gate.start(env.s1)
    a.enqueue(env.s1)
    ev_a = _event(env, env.s1)
    assert not gate_end.query(), "gate too short"
    got = host_call()
    handed_over = ev_a.query()
    if env.private_independent:
        assert handed_over, "the host form returned while %s still waits behind the gate: no hand-over" % a.symbol
    env.torch.cuda.synchronize()
    a.check(env.oracle, "A")
    for g in (first, got):
        _same(env.oracle, "host form", dict(enc=g[0], el=g[1]), want)
    _healthy(env.ctx)
    if not env.private_independent:
        pytest.skip("no stream independent of s1: ordering not checked")


def test_host_long_sums_queue_behind_resident_small_sums(env, cases):
    c = cases.long(5, 129)
    _host_behind(env, env.mk.small(8), lambda: env.ctx.msm_long(c["pts"], c["k"], c["m"], elements=True), c["want"])


def test_host_bucket_sums_queue_behind_resident_bucket_sums(env, cases):
    c = cases.buckets(3, 5, 4)
    _host_behind(env, env.mk.buckets(9, 33, 16),
                 lambda: env.ctx.msm_buckets(c["pts"], c["k"], c["m"], elements=True, window_bits=c["c"]), c["want"])


# ---- growth while the old area is in flight --------------------------------------------------------------------------------------
def _growth(env, cases, make_a, make_b, grows=None):
    """A fresh context.  A behind the gate allocates the area; B on s2 outgrows it: its reserve drains the guard on the host, so
    when B's call returns A has finished.  Then both are right, and A again, in the larger area, gives the same bytes."""
    import decaf377_amd as d
    torch = env.torch
    _warm(env, make_a(env.mk), make_b(env.mk))                   # on the module's context: the kernels are loaded
    ctx = _tuned(d.Context([0], comb_lazy=True))
    mk = Maker(Side(torch, ctx), cases)
    try:
        assert grows is None or grows(ctx)
        a, b, again = make_a(mk), make_b(mk), make_a(mk)
        torch.cuda.synchronize()
        gate_end = env.gate.start(env.s1)
        a.enqueue(env.s1)
        ev_a = _event(env, env.s1)
        assert not gate_end.query(), "gate too short"
        b.enqueue(env.s2)
        assert ev_a.query(), "%s outgrew the area and returned while %s still waits behind the gate: no drain" % (b.symbol, a.symbol)
        torch.cuda.synchronize()
        got_a = a.check(env.oracle, "A")
        b.check(env.oracle, "B")
        again.enqueue(env.s1)
        torch.cuda.synchronize()
        got_again = again.check(env.oracle, "A again")
        for kind in got_a:
            assert (got_a[kind] == got_again[kind]).all(), kind
        _healthy(ctx)
    finally:
        torch.cuda.synchronize()
        mk.close()
        ctx.close()


def test_table_scratch_grows_under_a_call_in_flight(env, cases):
    _growth(env, cases, lambda mk: mk.small(1), lambda mk: mk.small(8))


def test_partials_grow_under_a_call_in_flight(env, cases):
    assert 5 * lc.plan(600)[0] > 2 * 3 * lc.plan(17)[0]          # B's partial sums against A's
    _growth(env, cases, lambda mk: mk.long(3, 17), lambda mk: mk.long(5, 600))


def test_msm_workspace_grows_under_a_call_in_flight(env, cases):
    _growth(env, cases, lambda mk: mk.buckets(3, 17, 6), lambda mk: mk.buckets(5, 600, 6),
            lambda ctx: ctx.msm_buckets_plan(5, 600, 6)["workspace_bytes"] > 2 * ctx.msm_buckets_plan(3, 17, 6)["workspace_bytes"])


# ---- destroy while in flight -----------------------------------------------------------------------------------------------------
def test_destroy_waits_for_the_sums_in_flight_on_the_combs(env, cases):
    torch, s, c = env.torch, env.side, cases.fixed3()
    _warm(env, env.mk.fixed_dense())
    a = Call(s, "d377_batch_fixed_msm_resident", [0, s.dev(c["k"]), N], [("enc", N), ("el", N)], c["want"])   # (the handle: below)
    fb = env.ctx.fixed_bases(c["bases"], comb_bits=8)            # once without a gate: whatever a first handle allocates stays
    a.ins[0] = fb._h
    _warm(env, a)
    fb.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    fb = env.ctx.fixed_bases(c["bases"], comb_bits=8)            # the fresh handle; the call's tensors are those of the first run
    a.ins[0] = fb._h
    gate_end = env.gate.start(env.s1)
    a.enqueue(env.s1)
    ev_a = _event(env, env.s1)
    assert not gate_end.query(), "gate too short"
    fb.close()                                                   # d377_fixed_bases_destroy
    assert ev_a.query(), "d377_fixed_bases_destroy returned while the sums still wait behind the gate: the combs were freed under them"
    torch.cuda.synchronize()
    a.check(env.oracle, "A")
    free1 = torch.cuda.mem_get_info(0)[0]
    assert abs(free0 - free1) <= 1 << 20, (free0, free1)         # as test_create_destroy_returns_device_memory measures it
    _healthy(env.ctx)


# ---- two host threads, one context -----------------------------------------------------------------------------------------------
def test_two_host_threads_alternate_four_units_on_one_context(env, cases):
    """ctypes releases the interpreter lock; the context's mutex serialises the calls, the guards their kernels."""
    ctx, o = env.ctx, env.oracle
    sm, lg, bk, mx = cases.small(8), cases.long(5, 129), cases.buckets(3, 40, 8), cases.mixed(1, 1)
    fb = env.mk.handle(("mixed", 1, 1), mx["bases"])
    jobs = {
        1: [(lambda: ctx.msm_small(sm["pts"], sm["k"], 8, elements=True), sm["want"]),
            (lambda: ctx.msm_long(lg["pts"], lg["k"], lg["m"], elements=True), lg["want"])],
        2: [(lambda: ctx.msm_buckets(bk["pts"], bk["k"], bk["m"], elements=True, window_bits=bk["c"]), bk["want"]),
            (lambda: fb.msm_mixed(mx["idx"], mx["fk"], mx["pts"], mx["vk"], elements=True), mx["want"])],
    }
    results, errors = {1: [], 2: []}, []

    def worker(t):
        try:
            for r in range(6):
                call, want = jobs[t][r % 2]
                results[t].append((call(), want))
        except Exception as e:                                    # noqa: BLE001 -- reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in (1, 2):
        assert len(results[t]) == 6
        for r, (got, want) in enumerate(results[t]):
            _same(o, ("thread", t, "call", r), dict(enc=got[0], el=got[1]), want)
    _healthy(ctx)
