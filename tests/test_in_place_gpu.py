"""In-place calls on device buffers: every map of tests/_in_place_cases.py's table, on every route it has.

include/decaf377_amd.h allows an output buffer to be an input buffer of the same record size, and says that until a call
completes its output records may hold intermediate values: the chunked kernels park prefix products in the caller's output
records.  So every route must have read record i of every input before anything writes record i of an output, and a clamped idle
lane may only re-read a record its own wave owns.  Here that is checked, not argued: for every row of the table, every input the
output may be, every route (forced through the tuning keys at sizes that split a wave, a quad group, a workgroup round and a
chunk unevenly) the call on fresh buffers gives the oracle's bytes for all n records, and the same call with the output pointer
equal to an input's -- and to both inputs' -- gives exactly those bytes, leaves the other inputs alone and writes nothing outside
its n records.  Every comparison is exact.  Then the two paths around the kernels: the host path's pipelined copies into and out
of one host array, and the peer-copy path, "in place for the root".  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import _in_place_cases as cases

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
COUNTS = {"cases": 0, "launches": 0, "pairs": set()}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    import decaf377_amd as d
    c = d.Context([0], comb_bits=18)                   # (every comb width gives the same bytes; 18 bits are 0.24 GB)
    yield c
    torch_mod.cuda.synchronize()
    assert c.health()[0] == 0 and c.health()[2] == 0   # after the file's tests: no lane set claimed, nobody gave up
    c.close()


@pytest.fixture(scope="module")
def plan():
    return cases.plan_lib()


def to_dev(torch, a):
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


class Guarded:
    """A copy of `src` as records 1 .. n of an allocation of n + 2: a sentinel record (0xA5) at each end.  One record is 32 or 128
    bytes, so the copy keeps the 16-byte alignment the device-pointer calls ask for."""

    def __init__(self, torch, src):
        n = int(src.shape[0])
        self.rec = int(src[0].numel()) * src.element_size() if n else 32
        self.raw = torch.full(((n + 2) * self.rec,), SENTINEL, dtype=torch.uint8, device=src.device)
        self.buf = self.raw[self.rec:(n + 1) * self.rec].view(src.dtype).view(src.shape)
        self.buf.copy_(src)
        assert self.buf.data_ptr() == self.raw.data_ptr() + self.rec and self.buf.data_ptr() % 16 == 0

    def view(self, torch, kind):
        """The same n records as the output array of `kind`: [n, 32] u8, [n, 4] or [n, 16] int64."""
        n = int(self.buf.shape[0])
        flat = self.raw[self.rec:(n + 1) * self.rec]
        return flat.view(n, 32) if kind == "bytes" else flat.view(torch.int64).view(n, 4 if kind == "fq" else 16)

    def intact(self):
        return bool((self.raw[:self.rec] == SENTINEL).all()) and bool((self.raw[-self.rec:] == SENTINEL).all())


def same_bytes(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def call(op, ctx, ins, outs=None):
    """-> (out0, status or None)"""
    COUNTS["launches"] += 1
    res = op.call(ctx, ins, outs)
    res = list(res) if isinstance(res, (list, tuple)) else [res]
    assert len(res) == (2 if op.status else 1)
    return res[0], (res[1] if op.status else None)


def against_oracle(op, oracle, n, out, st, want, wst, tag):
    got = host(out)
    if not op.as_elements:
        assert (got == want).all(), tag
    else:
        # The one large shape: the first and last 300 records and a stride of about 200 in between; every record otherwise.
        sel = np.arange(n) if n <= 4096 else np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), np.arange(0, n, 199)]))
        assert oracle.eq_xyzt(got[sel], want[sel]).all(), tag
        assert (oracle.compress(got[sel]) == oracle.compress(want[sel])).all(), tag
    if op.status:
        assert (host(st) == wst).all(), tag


@pytest.mark.parametrize("key", [op.key for op in cases.OPS])
def test_in_place_on_every_route(ctx, oracle, torch_mod, plan, key):
    torch = torch_mod
    op = cases.BY_KEY[key]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fresh_st = lambda n: torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    batches = {}
    for route, tuning, n in cases.route_cases(op.family, cus):
        tag = (key, route, tuning, n)
        # the route this call takes, by the launcher's own plan for this device and these overrides
        f = cases.planned(plan, op.plan_op, n, cus, tuning)
        assert f["route"] == route, (tag, f)
        if route == "el_uniform":
            assert f["per_lane"] == cases.el_per_lane(n, cus), (tag, f)
        if n not in batches:
            data, want = cases.batch_of(op, oracle, n)
            batches[n] = ([to_dev(torch, a) for a in data], want)
        ins, (want, wst) = batches[n]
        with ctx.tuning(**tuning):
            # 1. out of place, on fresh tensors: the oracle's outputs for all n records
            out, st = call(op, ctx, [x.clone() for x in ins])
            against_oracle(op, oracle, n, out, st, want, wst, tag)
            # 2. in place: out0 is input a's buffer, between two sentinel records; the status tensor is separate
            for a in op.alias:
                mine = [x.clone() for x in ins]
                g = Guarded(torch, mine[a])
                mine[a] = g.buf
                st2 = fresh_st(n) if op.status else None
                res, rst = call(op, ctx, mine, [g.view(torch, op.out)] + ([st2] if op.status else []))
                assert res.data_ptr() == g.buf.data_ptr(), tag
                assert same_bytes(torch, g.view(torch, op.out), out), (tag, "out0 = input %d" % a)
                assert not op.status or torch.equal(rst, st), (tag, "status, out0 = input %d" % a)
                assert all(torch.equal(mine[j], ins[j]) for j in range(len(ins)) if j != a), (tag, "an input that was not aliased changed")
                assert g.intact(), (tag, "a guard record was written")
                COUNTS["cases"] += 1
            # 3. both inputs and the output one buffer: the out-of-place call on two copies of it
            if op.both:
                x = ins[0]
                out2, stb = call(op, ctx, [x.clone(), x.clone()])
                g = Guarded(torch, x)
                st2 = fresh_st(n) if op.status else None
                _, rst = call(op, ctx, [g.buf, g.buf], [g.view(torch, op.out)] + ([st2] if op.status else []))
                assert same_bytes(torch, g.view(torch, op.out), out2), (tag, "out0 = both inputs")
                assert (not op.status or torch.equal(rst, stb)) and g.intact(), (tag, "out0 = both inputs")
                COUNTS["cases"] += 1
        COUNTS["pairs"].add((key, route))
    assert all(ctx.get_tuning(k) is None for k in cases.PLAN_TUNE)
    assert {p for p in COUNTS["pairs"] if p[0] == key} == {p for p in cases.CLAIMED if p[0] == key}


def test_no_claimed_route_was_left_out(ctx):
    """Runs after the matrix: of the (operation, route) pairs claimed for the operations that ran (all of them, unless the run
    selected some), the share that no call above took is zero."""
    claimed = [p for p in cases.CLAIMED if p[0] in {k for k, _ in COUNTS["pairs"]}]
    left_out = set(claimed) - COUNTS["pairs"]
    share = len(left_out) / max(len(claimed), 1)
    print("\nin place: %d (operation, route, size, alias) cases in %d launches; %d of %d claimed (operation, route) pairs left out (%.3f)"
          % (COUNTS["cases"], COUNTS["launches"], len(left_out), len(claimed), share))
    assert share == 0, sorted(left_out)


# ---- the host path: staged copies into and out of ONE host array -------------------------------------------------------------------
def _host_cases(oracle, n):
    """(name, call(ctx, ins, outs), inputs, the input that is the output, oracle on rows) for the four operations of the host path."""
    rng = np.random.default_rng(9200 + n)
    pool_p = oracle.elligator_map_xyzt(rng.integers(0, 256, (1024, 32), dtype=np.uint8))
    pool_q = oracle.double_xyzt(oracle.elligator_map_xyzt(rng.integers(0, 256, (1024, 32), dtype=np.uint8)))
    pool_p[0], pool_q[1] = oracle.identity_xyzt(), oracle.generator_xyzt()
    r0 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    enc = oracle.encode_to_curve(rng.integers(0, 256, (1024, 32), dtype=np.uint8))[rng.integers(0, 1024, n)]
    enc[::1000, 31] |= 0x40                                          # invalid encodings every 1000th record
    a, b = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    P, Qp = pool_p[rng.integers(0, 1024, n)], pool_q[rng.integers(0, 1024, n)]
    return [
        ("encode_to_curve", lambda c, i, o: [c.encode_to_curve(i[0], outs=o)], [r0], 0, lambda i: [oracle.encode_to_curve(i[0])]),
        ("roundtrip", lambda c, i, o: c.roundtrip(i[0], outs=o), [enc], 0, lambda i: list(oracle.roundtrip(i[0]))),
        ("fr_op mul, out = b", lambda c, i, o: c.fr_op("mul", i[0], i[1], outs=o), [a, b], 1, lambda i: list(oracle.fr_op(2, i[0], i[1]))),
        ("add, out = P", lambda c, i, o: [c.add(i[0], i[1], outs=o)], [P, Qp], 0, lambda i: [oracle.add_xyzt(i[0], i[1])]),
    ]


@pytest.mark.parametrize("n", [(1 << 19) + (1 << 18) + 77, 1000])
def test_host_path_in_place(ctx, oracle, n):
    """Host-pointer calls with outs= the input array.  From 2^19 records the host path is pipelined in chunks of 2^18: chunk k + 1
    is read from the host array while chunk k - 1's outputs are written into it; below, one copy in and one copy out.  Each
    result equals the out-of-place call on copies, and the oracle's on the chunk-boundary records and a stride."""
    idx = np.unique(np.concatenate([[0, n - 1], np.arange(0, n, 30011)] + [[m - 1, m] for m in (1 << 18, 1 << 19, 3 << 18) if m < n]))
    for name, run, ins, a, want in _host_cases(oracle, n):
        ref = run(ctx, [x.copy() for x in ins], None)
        mine = [x.copy() for x in ins]
        st = [np.full(n, 0xEE, np.uint8)] if len(ref) == 2 else []
        res = run(ctx, mine, [mine[a]] + st)
        assert res[0] is mine[a] and (mine[a] == ref[0]).all(), name
        assert all((x == y).all() for x, y in zip(res[1:], ref[1:])), name
        assert all((mine[j] == ins[j]).all() for j in range(len(ins)) if j != a), name
        for got, w in zip(ref, want([x[idx] for x in ins])):
            assert (got[idx] == w).all(), name
        if name == "roundtrip":
            assert ref[1].sum() == len(range(0, n, 1000))


# ---- the peer-copy path: d377_batch_sharded_dev, "in place for the root" -----------------------------------------------------------
@pytest.mark.parametrize("ids", [[0, 0], [0, 0, 0]])
def test_sharded_path_in_place(oracle, torch_mod, ids):
    """The seven operations of the table that d377_batch_sharded_dev takes, out0 = in0 and, for the two-input ones, out0 = in1,
    on one GPU listed two and three times (slicing, staging, the event ordering, the gather): byte-identical to the
    single-device out-of-place result, statuses equal, the inputs that were not aliased unchanged."""
    import decaf377_amd as d
    torch = torch_mod
    c = d.Context(ids, comb_bits=18)
    try:
        for n in (17, 1000, 4099):
            for name, export in cases.SHARDED.items():
                op = next(o for o in cases.OPS if o.export == export)
                data, (want, wst) = cases.batch_of(op, oracle, n)
                ins = [to_dev(torch, x) for x in data]
                tag = (ids, n, name)
                out, st = call(op, c, [x.clone() for x in ins])       # one device, out of place
                against_oracle(op, oracle, n, out, st, want, wst, tag)
                for a in op.alias:
                    mine = [x.clone() for x in ins]
                    g = Guarded(torch, mine[a])
                    mine[a] = g.buf
                    st2 = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")] if op.status else []
                    res = c.sharded(name, *mine, outs=[g.view(torch, op.out)] + st2)
                    assert same_bytes(torch, res[0], out) and res[0].data_ptr() == g.buf.data_ptr(), (tag, a)
                    assert not op.status or torch.equal(res[1], st), (tag, a)
                    assert all(torch.equal(mine[j], ins[j]) for j in range(len(ins)) if j != a) and g.intact(), (tag, a)
        torch.cuda.synchronize()
        for dev in range(len(ids)):
            assert c.health(dev)[0] == 0 and c.health(dev)[2] == 0
    finally:
        c.close()
