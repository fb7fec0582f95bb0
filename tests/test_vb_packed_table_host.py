"""CPU check of the variable-base window table's packed slots: a slot is the field value as a 256-bit integer (8 words, four
slots = one 128-byte entry; fqs29.hpp fes_pack256 / fes_unpack256, d377.hip GlobalTab).

tests/cpp/vb_packed_table.cpp is a stand-alone program over the product's headers, built with g++: plain, with
-fsanitize=address,undefined (run as an ordinary executable), and with -DD377_BOUNDS (every precondition asserted: the pack's
own, and every column of every product that reads an unpacked entry).  It is fed over standard input; this file checks the
VALUES it prints with Python's integers: packed = value + 9q or value - 4q exactly, the unpacked limbs in their ranges and summing to
the packed integer, and the scalar multiplication through the packed table against the model's vectors (tests/golden/)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "vb_packed_table.cpp")
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
Q_TOP = Q >> 232                                         # what one q contributes to limb 8
RB = 29
BIG_TOP = 5 << 20                                        # fqs29.hpp PACK_BIG_TOP


def _build(name, flags):
    exe = os.path.join(ROOT, "build", "tests", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    srcs = [SRC] + [os.path.join(SIM_DIR, f) for f in ("vb_signed_sqrt_sim.cpp", "sim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-I" + CSRC] + flags + [SRC, "-o", exe])
    return exe


def _run(exe, lines, timeout=600):
    res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, (res.returncode, res.stderr[-3000:])
    out = res.stdout.split("\n")
    assert out[-2] == "OK"
    return out[:-2]


def _limbs(v):
    """v >= 0 as nine 29-bit digits (the top one takes the rest)"""
    return [(v >> (RB * i)) & ((1 << RB) - 1) for i in range(8)] + [v >> (RB * 8)]


def _value(l):
    return sum(x << (RB * i) for i, x in enumerate(l))


def _pack_inputs():
    rows = []
    # by value: 0, 1, q - 1, q, q + 1, 2q - 1, both sides of the top limb at which the pack turns from + 9q to - 4q, and both
    # ends of what a slot can take: -9q (below) and 2^256 + 4q - 1
    for v in (0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, (BIG_TOP << 232) - 1, BIG_TOP << 232, (1 << 256) + 4 * Q - 1):
        rows.append(_limbs(v))
    for v in (1, Q, 2 * Q + 1, 4 * Q, 9 * Q):                    # negative values as negated digits
        rows.append([-x for x in _limbs(v)])
    # per limb: limbs 0..7 at 0, 2^29 - 1 and the lazy edge 2^30 - 1 (all together, then one at a time), under a signed top
    # limb at both ends of what a product returns (fqs29.hpp sbound_set_product: value in (-q - eps, q + eps], top =
    # floor(value / 2^232) -+ 1) and of what a table entry, a sum or a difference of two products, can be
    # -- and of a sum or a difference of two carried fe coordinates (entry 1: -8.67q .. 17.32q), with the turning point's sides
    tops = [0, -(Q_TOP + 2), Q_TOP + 2, -2 * (Q_TOP + 2), 2 * (Q_TOP + 2), BIG_TOP - 1, BIG_TOP, -8 * Q_TOP - 2 * Q_TOP // 3,
            17 * Q_TOP + Q_TOP // 3]
    for top in tops:
        for edge in (0, (1 << 29) - 1, (1 << 30) - 1):
            rows.append([edge] * 8 + [top])
            for i in range(8):
                rows.append([edge if k == i else 0 for k in range(8)] + [top])
        rows.append([-((1 << 29) - 1)] * 8 + [top])       # a difference's limbs: down to -(2^29 - 1)
    return rows


def _check_pack(rows, out):
    assert len(out) == len(rows)
    for l, line in zip(rows, out):
        f = line.split()
        assert f[0] == "P" and len(f) == 1 + 8 + 9
        packed = sum(int(w, 16) << (32 * j) for j, w in enumerate(f[1:9]))
        un = [int(x) for x in f[9:]]
        v = _value(l)
        assert -9 * Q <= v < (1 << 256) + 4 * Q, "test input outside what a slot takes"
        assert packed == (v + 9 * Q if l[8] < BIG_TOP else v - 4 * Q), (l, hex(packed))
        assert 0 <= packed < (1 << 256)
        assert all(0 <= x < (1 << 29) for x in un[:8]) and 0 <= un[8] < (1 << 24), un
        assert _value(un) == packed and _value(un) % Q == v % Q


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "vb_packed_table_vectors.json")) as f:
        return json.load(f)


def _mul_lines(golden, vectors):
    pts = golden["points"]
    d_cases = golden["digit_cases"]
    s_cases = golden["scalar_cases"] + [dict(c, point=c["point"]) for c in vectors["scalar_mul_var"]]
    lines = ["D %s %s" % (pts[c["point"]], c["digits"]) for c in d_cases]
    lines += ["S %s %s" % (c["point"], c["scalar"]) for c in s_cases]
    return d_cases, s_cases, lines


@pytest.fixture(scope="module")
def plain_run(golden, vectors):
    """one run of the plain build over every input: shared by the tests below"""
    exe = _build("vb_packed_table", ["-O1", "-DD377_HOST_OUTLINE", "-DD377_FB_BITS=8"])
    rows = _pack_inputs()
    d_cases, s_cases, lines = _mul_lines(golden, vectors)
    out = _run(exe, ["P " + " ".join(str(x) for x in l) for l in rows] + lines)
    return rows, d_cases, s_cases, out


def test_pack_unpack_values_and_ranges(plain_run):
    rows, _, _, out = plain_run
    _check_pack(rows, out[:len(rows)])


def test_digits_cover_every_table_entry(golden):
    """the digit cases use every digit -8 .. 7 (entry 8 is read for -8 only: fr_digit never gives +8), digit 0 and a top digit 1"""
    seen, tops = set(), set()
    for c in golden["digit_cases"]:
        v = int.from_bytes(bytes.fromhex(c["digits"]), "little")
        n = [(v >> (4 * i)) & 15 for i in range(64)]
        seen |= {(x ^ 8) - 8 for x in n[:63]}
        tops.add(n[63])
    assert seen == set(range(-8, 8)) and tops == {0, 1}
    assert set(c["point"] for c in golden["digit_cases"]) == {"identity", "generator", "rm1_generator"}


def test_scalar_mul_packed_table_equals_limb_table_and_model(plain_run):
    rows, d_cases, s_cases, out = plain_run
    out = out[len(rows):]
    assert len(out) == len(d_cases) + len(s_cases)
    for c, line in zip(d_cases, out[:len(d_cases)]):
        f = line.split()
        assert f[0] == "D" and f[1] == f[2] == c["enc"], (c, line)
    for c, line in zip(s_cases, out[len(d_cases):]):
        f = line.split()
        assert f[0] == "S"
        assert f[1] == f[3] == f[5] == c["enc"], (c, line)              # lane kernel, Element kernel, limb table
        assert (int(f[2]) != 0) == (int(f[4]) != 0) == (int(f[6]) != 0) == (c["status"] != 0), (c, line)


def test_sanitized_build_runs_clean(golden, vectors):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain executable; a shorter input"""
    exe = _build("vb_packed_table_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                         "-DD377_HOST_OUTLINE", "-DD377_FB_BITS=8"])
    rows = _pack_inputs()
    d_cases, s_cases, lines = _mul_lines(golden, vectors)
    keep = lines[:len(d_cases)][::3] + lines[len(d_cases):][::5]
    out = _run(exe, ["P " + " ".join(str(x) for x in l) for l in rows] + keep)
    _check_pack(rows, out[:len(rows)])
    assert len(out) == len(rows) + len(keep)


def test_bounds_build_walks_pack_unpack_and_the_products(golden, vectors):
    """-DD377_BOUNDS: a violated precondition aborts.  Pack inputs inside what the chain produces, then the window loop over the
    packed table (every product that reads an unpacked entry checks its columns against +-2^63)."""
    exe = _build("vb_packed_table_bounds", ["-O1", "-g", "-DD377_BOUNDS", "-DD377_FB_BITS=8"])
    rows = _pack_inputs()
    d_cases, s_cases, lines = _mul_lines(golden, vectors)
    keep = lines[:len(d_cases)][::4] + lines[len(d_cases):][::7]
    out = _run(exe, ["P " + " ".join(str(x) for x in l) for l in rows] + keep, timeout=1800)
    _check_pack(rows, out[:len(rows)])
    assert len(out) == len(rows) + len(keep)
