"""Scalars built from their signed digits, for the CPU and the GPU tests of the digit edges.

Every scalar-consuming kernel recodes its scalar h (k mod r, or k / 2 mod r where the kernel halves) into signed digits,
window by window with a running carry: digit = window value + carry, and from 2^(w-1) up the digit is taken 2^w lower
and carries one into the next window.  The top window is not wrapped.  That recoding is unique, so a scalar can be
written down from the digits a test wants -- entry 2^(B-1) of a comb window, the last bucket of an MSM window, nibble 8
of a Straus chain -- and the test can assert, before any kernel runs, which entry and which bucket each case reaches.

Plain Python on big integers; nothing here is derived from the C++ (decaf377_amd/csrc: fb_digit, msm_digit,
fr_recode_signed16), which tests/test_digit_edges_host.py checks against this restatement.

A layout is a list of (first_bit, width) pairs, least significant window first:
  comb(B)  the fixed-base combs (FbShape): ceil(252 / B) windows of B bits
  msm(c)   the bucket MSM (win_shape): ceil(252 / c) windows that tile the 252 bits, the wide ones (c bits) first,
           then windows of c - 1 bits
  w4()     the Straus chains and the variable-base kernel: 63 four-bit windows and the carry window above them
"""
import numpy as np

R = 2111115437357092606062206234695386632838870926408408195193685246394721360383
COMB_WIDTHS = (8, 12, 16, 18, 21, 23)
MSM_WIDTHS = tuple(range(4, 19))
FB_RUN = 16                                            # entries a thread of the comb builder makes in one run


def comb(B):
    return [(B * i, B) for i in range(-(-252 // B))]


def msm(c):
    W = -(-252 // c)
    nwide = W - (W * c - 252)
    widths = [c if w < nwide else c - 1 for w in range(W)]
    return [(sum(widths[:w]), widths[w]) for w in range(W)]


def w4():
    return [(4 * i, 4) for i in range(64)]


def top_index(layout):
    """The highest window a scalar below r can reach: the one that holds the top bit of r - 1."""
    top_bit = (R - 1).bit_length() - 1
    return max(i for i, (fb, _) in enumerate(layout) if fb <= top_bit)


def lo(w):
    return -(1 << (w - 1))


def hi(w):
    return (1 << (w - 1)) - 1


def raw_windows(layout, h):
    """The unsigned window values of h: what a kernel masks out of the scalar words before the carry is added."""
    last = len(layout) - 1
    return [(h >> fb) if i == last else (h >> fb) & ((1 << w) - 1) for i, (fb, w) in enumerate(layout)]


def recode(layout, h):
    """The signed digits of h: digit = window + carry; from 2^(w-1) up it is taken 2^w lower and carries.  The last
    window of the layout takes the carry and is not wrapped."""
    out, carry, last = [], 0, len(layout) - 1
    for i, v in enumerate(raw_windows(layout, h)):
        d = v + carry
        carry = 0
        if i != last and d >= 1 << (layout[i][1] - 1):
            d -= 1 << layout[i][1]
            carry = 1
        out.append(d)
    return out


def recode_rows(layout, hb):
    """recode for many scalars at once: hb is [n, 32] u8, the little-endian bytes of n values of h below 2^252.  Returns
    [n, windows] int64.  (The sweeps' plans hold a million scalars; tests/test_digit_edges_host.py holds this against
    recode.)"""
    words = np.ascontiguousarray(hb).view("<u4").reshape(-1, 8).astype(np.uint64)
    assert not (words[:, 7] >> np.uint64(28)).any()
    out = np.zeros((words.shape[0], len(layout)), np.int64)
    carry = np.zeros(words.shape[0], np.int64)
    last = len(layout) - 1
    for i, (fb, w) in enumerate(layout):
        wi, sh = fb >> 5, fb & 31
        v = words[:, wi] >> np.uint64(sh)
        if wi + 1 < 8:
            v = v | (words[:, wi + 1] << np.uint64(32 - sh))       # 64 bits from the window's first bit: a window is at most 23
        assert w <= 32
        if i != last:
            v = v & np.uint64((1 << w) - 1)
        else:
            v = v & np.uint64((1 << 32) - 1)                       # the rest of the scalar: below 2^252, and the last window starts at 220 or above
            assert fb >= 220
        d = v.astype(np.int64) + carry
        wrap = (d >= (1 << (w - 1))) if i != last else np.zeros(d.shape, bool)
        out[:, i] = d - (wrap.astype(np.int64) << w)
        carry = wrap.astype(np.int64)
    return out


def from_digits(layout, d):
    assert len(d) == len(layout)
    h = sum(dv << fb for dv, (fb, _) in zip(d, layout))
    assert 0 <= h < R, h
    assert recode(layout, h) == list(d), (d, recode(layout, h))
    return h


def top_max(layout):
    """The largest digit the top window takes for a scalar below r (the recoding's top digit grows with h)."""
    return recode(layout, R - 1)[top_index(layout)]


def scalar(h, halved, plus_r=False):
    """The 32 bytes a caller passes so that the kernel walks h: k = 2 h mod r for a kernel that walks k / 2 mod r, h
    itself otherwise; plus_r: k + r (below 2^252), so that the reduction mod r runs before the recoding."""
    assert 0 <= h < R
    k = (2 * h) % R if halved else h
    if plus_r:
        k += R
    return np.frombuffer(k.to_bytes(32, "little"), np.uint8).copy()


def scalars(hs, halved, plus_r=False):
    return np.stack([scalar(h, halved, plus_r) for h in hs]) if len(hs) else np.zeros((0, 32), np.uint8)


def _zeros(layout):
    return [0] * len(layout)


def one_window_cases(layout):
    """For every window below the top: the digits lo, lo + 1, -1, 1, hi alone (a negative digit with the 1 above it that
    makes the scalar positive), lo and hi with a carry arriving from a -1 below, and the digit 0 that is all ones plus a
    carry."""
    top = top_index(layout)
    out = []
    for i in range(top):
        w = layout[i][1]
        for name, v in (("lo", lo(w)), ("lo+1", lo(w) + 1), ("-1", -1), ("1", 1), ("hi", hi(w))):
            d = _zeros(layout)
            d[i] = v
            if v < 0:
                d[i + 1] = 1
            out.append(("w%d:%s" % (i, name), d))
        if i >= 1:
            for name, v in (("lo<carry", lo(w)), ("hi<carry", hi(w)), ("ones+carry", 0)):
                d = _zeros(layout)
                d[i - 1], d[i], d[i + 1] = -1, v, 1
                out.append(("w%d:%s" % (i, name), d))
    return out


def top_cases(layout):
    """The top window at 1, at the largest window value of a scalar below r and at its largest digit, each with and
    without a carry arriving from a negative digit below; and r - 1 itself."""
    top = top_index(layout)
    wb = layout[top - 1][1]
    T, M = (R - 1) >> layout[top][0], top_max(layout)
    out = []
    for v in sorted({1, T, M}):
        for name, below in (("alone", 0), ("<-1", -1), ("<lo", lo(wb))):
            d = _zeros(layout)
            d[top], d[top - 1] = v, below
            h = sum(dv << fb for dv, (fb, _) in zip(d, layout))
            if 0 <= h < R and recode(layout, h) == d:          # T + 1 is reached only over a carry; T alone may pass r
                out.append(("top:%d%s" % (v, name), d))
    out.append(("top:r-1", recode(layout, R - 1)))
    return out


def all_window_cases(layout):
    """Every window below the top at lo, at hi, and alternating between the two (both phases)."""
    top = top_index(layout)
    out = []
    for name, pick in (("all-lo", lambda i, w: lo(w)), ("all-hi", lambda i, w: hi(w)),
                       ("lo-hi", lambda i, w: lo(w) if i % 2 == 0 else hi(w)), ("hi-lo", lambda i, w: hi(w) if i % 2 == 0 else lo(w))):
        d = _zeros(layout)
        for i in range(top):
            d[i] = pick(i, layout[i][1])
        d[top] = 1
        out.append((name, d))
    d = _zeros(layout)
    for i in range(top):
        d[i] = hi(layout[i][1])
    out.append(("all-hi,top0", d))
    return out


def run_entries(B):
    """Comb entries at the edges of the builder's runs of FB_RUN: the end of the first run and the start of the second,
    and the last full run with the lone entry 2^(B-1) after it."""
    e = 1 << (B - 1)
    return sorted(set([FB_RUN - 1, FB_RUN, FB_RUN + 1]) | set(range(e - FB_RUN - 1, e + 1)))


def run_boundary_cases(B):
    layout = comb(B)
    top = top_index(layout)
    out = []
    for i in range(top + 1):
        for e in run_entries(B):
            for sign in (1, -1):
                v = sign * e
                if i == top:
                    if not 0 < v <= (R - 1) >> layout[top][0]:
                        continue
                elif not lo(B) <= v <= hi(B):
                    continue
                d = _zeros(layout)
                d[i] = v
                if v < 0:
                    d[i + 1] = 1
                out.append(("w%d:entry%+d" % (i, v), d))
    return out


def cases(layout, comb_bits=None):
    """[(name, digits, h)] of every family for the layout, each scalar once; comb_bits adds the run boundaries of that comb."""
    c = one_window_cases(layout) + top_cases(layout) + all_window_cases(layout)
    if comb_bits is not None:
        c += run_boundary_cases(comb_bits)
    out, seen = [], set()
    for name, d in c:
        h = from_digits(layout, d)
        if h not in seen:
            seen.add(h)
            out.append((name, d, h))
    return out


def comb_cases(B):
    return cases(comb(B), B)


def msm_cases(c):
    return cases(msm(c))


def w4_cases():
    return cases(w4())


def claimed_pairs(layout):
    """What the union of a layout's cases must reach: (window, lo) and (window, hi) of every window below the top, and
    the top window's largest digit."""
    top = top_index(layout)
    return ({(i, lo(layout[i][1])) for i in range(top)} | {(i, hi(layout[i][1])) for i in range(top)}
            | {(top, top_max(layout))})


def pairs_met(layout, hs):
    """The (window, digit) pairs that the scalars hs reach, by the recoding."""
    met = set()
    for h in hs:
        met.update(enumerate(recode(layout, h)))
    return met


def assert_covers(layout, hs, pairs=None):
    """The share of claimed pairs left out is zero."""
    want = claimed_pairs(layout) if pairs is None else set(pairs)
    missing = want - pairs_met(layout, hs)
    assert not missing, sorted(missing)[:8]
