"""What tests/test_msm_short_host.py and tests/test_msm_short_gpu.py share: msm_plan.hpp's window shape for a bit count restated
in Python (the host test holds it against the C++), the edge scalars built from it, and records <-> integers."""
import numpy as np

BITS = {8: 65, 16: 129}                                          # 8 * scalar_bytes + 1: room for the carry into the top window


def py_shape(B, c):
    """win_shape_bits(B, c) -> (c', W, nwide, first_bit[W], width[W])"""
    W = -(-B // c)
    cw = -(-B // W)
    nwide = W - (W * cw - B)
    width = [cw] * nwide + [cw - 1] * (W - nwide)
    first = [sum(width[:w]) for w in range(W)]
    return cw, W, nwide, first, width


def pick_window(n):
    """msm.hip's width rule by n, which the short forms keep"""
    return 16 if n >= 3 << 20 else (14 if n >= 1 << 19 else 12)


def edge_scalars(nbytes, c):
    """0, 1, 2^bits - 1 (a carry through every window into the top one, which it leaves at +2^(width-1)), 2^(bits-1), and every
    k that puts exactly -2^(width-1) in one window (below the top a digit lies in [-2^(width-1), 2^(width-1) - 1]): alone, with
    every bit below set, one less, and with every other bit set."""
    bits = 8 * nbytes
    _, W, _, first, width = py_shape(BITS[nbytes], c)
    ks = [0, 1, (1 << bits) - 1, 1 << (bits - 1)]
    for w in range(W):
        half = 1 << (first[w] + width[w] - 1)
        if half < 1 << bits:
            ks += [half, half - 1, half | (half - 1), ((1 << bits) - 1) ^ half]
    return ks


def records(ks, nbytes):
    """[n, nbytes] uint8: the integers as packed little-endian records"""
    return np.frombuffer(b"".join(int(k).to_bytes(nbytes, "little") for k in ks), np.uint8).reshape(len(ks), nbytes).copy()


def extended(rec):
    """[n, 32] uint8: the records zero-extended to d377_msm's scalars"""
    out = np.zeros((rec.shape[0], 32), np.uint8)
    out[:, :rec.shape[1]] = rec
    return out
