"""Inputs shared by tests/test_vb_lean_host.py and tests/test_vb_lean_gpu.py: the scalars and encodings at which the lean
variable-base chain (curve.hpp ge_scalar_mul_w4_lean) could go wrong."""
import numpy as np

Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383


def le(v):
    return np.frombuffer(int(v % (1 << 256)).to_bytes(32, "little"), np.uint8)


def _top_digit_halves():
    """h_t, t = 0..5: values below r whose signed window digit 62 is t (t = 5: nibble 62 is 4 and the digit below, 8, carries)"""
    h = [t * 16 ** 62 for t in range(5)] + [4 * 16 ** 62 + 8 * 16 ** 61]
    assert all(0 <= v < R_ORDER for v in h)
    return h


def special_scalars():
    eights = [8 * 16 ** i for i in (0, 1, 7, 31, 61)]
    halves = _top_digit_halves()
    # a kernel that halves the scalar first sees h_t for k = 2 h_t mod r; the Element kernel for k = h_t
    return [0, 1, 2, R_ORDER - 1, R_ORDER - 2, (1 << 256) - 1] + eights + [2 * e % R_ORDER for e in eights] + \
        [2 * v % R_ORDER for v in halves] + halves


def special_points(oracle, valid):
    """identity, not a field element (non-canonical), a negative s, and a canonical non-negative s that is on no curve point
    (about half of them are not: the first such neighbour of a valid encoding) -- from valid encodings"""
    enc = valid[:4].copy()
    enc[0] = 0
    enc[1] = 0xFF
    enc[2] = le((Q - int.from_bytes(bytes(valid[2]), "little")) % Q)
    s = int.from_bytes(bytes(valid[3]), "little")
    cand = np.stack([le(s ^ (2 << b)) for b in range(64)])        # bit 0 stays: s remains non-negative; far below q's top bits
    _, st = oracle.decompress(cand)
    assert st.any()
    enc[3] = cand[int(np.argmax(st != 0))]
    assert int.from_bytes(bytes(enc[3]), "little") < Q and enc[3, 0] % 2 == 0
    return enc
