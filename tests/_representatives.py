"""Every representative of a group element as an Element record, for tests/test_representatives_host.py and
tests/test_representatives_gpu.py.

An Element record (X, Y, Z, T: fully reduced Montgomery limbs) is one of many representatives of its group element: any
non-zero scaling (lX, lY, lZ, lT) is the same element, and so is the 2-torsion twin (-X, -Y, Z, T) = P + (0, -1), which the
encoding and eq quotient away.  build() makes, from a seed and a count, the plain records A (Z = 1) and the same group elements
in every kind of KINDS, the identity class in every form of IDENTITY_FORMS, and scalars whose halves k / 2 mod r take both
parities; mixed(), plant() and layouts() arrange them into the arrays the tests hand to the code under test, always together with
the plain records of the same group elements, on which the oracle gives the expected value.

Run as a program (python _representatives.py LIBRARY IN.npz OUT.npz) it is the child process that walks the host simulation's
Element-taking entry points in a library built with -DD377_BOUNDS, where a violated precondition aborts."""
import ctypes
import sys

import numpy as np

Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R = 2111115437357092606062206234695386632838870926408408195193685246394721360383
D = 3021                                                         # -x^2 + y^2 = 1 + D x^2 y^2

KINDS = ("affine", "proj", "scaled", "minus", "twin", "twin_scaled", "twin_minus")
SCALED_KINDS = ("scaled", "minus")                               # l A: to_affine gives the limbs of to_affine(A); the Elligator
                                                                 # record may be l twin(A), whichever the encoding decodes to
TWIN_KINDS = ("twin", "twin_scaled", "twin_minus")
IDENTITY_FORMS = ("canonical", "scaled", "torsion", "torsion_scaled", "p_minus_p", "p_plus_twin_minus_p")
FIXED_SCALARS = (0, 1, 2, R - 1, R, R + 1, (1 << 256) - 1)
PLANTS = (0, 63, 64)                                             # ... and n - 1: where plant() puts identity-class records


def scalar_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def half_is_odd(k):
    """[n] bool: is h = k / 2 mod r odd, for the scalars k [n, 32] (any bytes: reduced mod r first)?  The chains walk h and
    double at the end; h = k / 2 for an even k mod r and (k + r) / 2 for an odd one."""
    inv2 = (R + 1) // 2
    return np.array([(int.from_bytes(bytes(row), "little") % R * inv2 % R) & 1 for row in k], bool)


def neg_fq(oracle, a):
    return oracle.fq_op(4, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4))[0]


def scale(oracle, recs, lam):
    """(l X, l Y, l Z, l T) of every record, l = lam[i] ([n, 4] Montgomery limbs)."""
    recs = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 16)
    return oracle.fq_op(2, recs.reshape(-1, 4), np.repeat(lam, 4, axis=0))[0].reshape(-1, 16)


def twin(oracle, recs):
    """(-X, -Y, Z, T) = P + (0, -1) of every record."""
    out = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 16).copy()
    out[:, :8] = neg_fq(oracle, out[:, :8]).reshape(-1, 8)
    return out


def minus(oracle, recs):
    """The record scaled by -1: (-X, -Y, -Z, -T)."""
    return neg_fq(oracle, recs).reshape(-1, 16)


def random_lambda(oracle, rng, n):
    """n random non-zero field elements as [n, 4] Montgomery limbs."""
    lam = oracle.fq_from_bytes_mod_order(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    assert lam.any(axis=1).all()
    return lam


class Reps:
    """What build() returns.  A: [count, 16] the plain records (Z = 1); kinds: kind -> [count, 16], record i a representative
    of A[i] (kinds["affine"] is A); ident: [6 * ident_rounds, 16] the identity class, record j in form
    IDENTITY_FORMS[j % 6]; scalars: [count, 32], FIXED_SCALARS first."""

    def __init__(self, A, kinds, ident, scalars):
        self.A, self.kinds, self.ident, self.scalars = A, kinds, ident, scalars
        self.count = A.shape[0]


def make_scalars(rng, count):
    """FIXED_SCALARS (as many as count holds), then random 32-byte strings.  Of the random ones at least a quarter have an
    odd h = k / 2 mod r and at least a quarter an even one (asserted when there are 8 or more)."""
    k = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    for i, v in enumerate(FIXED_SCALARS[:count]):
        k[i] = scalar_bytes(v)
    rand = k[len(FIXED_SCALARS):]
    if rand.shape[0] >= 8:
        odd = int(half_is_odd(rand).sum())
        assert 4 * odd >= rand.shape[0] and 4 * (rand.shape[0] - odd) >= rand.shape[0], (odd, rand.shape[0])
    return k


def build(oracle, seed, count, ident_rounds=4):
    """-> Reps.  Point 0 is the generator; the others are Elligator outputs.  A = decompress(compress(.)): Z = 1."""
    rng = np.random.default_rng(seed)
    proj = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (count, 32), dtype=np.uint8)), dtype=np.uint64)
    proj[0] = scale(oracle, oracle.generator_xyzt(), random_lambda(oracle, rng, 1))[0]    # the generator with Z != 1
    A, st = oracle.decompress(oracle.compress(proj))
    assert not st.any()
    A = np.ascontiguousarray(A, dtype=np.uint64)
    one = oracle.identity_xyzt()[4:8]                           # Y of (0, 1, 1, 0): the limbs of 1
    assert (A[:, 8:12] == one).all() and not (proj[:, 8:12] == one).all(axis=1).any()
    tw = twin(oracle, A)
    tm = A.copy()                                                # (X, Y, -Z, -T) = -1 * twin
    tm[:, 8:] = neg_fq(oracle, A[:, 8:]).reshape(-1, 8)
    kinds = {"affine": A, "proj": proj, "scaled": scale(oracle, A, random_lambda(oracle, rng, count)), "minus": minus(oracle, A),
             "twin": tw, "twin_scaled": scale(oracle, tw, random_lambda(oracle, rng, count)), "twin_minus": tm}
    canon = oracle.identity_xyzt()
    ident = []
    for r in range(ident_rounds):
        p = proj[(r + 1) % count:(r + 1) % count + 1]
        np_ = oracle.neg_xyzt(p)
        lam = random_lambda(oracle, rng, 2)
        ident += [canon, scale(oracle, canon, lam[:1])[0], twin(oracle, canon)[0], scale(oracle, twin(oracle, canon), lam[1:])[0],
                  oracle.add_xyzt(p, np_)[0], oracle.add_xyzt(p, twin(oracle, np_))[0]]
    return Reps(A, kinds, np.ascontiguousarray(np.stack(ident), dtype=np.uint64), make_scalars(rng, count))


def mixed(reps, n, shift=0, first=0, kinds=KINDS):
    """n records that mix `kinds` cyclically: record i is kind kinds[(i + shift) % len(kinds)] of point first + i (mod count), so
    every wave holds every kind -> (records, the plain records of the same points, the kind of every record)."""
    idx = (first + np.arange(n)) % reps.count
    names = [kinds[(i + shift) % len(kinds)] for i in range(n)]
    recs = np.stack([reps.kinds[k][j] for k, j in zip(names, idx)]) if n else np.zeros((0, 16), np.uint64)
    return np.ascontiguousarray(recs, dtype=np.uint64), np.ascontiguousarray(reps.A[idx]), names


def plant(reps, recs, plain, names=None):
    """Identity-class records at positions 0, 63, 64 and n - 1 (those that exist), each position another form; the plain
    records there become the canonical identity -> (records, plain, names), copies."""
    recs, plain = recs.copy(), plain.copy()
    names = list(names) if names is not None else [None] * len(recs)
    n = recs.shape[0]
    for j, pos in enumerate(sorted({p for p in PLANTS + (n - 1,) if 0 <= p < n})):
        f = (2 * j + 1 + n) % reps.ident.shape[0]                # 2 j + 1: the scaled, torsion-scaled and P + twin(-P) forms come first
        recs[pos], plain[pos] = reps.ident[f], reps.ident[0]
        names[pos] = "identity:" + IDENTITY_FORMS[f % len(IDENTITY_FORMS)]
    return recs, plain, names


def all_identity_but_one(reps, n):
    """Every record of the identity class (the forms in turn) except one ordinary record, a scaled twin, in the middle."""
    recs = reps.ident[np.arange(n) % reps.ident.shape[0]].copy()
    plain = np.tile(reps.ident[0], (n, 1))
    recs[n // 2], plain[n // 2] = reps.kinds["twin_scaled"][n // 2 % reps.count], reps.A[n // 2 % reps.count]
    return np.ascontiguousarray(recs), np.ascontiguousarray(plain)


def one_identity(reps, n, where=None):
    """Every record ordinary (all kinds mixed) except one of the identity class, (0, -l, l, 0), inside the second wave."""
    recs, plain, _ = mixed(reps, n, shift=3)
    where = min(n - 1, 70) if where is None else where
    recs[where], plain[where] = reps.ident[3], reps.ident[0]
    return recs, plain


def layouts(reps, n, shift=0):
    """name -> (records, plain records): all kinds mixed with the plants of plant(); at n = 257 also the two extreme layouts."""
    recs, plain, _ = mixed(reps, n, shift=shift)
    out = {"mixed_planted": plant(reps, recs, plain)[:2]}
    if n == 257:
        out["all_identity_but_one"] = all_identity_but_one(reps, n)
        out["one_identity"] = one_identity(reps, n)
    return out


def right_operands(oracle, reps, n, shift=0):
    """The right operands that go with mixed(reps, n, shift) as left operands: record i is of the NEXT kind, and of point i + 1
    (groups 0, 3, 6 .. of seven records), of point i itself (groups 1, 4 ..: P + P', P - P'), or of -P_i (groups 2, 5 ..:
    P + (-P)', which is of the identity class) -- so that with the twin kinds on the right P + twin(P), P - twin(P) (the point of
    order 2 as a difference) and P + twin(-P) all occur -> (records, the plain records of the same group elements)."""
    recs, plain = np.zeros((n, 16), np.uint64), np.zeros((n, 16), np.uint64)
    for i in range(n):
        kind = KINDS[(i + shift + 1) % len(KINDS)]
        variant = (i // len(KINDS)) % 3
        j = ((i + 1) if variant == 0 else i) % reps.count
        recs[i], plain[i] = reps.kinds[kind][j], reps.A[j]
    neg = (np.arange(n) // len(KINDS)) % 3 == 2
    if neg.any():
        recs[neg], plain[neg] = oracle.neg_xyzt(recs[neg]), oracle.neg_xyzt(plain[neg])
    return recs, plain


def cancelling_scalars(reps, which=0):
    """(k, r - k) as two 32-byte rows, k a random scalar of the builder's reduced mod r (not 0)."""
    kv = int.from_bytes(bytes(reps.scalars[len(FIXED_SCALARS) + which % (reps.count - len(FIXED_SCALARS))]), "little") % R
    assert kv
    return scalar_bytes(kv), scalar_bytes(R - kv)


def plant_cancelling_pair(reps, P, PA, k, lo, length, which=0):
    """Terms lo and lo + 1 become one point as a plain-side kind with k and as a twin kind with r - k, every other scalar of the
    sum lo .. lo + length - 1 becomes 0: the half-sums meet as a point and its twin, and the sum is of the identity class."""
    j = (7 * which + 1) % reps.count
    P[lo], P[lo + 1] = reps.kinds[KINDS[which % 4]][j], reps.kinds[TWIN_KINDS[which % 3]][j]
    PA[lo] = PA[lo + 1] = reps.A[j]
    k[lo], k[lo + 1] = cancelling_scalars(reps, which)
    k[lo + 2:lo + length] = 0


def plant_identity_sum(reps, P, PA, k, lo, length):
    """Every term of the sum lo .. lo + length - 1 becomes an identity-class record (the forms in turn) with a random scalar."""
    t = np.arange(length)
    P[lo:lo + length] = reps.ident[(t + 1) % reps.ident.shape[0]]
    PA[lo:lo + length] = reps.ident[0]
    k[lo:lo + length] = reps.scalars[len(FIXED_SCALARS) + t % (reps.count - len(FIXED_SCALARS))]


def sums_case(reps, lengths, shift=0):
    """The terms of len(lengths) sums, sum i of lengths[i] terms: all kinds mixed with the plants of plant() over the whole term
    array, the builder's scalars -- and, from three sums on, a cancelling pair (plant_cancelling_pair) in the first sum after sum 0
    that has two terms and an all-identity sum (plant_identity_sum) in the next non-empty one -> (records, plain records, scalars,
    offsets [n + 1] u64, {"cancel": sum or None, "identity": sum or None})."""
    lengths = [int(v) for v in lengths]
    n, total = len(lengths), sum(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    P, PA, names = mixed(reps, total, shift=shift)
    if total:
        P, PA, _ = plant(reps, P, PA, names)
    k = np.roll(reps.scalars, 5, axis=0)[np.arange(total) % reps.count].copy()
    info = {"cancel": None, "identity": None}
    if n >= 3:
        c = next((i for i in range(1, n) if lengths[i] >= 2), None)
        d = next((i for i in range((c or 1) + 1, n) if lengths[i] >= 1), None)
        if c is not None:
            plant_cancelling_pair(reps, P, PA, k, int(off[c]), lengths[c], which=c)
        if d is not None:
            plant_identity_sum(reps, P, PA, k, int(off[d]), lengths[d])
        info = {"cancel": c, "identity": d}
    return P, PA, k, off, info


def special_sums(reps, m):
    """Two sums of m terms on their own: a cancelling pair whose other scalars are 0 (m >= 2; for m = 1 a second all-identity
    sum) and a sum whose every term is of the identity class -> (records, plain records, scalars).  Both give the all-zero
    Encoding."""
    P, PA, _ = mixed(reps, 2 * m, shift=2)
    k = reps.scalars[np.arange(2 * m) % reps.count].copy()
    if m >= 2:
        plant_cancelling_pair(reps, P, PA, k, 0, m, which=m)
    else:
        plant_identity_sum(reps, P, PA, k, 0, m)
    plant_identity_sum(reps, P, PA, k, m, m)
    return P, PA, k


def to_ints(oracle, recs):
    """[n, 16] records -> n tuples (X, Y, Z, T) of python ints (out of Montgomery form)."""
    b = oracle.fq_to_bytes(np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 4))
    v = [int.from_bytes(bytes(r), "little") for r in b]
    return [tuple(v[4 * i:4 * i + 4]) for i in range(len(v) // 4)]


def assert_valid(oracle, recs, what=""):
    """Every record is an Element as the crate checks one (src/min_curve/element.rs:84-110), in integers: the limbs as stored
    are below q, Z != 0, T Z = X Y and -X^2 + Y^2 = Z^2 + D T^2."""
    recs = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 16)
    for i, row in enumerate(recs):
        for c in range(4):
            assert sum(int(l) << (64 * j) for j, l in enumerate(row[4 * c:4 * c + 4])) < Q, (what, i, c)
    for i, (X, Y, Z, T) in enumerate(to_ints(oracle, recs)):
        assert Z % Q != 0, (what, i)
        assert (X * Y - Z * T) % Q == 0, (what, i)
        assert (-X * X + Y * Y - Z * Z - D * T * T) % Q == 0, (what, i)


# ---- the host simulation's Element-taking entry points (tests/host_sim/sim.cpp) ----------------------------------------------------
SIM_MSM_M = (1, 3, 8)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_sim(L, P, Q2, k):
    """Every Element-taking entry point of the simulation on the records P (and Q2 as right operands, k as scalars) -> dict of
    results.  L: the loaded library, sim_init() already called."""
    P, Q2, k = (np.ascontiguousarray(a) for a in (P, Q2, k))
    n = P.shape[0]
    n_ = ctypes.c_size_t
    z = lambda *shape: np.zeros(shape, np.uint64)
    out = {"compress": np.zeros((n, 32), np.uint8), "compress_assisted": np.zeros((n, 32), np.uint8), "to_affine": z(n, 8)}
    L.sim_compress(_p(P), n_(n), _p(out["compress"]))
    L.sim_compress_assisted(_p(P), n_(n), _p(out["compress_assisted"]))
    L.sim_to_affine_raw(_p(P), n_(n), _p(out["to_affine"]))
    out.update(raw_add=z(n, 16), raw_double=z(n, 16), raw_neg=z(n, 16), raw_eq=np.zeros(n, np.uint8), raw_neg_ok=np.zeros(n, np.uint8),
               raw_f_ok=np.zeros(n, np.uint8))
    f = [z(n, 4) for _ in range(5)]
    L.sim_raw_forms(_p(P), _p(Q2), n_(n), _p(out["raw_add"]), _p(out["raw_double"]), _p(out["raw_neg"]), _p(out["raw_eq"]),
                    _p(out["raw_neg_ok"]), _p(f[0]), _p(f[1]), _p(f[2]), _p(f[3]), _p(f[4]), _p(out["raw_f_ok"]))
    out.update(misc_add=z(n, 16), misc_neg=z(n, 16))
    L.sim_group_misc(_p(P), _p(Q2), n_(n), _p(out["misc_add"]), _p(out["misc_neg"]))
    for m in SIM_MSM_M:
        sums = n // m
        out["msm%d" % m] = np.zeros((sums, 32), np.uint8)
        L.sim_batch_msm(_p(P), _p(k), ctypes.c_int(m), n_(sums), _p(out["msm%d" % m]))
    return out


def main(argv):
    L = ctypes.CDLL(argv[1])
    L.sim_init.restype = ctypes.c_int
    assert L.sim_init() == 0
    inp = np.load(argv[2])
    res = {}
    for name in sorted({key.split(".")[0] for key in inp.files}):
        got = run_sim(L, inp[name + ".P"], inp[name + ".Q"], inp[name + ".k"])
        res.update({name + "." + key: v for key, v in got.items()})
    np.savez(argv[3], **res)
    print("REPRESENTATIVES_SIM_OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
