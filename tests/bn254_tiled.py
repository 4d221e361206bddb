"""Test helper (not collected): expected values for MSMs and Groth16 proofs over *tiled* points, at sizes where per-point curve
arithmetic in Python would be too slow.  Built on tests/bn254_ref.py and numpy alone; shares no code with the library.

* `tables()`: 1024 G1 and 256 G2 points with known discrete logs (the same seeded values the Groth16 GPU tests always used);
* `tiled_total`: sum_i s_i k_(i mod T) for any n, from per-table-entry limb sums, so an n-point MSM's expected value costs T
  big-integer products and one scalar multiplication;
* `window_shape`: the (c, W, G, seg) the library's Pippenger derives from n, restated from its documentation;
* seeded scalar patterns (uniform below r, sparse, single-digit, all 2^253 - 1, circom-like skew), every scalar canonical;
* `TiledKey`: a Groth16 key whose A / B1 / B2 / C / H / IC points are drawn by index from the tables and whose discrete logs are
  tiled to match.  It is no trusted setup (its proofs do not verify), but `bn254_ref.prove(key, ..., definitional=False)` is still
  the exact proof a prover must return for it, and building it costs no curve arithmetic per point.
"""
import functools
import random

import numpy as np

import bn254_ref as ref

R = ref.R
T1, T2 = 1024, 256


@functools.lru_cache(maxsize=None)
def tables():
    """(k1, p1, k2, p2): p1[i] = k1[i] G1 (1024 entries), p2[i] = k2[i] G2 (256 entries), k2 = k1[:256]"""
    rng = random.Random(99)
    k1 = [rng.randrange(1, R) for _ in range(T1)]
    k2 = k1[:T2]
    return k1, ref.fixed_base(1).many(k1), k2, ref.fixed_base(2).many(k2)


def ilog2(n):
    return n.bit_length() - 1


def window_shape(n):
    """(c, W, G, seg) of an n-point MSM: window width, windows, workgroups per window and buckets per lane of the weighted reduction"""
    c = min(16, max(4, ilog2(n) - 4))
    G = max(1, (1 << c) // 2048)
    return c, -(-256 // c), G, -(-(1 << c) // (256 * G))


def scalar_ints(sc):
    """rows of 8 little-endian u32 words -> Python ints"""
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(sc, dtype="<u4")]


def tiled_total(ks, sc, dead=()):
    """sum_i sc[i] * ks[i mod len(ks)] mod r for sc of shape (n, 8) u32 words, any n; rows listed in `dead` (points at infinity)
    add nothing.  Per table entry the limbs are summed in uint64 (at most ceil(n / T) values below 2^32 each: n / T < 2^32)."""
    t, n = len(ks), len(sc)
    sc = np.asarray(sc, dtype=np.uint32)
    if len(dead):
        sc = sc.copy()
        sc[list(dead)] = 0
    full = n // t
    limb = sc[:full * t].reshape(full, t, 8).astype(np.uint64).sum(axis=0)
    limb[:n - full * t] += sc[full * t:]
    total = 0
    for j in range(t):
        total += sum(int(limb[j, l]) << (32 * l) for l in range(8)) * ks[j]
    return total % R


def tile_words(words, per_point, n):
    """the device layout of n points drawn cyclically from a table's words (per_point words each)"""
    tab = np.asarray(words, dtype=np.uint32).reshape(-1, per_point)
    reps = -(-n // len(tab))
    return np.tile(tab, (reps, 1))[:n].ravel()


# ---- scalar patterns: (n, 8) u32 words, every scalar below r ----
_R_WORDS = np.frombuffer(R.to_bytes(32, "little"), dtype="<u4").astype(np.uint32)


def below_r(w):
    """per row: the 256-bit value is below r"""
    lt = np.zeros(len(w), bool)
    eq = np.ones(len(w), bool)
    for l in range(7, -1, -1):
        lt |= eq & (w[:, l] < _R_WORDS[l])
        eq &= w[:, l] == _R_WORDS[l]
    return lt


def uniform(rng, n):
    """uniform below r by rejection from 254 bits; the first rows are r - 1, 0 and 1"""
    w = np.zeros((n, 8), np.uint32)
    todo = np.arange(n)
    while len(todo):
        x = rng.integers(0, 1 << 32, size=(len(todo), 8), dtype=np.uint64).astype(np.uint32)
        x[:, 7] &= 0x3FFFFFFF
        w[todo] = x
        todo = todo[~below_r(x)]
    for i, v in enumerate((R - 1, 0, 1)[:n]):
        w[i] = np.frombuffer(v.to_bytes(32, "little"), dtype="<u4")
    return w


def digit_set(c, seg):
    """the first and last bucket of a lane's segment and of the window"""
    top = 1 << c
    return sorted({d for d in (1, 2, seg - 1, seg, seg + 1, top - seg, top - 2, top - 1) if 1 <= d < top})


def top_window(c):
    """the last window a canonical scalar can have a non-zero digit in (r has 254 bits; a window above bit 253 stays zero)"""
    return 253 // c


def top_digit_max(c):
    """the largest digit of the top window that keeps d * 2^(c w) below r"""
    return (R - 1) >> (c * top_window(c))


def place_digits(ws, ds, c):
    """the scalars d * 2^(c w) as words"""
    ws, ds = np.asarray(ws, np.int64), np.asarray(ds, np.uint64)
    out = np.zeros((len(ws), 8), np.uint32)
    bit = ws * c
    word, sh = bit >> 5, (bit & 31).astype(np.uint64)
    v = ds << sh  # below 2^(16 + 31)
    rows = np.arange(len(ws))
    out[rows, word] = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = word < 7
    out[rows[hi], word[hi] + 1] = (v[hi] >> np.uint64(32)).astype(np.uint32)
    assert not (v[~hi] >> np.uint64(32)).any()
    return out


def single_digit(rng, n, c, seg):
    """d * 2^(c w): w over every window up to the top one, d from digit_set (in the top window only the digits that keep the
    scalar below r, and the largest such digit)"""
    W = top_window(c) + 1
    ds_all = np.array(digit_set(c, seg), np.uint64)
    dmax = top_digit_max(c)
    ds_top = np.array(sorted({int(d) for d in ds_all if d <= dmax} | {dmax}), np.uint64)
    ws = rng.integers(0, W, size=n)
    ds = ds_all[rng.integers(0, len(ds_all), size=n)]
    top = ws == W - 1
    ds[top] = ds_top[rng.integers(0, len(ds_top), size=int(top.sum()))]
    return place_digits(ws, ds, c)


def sparse(rng, n, c, seg):
    """about one scalar in 64 non-zero: uniform ones below c = 9, single-digit ones from there (most buckets of every window
    stay empty)"""
    w = single_digit(rng, n, c, seg) if c >= 9 else uniform(rng, n)
    w[rng.random(n) >= 1 / 64] = 0
    return w


def all_ones_253(n):
    """every scalar 2^253 - 1: every digit below the top window is 2^c - 1, so each window has one bucket, holding n entries"""
    w = np.full((n, 8), 0xFFFFFFFF, np.uint32)
    w[:, 7] = 0x1FFFFFFF
    return w


def skewed(rng, n):
    """circom-like: 45 % ones, 45 % zeros, the rest uniform below 2^253"""
    w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 7] &= 0x1FFFFFFF
    m = rng.random(n)
    w[m < 0.9] = 0
    w[m < 0.45, 0] = 1
    return w


PATTERNS = ("uniform", "sparse", "single_digit", "all_ones_253", "skewed")


def pattern(name, seed, n):
    """the scalars of one named pattern for an n-point MSM (the width and segment are those n implies)"""
    c, _, _, seg = window_shape(n)
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return uniform(rng, n)
    if name == "sparse":
        return sparse(rng, n, c, seg)
    if name == "single_digit":
        return single_digit(rng, n, c, seg)
    if name == "all_ones_253":
        return all_ones_253(n)
    if name == "skewed":
        return skewed(rng, n)
    raise KeyError(name)


def sweep_sizes():
    """the n of the width sweep: per c in 4 .. 16 one n in [2^(c+4), 2^(c+5)) that is no power of two (just above the threshold,
    where the width changes), n = 200 at c = 4 and exactly 2^20 at c = 16"""
    ns = [200]
    for c in range(4, 17):
        ns.append((1 << (c + 4)) + (3 << max(0, c - 6)) + 3 if c < 16 else (1 << 20) + 3)
    ns.append(1 << 20)
    return sorted(ns)


CHUNK_LENGTHS = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)


def chunk_boundary_case(seed):
    """(scalars, dead rows): single-digit scalars that give ten distinct buckets of one MSM exactly CHUNK_LENGTHS entries, one zero
    scalar, and one row whose point is to be the point at infinity (it carries the scalar of the 16-entry bucket, so counting it
    would make that list 17 long); rows shuffled.  13 107 rows: c = 9."""
    n = sum(CHUNK_LENGTHS) + 2
    c, _, _, seg = window_shape(n)
    assert c == 9
    rng = np.random.default_rng(seed)
    W, dmax = top_window(c) + 1, top_digit_max(c)
    # distinct (window, digit) pairs: the bottom and the top window, segment and window edges
    buckets = [(0, 1), (W - 1, dmax), (0, (1 << c) - 1), (W - 1, 1), (5, seg), (5, seg + 1), (11, (1 << c) - seg), (17, (1 << c) - 2),
               (W - 2, (1 << c) - 1), (3, seg - 1)]
    assert len(set(buckets)) == len(CHUNK_LENGTHS)
    ws, ds = [], []
    for (w, d), length in zip(buckets, CHUNK_LENGTHS):
        ws += [w] * length
        ds += [d] * length
    w16, d16 = buckets[CHUNK_LENGTHS.index(16)]
    sc = np.concatenate([place_digits(ws, ds, c), place_digits([w16], [d16], c), np.zeros((1, 8), np.uint32)])
    perm = rng.permutation(n)
    sc = sc[perm]
    dead = int(np.nonzero(perm == n - 2)[0][0])
    return sc, [dead], buckets


# ---- tiled keys ----
def r1cs_coefs(r1cs):
    """the zkey's coefficient list (matrix, constraint, signal, value) of an R1CS: its A and B rows, then snarkjs's one extra A row
    per public signal and the constant one"""
    coefs = []
    for ci, (a, b, _c) in enumerate(r1cs.constraints):
        coefs += [(0, ci, s, k) for s, k in a.items()]
        coefs += [(1, ci, s, k) for s, k in b.items()]
    m = len(r1cs.constraints)
    coefs += [(0, m + s, s, 1) for s in range(r1cs.n_public + 1)]
    return coefs


class TiledKey:
    """The fields `bn254_ref.write_zkey` and `bn254_ref.prove` read, over tiled points.  Point j of a list is table entry
    (stride * j + start) mod T; B1 and B2 share their logs, so they index the first 256 entries; alpha, beta, gamma, delta are
    table logs too."""

    def __init__(self, r1cs):
        k1, p1, k2, p2 = tables()
        self.r1cs = r1cs
        self.N = r1cs.domain()
        self.coefs = r1cs_coefs(r1cs)
        n, npub = r1cs.n_vars, r1cs.n_public
        g1 = lambda count, stride, start: [(stride * j + start) % T1 for j in range(count)]
        ia, ib = g1(n, 1, 11), [(3 * j + 5) % T2 for j in range(n)]
        ic, ih, iic = g1(n - npub - 1, 7, 1), g1(self.N, 5, 2), g1(npub + 1, 1, 900)
        self.u, self.A = [k1[i] for i in ia], [p1[i] for i in ia]
        self.v, self.B1, self.B2 = [k2[i] for i in ib], [p1[i] for i in ib], [p2[i] for i in ib]
        self.c_k, self.C = [k1[i] for i in ic], [p1[i] for i in ic]
        self.h_k, self.H = [k1[i] for i in ih], [p1[i] for i in ih]
        self.ic_k, self.IC = [k1[i] for i in iic], [p1[i] for i in iic]
        self.tau = 0  # takes no part: the logs above are not derived from a trapdoor
        self.alpha, self.beta, self.gamma, self.delta = k1[0], k1[1], k1[3], k1[2]
        self.alpha1, self.beta1, self.delta1 = p1[0], p1[1], p1[2]
        self.beta2, self.gamma2, self.delta2 = p2[1], p2[3], p2[2]

    def zkey(self):
        return ref.write_zkey(self)


def tiled_key(n_vars, n_public, n_cons, kind, seed, empty_a_from=None, empty_b_from=None):
    """(TiledKey, witness) over a seeded random R1CS; constraints from index empty_a_from (empty_b_from) on have no A (B)
    entries, so their CSR rows are empty ranges.  The prover needs no satisfied witness: C on the domain is A times B."""
    rng = random.Random(seed)
    w = ref.random_witness(rng, n_vars, kind)
    r1 = ref.random_r1cs(rng, w, n_public, n_cons)
    for ci, (a, b, c) in enumerate(r1.constraints):
        if empty_a_from is not None and ci >= empty_a_from:
            a.clear()
        if empty_b_from is not None and ci >= empty_b_from:
            b.clear()
    return TiledKey(r1), w


# n_vars, n_public, n_cons, witness kind, constraints from this index on without A entries / without B entries.
# The A, B1 and B2 MSMs have n_vars + 2 points and the C MSM n_vars - n_public - 1 + N + 3, so with (c of A / B, c of C):
PROOF_SHAPES = [
    (5, 0, 0, "random", None, None),          # N = 1: no NTT stage at all; (4, 4)
    (5, 0, 1, "edge", None, None),            # N = 2: LDS workgroups of 1 lane
    (6, 1, 2, "small", None, None),           # N = 4: 2 lanes
    (7, 1, 5, "repeat", None, 2),             # N = 8: 4 lanes
    (300, 0, 1500, "random", 700, None),      # N = 2^11: one global stage; (4, 7)
    (5000, 1, 6000, "small", None, 3000),     # N = 2^13: three; (8, 9)
    (20000, 1, 12000, "repeat", 9000, None),  # N = 2^14: four; (10, 11)
    (3000, 0, 9000, "edge", None, None),      # N = 2^14; (7, 10)
]


def proof_domain(case):
    """the domain size N of a PROOF_SHAPES case: the power of two that holds its constraints and public rows"""
    N = 1
    while N < case[2] + case[1] + 1:
        N *= 2
    return N
