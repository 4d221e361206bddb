"""Test helper (not collected): edge operands for the BN254 field and curve code (boundless_amd/csrc/bn254_arith.hpp), exact
references in plain Python integers, and the two builds of the one op table (tests/bn254_edge_ops.hpp) that run them: a host
program (bn254_edge_host.cpp, plain and under -fsanitize=address,undefined) and a gfx950 module (bn254_edge_dev.hip).

Operands are the STORED limb patterns, i.e. the Montgomery representation (value = pattern / 2^256 mod m); the references convert
them, the operands are never converted.  Everything is deterministic: the only randomness is random.Random(seed).

Curve references: the XYZZ and affine formulas never use the curve coefficient b, so any pair (x, y) is a point of
y^2 = x^3 + b' with b' = y^2 - x^3, and the affine chord-and-tangent law with a = 0 is an exact, independent reference for edge
coordinates.  Nothing here transcribes the XYZZ formulas; results are compared as affine canonical coordinates.

build() runs where hipcc is (__graft_entry__.build()); the tests only read what it made under tests/_build/bn254_edge/."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RR = 1 << 256  # the Montgomery radix
MAGIC = 0x45444742
_RINV_Q = pow(RR, -1, Q)

# families and ops of tests/bn254_edge_ops.hpp
FIELD_Q, FIELD_R, FQ2, CURVE_Q, CURVE_Q2 = range(5)
F_ADD, F_SUB, F_NEG, F_DBL, F_MUL, F_SQR, F_TO_MONT, F_FROM_MONT, F_INV, F_POW, F_IS_ZERO, F_EQ, F_GE_MOD = range(13)
E_ADD, E_SUB, E_NEG, E_DBL, E_MUL, E_SQR, E_INV, E_TO_MONT, E_FROM_MONT = range(9)
C_ROUNDTRIP, C_AFF_DBL, C_XYZZ_DBL, C_ADD_AFF, C_ADD, C_MUL_SMALL, C_ON_CURVE = range(7)
WORDS_IN = {FIELD_Q: 19, FIELD_R: 19, FQ2: 33, CURVE_Q: 66, CURVE_Q2: 130}
WORDS_OUT = {FIELD_Q: 9, FIELD_R: 9, FQ2: 16, CURVE_Q: 17, CURVE_Q2: 33}
FAMILY_NAMES = {FIELD_Q: "field_q", FIELD_R: "field_r", FQ2: "fq2", CURVE_Q: "curve_q", CURVE_Q2: "curve_q2"}

POW_EXPONENTS = (0, 1, 2, (1 << 32) - 1, 1 << 63, (1 << 64) - 1)
MUL_SMALL_KS = (0, 1, 2, 3, 1 << 31, 0x80000001, (1 << 32) - 1)
FORCED_TARGETS = lambda m: (0, 1, m - 1, m - 2, (1 << 224) - 1)  # noqa: E731
PARTNERS, FORCED_PER_TARGET = 40, 200


# ---------------- operands ----------------
def edge_categories(m):
    """the edge residues of modulus m by rule, in a fixed order (values may repeat across categories)"""
    r = RR % m
    top = m >> 224
    cats = {"small": [0, 1, 2, 3, m - 1, m - 2, m - 3, (m - 1) // 2, (m + 1) // 2],
            "montgomery": [r, m - r, r * r % m, pow(r, -1, m)]}
    powers = []
    for k in range(254):
        for v in (1 << k, (1 << k) + 1, (1 << k) - 1):
            powers += [v % m, (-v) % m]
    cats["powers"] = powers
    cats["below_m"] = [m - (1 << (32 * j)) for j in range(8)]
    masks = []
    for t in (0, top - 1, top):
        for mask in range(128):
            v = t << 224
            for j in range(7):
                if (mask >> j) & 1:
                    v |= 0xFFFFFFFF << (32 * j)
            if v < m:
                masks.append(v)
    cats["limb_masks"] = masks
    return cats


@functools.lru_cache(maxsize=None)
def edge_residues(m):
    """the edge set: the categories above, duplicates dropped, order kept"""
    seen, out = set(), []
    for vals in edge_categories(m).values():
        for v in vals:
            assert 0 <= v < m
            if v not in seen:
                seen.add(v)
                out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def operand_pairs(m):
    """(pairs, kinds): every value with itself, with PARTNERS seeded partners, and the forced products whose Montgomery product
    a b / R lands on each of FORCED_TARGETS"""
    vals = edge_residues(m)
    rng = random.Random(0xB254 ^ (m & 0xFFFF))
    pairs = [(a, a) for a in vals]
    kinds = ["self"] * len(vals)
    for a in vals:
        for b in rng.sample(vals, PARTNERS):
            pairs.append((a, b))
            kinds.append("partner")
    nz = [v for v in vals if v]
    for t in FORCED_TARGETS(m):
        for a in rng.sample(nz, FORCED_PER_TARGET):
            pairs.append((a, t * RR * pow(a, -1, m) % m))
            kinds.append("forced")
    return tuple(pairs), tuple(kinds)


def words(vals):
    """ints below 2^256 -> (n, 8) u32 little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u4").reshape(-1, 8).astype(np.uint32)


def ints(w):
    """(n, 8) u32 limbs -> ints"""
    b = np.ascontiguousarray(w, dtype="<u4").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def below(w, m):
    """per row of (n, 8) limbs: the value is below m"""
    mw = words([m])[0]
    lt, eq = np.zeros(len(w), bool), np.ones(len(w), bool)
    for l in range(7, -1, -1):
        lt |= eq & (w[:, l] < mw[l])
        eq &= w[:, l] == mw[l]
    return lt


# ---------------- field cases ----------------
def ge_mod_extras(m):
    """raw 256-bit values around m for ge_mod: m, m +- 1, 2^256 - 1, and m with each single limb +- 1 (within the limb)"""
    out = [m, m + 1, m - 1, RR - 1]
    for j in range(8):
        limb = (m >> (32 * j)) & 0xFFFFFFFF
        for d in (1, -1):
            out.append(m - (limb << (32 * j)) + (((limb + d) & 0xFFFFFFFF) << (32 * j)))
    return out


@functools.lru_cache(maxsize=None)
def field_cases(m):
    """(records, expected, ops) of the field family of modulus m: binary ops over operand_pairs, unary ops over the edge set"""
    vals = edge_residues(m)
    pairs, _ = operand_pairs(m)
    rinv = pow(RR, -1, m)
    ops, A, B, EXP, res, flag = [], [], [], [], [], []

    def put(op, a, b=0, e=0, r=0, f=0):
        ops.append(op), A.append(a), B.append(b), EXP.append(e), res.append(r), flag.append(f)

    for a, b in pairs:
        put(F_ADD, a, b, r=(a + b) % m)
        put(F_SUB, a, b, r=(a - b) % m)
        put(F_MUL, a, b, r=a * b * rinv % m)
        put(F_EQ, a, b, f=int(a == b))
    for a in vals:
        put(F_NEG, a, r=(-a) % m)
        put(F_DBL, a, r=2 * a % m)
        put(F_SQR, a, r=a * a * rinv % m)
        put(F_TO_MONT, a, r=a * RR % m)
        put(F_FROM_MONT, a, r=a * rinv % m)
        put(F_INV, a, r=pow(a * rinv % m, m - 2, m) * RR % m)  # 0 -> 0
        put(F_IS_ZERO, a, f=int(a == 0))
        put(F_GE_MOD, a, f=0)
        for e in POW_EXPONENTS:
            put(F_POW, a, e=e, r=pow(a * rinv % m, e, m) * RR % m)
    for a in ge_mod_extras(m):
        put(F_GE_MOD, a, f=int(a >= m))
    n = len(ops)
    rec = np.zeros((n, WORDS_IN[FIELD_Q]), np.uint32)
    rec[:, 0] = ops
    rec[:, 1:9], rec[:, 9:17] = words(A), words(B)
    e = np.array(EXP, dtype=np.uint64)
    rec[:, 17], rec[:, 18] = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32)
    exp = np.zeros((n, WORDS_OUT[FIELD_Q]), np.uint32)
    exp[:, :8], exp[:, 8] = words(res), flag
    return rec, exp, np.array(ops)


@functools.lru_cache(maxsize=None)
def raw_mul_cases(m):
    """(records, expected): `mul` on limb patterns OUTSIDE its stated domain, up to 2^256 - 1.  The header promises nothing there,
    but the CIOS product carries two words (t[8], t[9]) that only such operands can make non-zero, and on_curve meets coordinates
    not below q before the loader's range check existed.  The reference is what a Montgomery reduction with one conditional
    subtraction is for any a, b < 2^256: t = (a b + ((a b (-1/m)) mod R) m) / R, then t - m if t >= m (t < R + m, so the answer
    fits 256 bits; it need not be below m)."""
    rng = random.Random(0x7A ^ (m & 0xFF))
    raw = []
    for mask in range(128):
        v = 0xFFFFFFFF << 224
        for j in range(7):
            if (mask >> j) & 1:
                v |= 0xFFFFFFFF << (32 * j)
        raw.append(v)
    raw += [1 << 255, (1 << 255) + 1, (1 << 255) - 1, RR - m, RR - m + 1, RR - m - 1, RR - 2, RR - 3, 5 * m, 5 * m - 1, 4 * m + 1]
    vals = edge_residues(m)
    pairs = [(a, a) for a in raw]
    for a in raw:
        pairs += [(a, b) for b in rng.sample(raw, 8)] + [(a, b) for b in rng.sample(vals, 4)] + [(b, a) for b in rng.sample(vals, 4)]
    ninv = (-pow(m, -1, RR)) % RR
    res = []
    for a, b in pairs:
        ab = a * b
        t, rem = divmod(ab + (ab * ninv % RR) * m, RR)
        assert rem == 0 and t < RR + m
        res.append(t - m if t >= m else t)
    rec = np.zeros((len(pairs), WORDS_IN[FIELD_Q]), np.uint32)
    rec[:, 0] = F_MUL
    rec[:, 1:9], rec[:, 9:17] = words([p[0] for p in pairs]), words([p[1] for p in pairs])
    exp = np.zeros((len(pairs), WORDS_OUT[FIELD_Q]), np.uint32)
    exp[:, :8] = words(res)
    return rec, exp


# ---------------- Fq2 ----------------
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2inv(a):
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    d = pow(n, -1, Q) if n else 0
    return (a[0] * d % Q, (-a[1]) * d % Q)


@functools.lru_cache(maxsize=None)
def fq2_elements():
    """Fq2 operands (c0, c1) from the edge set: c1 = 0, c0 = 0, c0 = c1 and c0 = -c1 (one factor of sqr vanishes in the last two),
    and seeded pairs"""
    vals = edge_residues(Q)
    rng = random.Random(0xF92)
    base = list(vals[:16]) + rng.sample(vals, 84)
    out = [(0, 0)]
    for e in base:
        out += [(e, 0), (0, e), (e, e), (e, (-e) % Q)]
    out += [(rng.choice(vals), rng.choice(vals)) for _ in range(300)]
    return tuple(dict.fromkeys(out))


def _w2(elems):
    return np.hstack([words([e[0] for e in elems]), words([e[1] for e in elems])])


@functools.lru_cache(maxsize=None)
def fq2_cases():
    els = fq2_elements()
    rng = random.Random(0xF93)
    rinv = pow(RR, -1, Q)
    val = lambda a: (a[0] * rinv % Q, a[1] * rinv % Q)  # noqa: E731
    mont = lambda a: (a[0] * RR % Q, a[1] * RR % Q)  # noqa: E731
    ops, A, B, res = [], [], [], []

    def put(op, a, b, r):
        ops.append(op), A.append(a), B.append(b), res.append(r)

    for a in els:
        for b in [a] + rng.sample(els, 4):
            put(E_ADD, a, b, ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
            put(E_SUB, a, b, ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
            put(E_MUL, a, b, mont(f2mul(val(a), val(b))))
        z = (0, 0)
        put(E_NEG, a, z, ((-a[0]) % Q, (-a[1]) % Q))
        put(E_DBL, a, z, (2 * a[0] % Q, 2 * a[1] % Q))
        put(E_SQR, a, z, mont(f2mul(val(a), val(a))))
        put(E_INV, a, z, mont(f2inv(val(a))))  # 0 -> 0
        put(E_TO_MONT, a, z, mont(a))
        put(E_FROM_MONT, a, z, val(a))
    rec = np.zeros((len(ops), WORDS_IN[FQ2]), np.uint32)
    rec[:, 0] = ops
    rec[:, 1:17], rec[:, 17:33] = _w2(A), _w2(B)
    return rec, _w2(res), np.array(ops)


# ---------------- curves: the affine law on y^2 = x^3 + b' ----------------
class _Fq:
    zero, one, E = 0, 1, 8
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    inv = staticmethod(lambda a: pow(a, -1, Q))
    mont = staticmethod(lambda a: a * RR % Q)
    val = staticmethod(lambda a: a * _RINV_Q % Q)
    w = staticmethod(words)
    edge = staticmethod(lambda rng: rng.choice(edge_residues(Q)))


class _Fq2:
    zero, one, E = (0, 0), (1, 0), 16
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
    mul = staticmethod(f2mul)
    inv = staticmethod(f2inv)
    mont = staticmethod(lambda a: (a[0] * RR % Q, a[1] * RR % Q))
    val = staticmethod(lambda a: (_Fq.val(a[0]), _Fq.val(a[1])))
    w = staticmethod(_w2)
    edge = staticmethod(lambda rng: (rng.choice(edge_residues(Q)), rng.choice(edge_residues(Q))))


FIELD_OF = {CURVE_Q: _Fq, CURVE_Q2: _Fq2}


def aff_add(F, P, S):
    """chord and tangent, a = 0; None = infinity.  P and S lie on one curve y^2 = x^3 + b'."""
    if P is None:
        return S
    if S is None:
        return P
    (x1, y1), (x2, y2) = P, S
    if x1 == x2:
        if y1 != y2 or y1 == F.zero:
            return None  # S = -P; or a point with y = 0, which is its own inverse
        x1s = F.mul(x1, x1)
        lam = F.mul(F.add(F.add(x1s, x1s), x1s), F.inv(F.add(y1, y1)))
    else:
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def aff_neg(F, P):
    return None if P is None else (P[0], F.sub(F.zero, P[1]))


def aff_mul(F, P, k):
    if k < 0:
        return aff_mul(F, aff_neg(F, P), -k)
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = aff_add(F, acc, acc)
        if bit == "1":
            acc = aff_add(F, acc, P)
    return acc


def scaled(F, P, lam, junk):
    """stored XYZZ coordinates (X l^2, Y l^3, l^2, l^3) of the affine VALUE point P; infinity = (junk, junk, 0, 0)"""
    if P is None:
        return (junk[0], junk[1], F.zero, F.zero)
    l2 = F.mul(lam, lam)
    l3 = F.mul(l2, lam)
    return tuple(F.mont(v) for v in (F.mul(P[0], l2), F.mul(P[1], l3), l2, l3))


ADD_AFF_KS = (0, 1, -1, 2, 3)
ADD_JKS = ((0, 1), (1, 0), (0, 0), (1, 1), (1, -1), (-1, 1), (2, 1), (1, 2), (3, 1), (2, 3), (3, -3))
N_CURVE_PAIRS = 256


@functools.lru_cache(maxsize=None)
def curve_pairs(family):
    """N_CURVE_PAIRS stored coordinate pairs (x, y) from the edge set: (0, 0) = infinity, x = 0 with y != 0 (an ordinary point),
    y = 0 (doubles to infinity), x = y, and seeded pairs"""
    F = FIELD_OF[family]
    rng = random.Random(0xC0 + family)
    z = F.zero
    out = [(z, z)]
    for shape in (0, 1, 0, 1, 0, 1, 2, 2):
        e = F.edge(rng)
        while e == z:
            e = F.edge(rng)
        out.append(((z, e), (e, z), (e, e))[shape])
    while len(out) < N_CURVE_PAIRS:
        p = (F.edge(rng), F.edge(rng))
        if p not in out:
            out.append(p)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def curve_cases(family):
    """(records, expected, ops): per coordinate pair P the round trip, aff_dbl, xyzz_dbl of a scaled P, xyzz_add_aff(scaled k P, P)
    for k in ADD_AFF_KS, xyzz_add(scaled j P, scaled k P) for (j, k) in ADD_JKS, xyzz_mul_small(scaled P, k) for k in
    MUL_SMALL_KS and both additions of P and (w x, y); then on_curve of real curve points and of the same points with y + 1"""
    F = FIELD_OF[family]
    E = F.E
    rng = random.Random(0xCA + family)
    zero4 = (F.zero,) * 4
    w3 = next(w for w in (pow(g, (Q - 1) // 3, Q) for g in range(2, 50)) if w != 1)
    omega = w3 if family == CURVE_Q else (w3, 0)
    ops, ks, Ps, Qs, res = [], [], [], [], []

    def lam():
        while True:
            v = F.val(F.edge(rng))
            if v != F.zero:
                return v

    def put(op, P4, Q4, want, k=0):
        ops.append(op), ks.append(k), Ps.append(P4), Qs.append(Q4), res.append(want)

    for xs, ys in curve_pairs(family):
        stored = (xs, ys, F.zero, F.zero)
        P = None if (xs, ys) == (F.zero, F.zero) else (F.val(xs), F.val(ys))
        mult = {k: aff_mul(F, P, k) for k in (-3, -1, 0, 1, 2, 3)}
        put(C_ROUNDTRIP, zero4, stored, P)
        put(C_AFF_DBL, zero4, stored, mult[2])
        put(C_XYZZ_DBL, scaled(F, P, lam(), (xs, ys)), zero4, mult[2])
        for k in ADD_AFF_KS:
            put(C_ADD_AFF, scaled(F, mult[k], lam(), (xs, ys)), stored, aff_add(F, mult[k], P))
        for k in (1, 2):  # affine (0, 0) = infinity beside a finite accumulator: the sum is the accumulator
            put(C_ADD_AFF, scaled(F, mult[k], lam(), (xs, ys)), zero4, mult[k])
        for j, k in ADD_JKS:
            put(C_ADD, scaled(F, mult[j], lam(), (xs, ys)), scaled(F, mult[k], lam(), (ys, xs)), aff_add(F, mult[j], mult[k]))
        for k in MUL_SMALL_KS:
            put(C_MUL_SMALL, scaled(F, P, lam(), (xs, ys)), zero4, aff_mul(F, P, k), k)
        # the other point of the same curve with the same y: (w x, y), w^3 = 1.  Equal y, unequal x: neither doubling nor inverse
        S = None if P is None else (F.mul(omega, P[0]), P[1])
        put(C_ADD_AFF, scaled(F, P, lam(), (xs, ys)), scaled(F, S, F.one, (xs, ys)), aff_add(F, P, S))
        put(C_ADD, scaled(F, P, lam(), (xs, ys)), scaled(F, S, lam(), (ys, xs)), aff_add(F, P, S))
    n_law = len(ops)
    flags = [int(w is None) for w in res]
    # on_curve: real points, and the same with y + 1
    import bn254_ref as ref

    G, RF = (ref.G1_GEN, ref.G1F) if family == CURVE_Q else (ref.G2_GEN, ref.G2F)
    for k in range(1, 9):
        x, y = ref.mul(RF, G, k)
        for good, yy in ((1, y), (0, F.add(y, F.one))):
            put(C_ON_CURVE, zero4, (F.mont(x), F.mont(yy), F.zero, F.zero), None)
            flags.append(good)
    put(C_ON_CURVE, zero4, zero4, None)  # infinity is on the curve
    flags.append(1)
    rec = np.zeros((len(ops), WORDS_IN[family]), np.uint32)
    rec[:, 0], rec[:, 1] = ops, ks
    for c in range(4):
        rec[:, 2 + c * E:2 + (c + 1) * E] = F.w([p[c] for p in Ps])
        rec[:, 2 + (4 + c) * E:2 + (5 + c) * E] = F.w([q[c] for q in Qs])
    exp = np.zeros((len(ops), WORDS_OUT[family]), np.uint32)
    exp[:, :E] = F.w([F.zero if w is None else w[0] for w in res])
    exp[:, E:2 * E] = F.w([F.zero if w is None else w[1] for w in res])
    exp[:, 2 * E] = flags
    assert n_law == len(curve_pairs(family)) * (7 + len(ADD_AFF_KS) + len(ADD_JKS) + len(MUL_SMALL_KS))
    return rec, exp, np.array(ops)


def on_curve_records(family, stored_points):
    """C_ON_CURVE records of stored affine points ((x, y) as F's stored patterns, coordinates up to 2^256 - 1)"""
    F = FIELD_OF[family]
    E = F.E
    rec = np.zeros((len(stored_points), WORDS_IN[family]), np.uint32)
    rec[:, 0] = C_ON_CURVE
    rec[:, 2 + 4 * E:2 + 5 * E] = F.w([p[0] for p in stored_points])
    rec[:, 2 + 5 * E:2 + 6 * E] = F.w([p[1] for p in stored_points])
    return rec


@functools.lru_cache(maxsize=None)
def noncanonical_points(family):
    """encodings of k G (k = 1 .. 8, Montgomery form) with multiples of q added to their coordinates: the same residues, limbs not
    below q.  G1: every (i q, j q) != (0, 0) with i, j < 4 on (x, y), 120 encodings; G2: i q on one of the four coordinates, 96."""
    import bn254_ref as ref

    out = []
    for k in range(1, 9):
        if family == CURVE_Q:
            x, y = (_Fq.mont(v) for v in ref.mul(ref.G1F, ref.G1_GEN, k))
            out += [(x + i * Q, y + j * Q) for i in range(4) for j in range(4) if i or j]
        else:
            x, y = (_Fq2.mont(v) for v in ref.mul(ref.G2F, ref.G2_GEN, k))
            c = [x[0], x[1], y[0], y[1]]
            for pos in range(4):
                for i in (1, 2, 3):
                    d = list(c)
                    d[pos] += i * Q
                    out.append(((d[0], d[1]), (d[2], d[3])))
    return tuple(out)


def noncanonical_doubling(family):
    """(records, expected): xyzz_add_aff(P, P') with P = k G in reduced coordinates (ZZ = ZZZ = 1) and P' each encoding of
    noncanonical_points; expected is 2 k G, what the sum of a point and another encoding of ITSELF should be.  Where the code
    answers otherwise, its limb compares missed the doubling branch: the reason bx_groth16_key_load refuses such coordinates."""
    import bn254_ref as ref

    F = FIELD_OF[family]
    E = F.E
    G, RF = (ref.G1_GEN, ref.G1F) if family == CURVE_Q else (ref.G2_GEN, ref.G2F)
    pts = noncanonical_points(family)
    per = len(pts) // 8
    rec = on_curve_records(family, pts)
    rec[:, 0] = C_ADD_AFF
    exp = np.zeros((len(pts), WORDS_OUT[family]), np.uint32)
    for k in range(1, 9):
        x, y = ref.mul(RF, G, k)
        rows = slice((k - 1) * per, k * per)
        for c, v in enumerate((F.mont(x), F.mont(y), F.mont(F.one), F.mont(F.one))):
            rec[rows, 2 + c * E:2 + (c + 1) * E] = F.w([v])
        x2, y2 = ref.mul(RF, G, 2 * k)
        exp[rows, :E], exp[rows, E:2 * E] = F.w([x2]), F.w([y2])
    return rec, exp


@functools.lru_cache(maxsize=None)
def cases(family):
    """(records, expected, ops) of a family"""
    if family == FIELD_Q:
        return field_cases(Q)
    if family == FIELD_R:
        return field_cases(FR)
    if family == FQ2:
        return fq2_cases()
    return curve_cases(family)


# ---------------- the two builds ----------------
OUT = os.path.join(HERE, "_build", "bn254_edge")
HOST_SRC, DEV_SRC, OPS_HDR = (os.path.join(HERE, f) for f in ("bn254_edge_host.cpp", "bn254_edge_dev.hip", "bn254_edge_ops.hpp"))
HOST, HOST_SAN, DEV = (os.path.join(OUT, f) for f in ("bn254_edge_host", "bn254_edge_host_san", "libbn254_edge_dev.so"))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _csrc():
    return os.path.join(ROOT, "boundless_amd", "csrc")


def _stamp(flags, srcs):
    """what a build product depends on: its compile flags (include paths left out: they name where the tree lies) and the TEXT of
    its sources.  Kept beside the product as <product>.stamp; contents, not mtimes, so a copy of the tree stays fresh and a change
    of a flag or of a compile line here rebuilds."""
    import hashlib

    h = hashlib.sha256("\n".join(f for f in flags if not f.startswith("-I")).encode())
    for s in srcs:
        h.update(b"\0" + os.path.basename(s).encode() + b"\0" + open(s, "rb").read())
    return h.hexdigest()


def _fresh(out, stamp):
    path = out + ".stamp"
    return os.path.exists(out) and os.path.exists(path) and open(path).read().strip() == stamp


def _done(out, stamp):
    with open(out + ".stamp", "w") as f:
        f.write(stamp + "\n")


def _run(cmd, what):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building {what} failed:\n{r.stdout}{r.stderr}")


def _host_flags(sanitized):
    return ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + (SANITIZE + ["-g"] if sanitized else [])


def build_host(sanitized, force=False, csrc=None, out=None):
    """the host program, plain or sanitized (g++ only), rebuilt when its flags or sources changed; csrc / out: another copy of the
    arithmetic header and where to put the program (the mutation table of the change that added these tests was made this way)"""
    out = out or (HOST_SAN if sanitized else HOST)
    csrc = csrc or _csrc()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = _host_flags(sanitized)
    stamp = _stamp(flags, [HOST_SRC, OPS_HDR, os.path.join(csrc, "bn254_arith.hpp")])
    if force or not _fresh(out, stamp):
        _run(flags + [f"-I{csrc}", HOST_SRC, "-o", out], os.path.basename(out))
        _done(out, stamp)
    return out


DEV_UNITS = [CURVE_Q2, CURVE_Q, FQ2, FIELD_Q, FIELD_R, "run"]  # the slowest first


def _dev_flags(unit):
    from boundless_amd import build as b

    define = [] if unit == "run" else [f"-DBN_EDGE_FAMILY={unit}"]
    return ["hipcc", "-x", "hip"] + b.FLAGS + define + [f"-cuid=bxbn254edgedev{unit}"]


def _dev_link_flags():
    from boundless_amd import build as b

    return ["hipcc", "-shared", "-fPIC", f"--offload-arch={b.ARCH}", "-fno-gpu-rdc"]


def _dev_stamp():
    from boundless_amd import build as b

    flags = [f for u in DEV_UNITS for f in _dev_flags(u)] + _dev_link_flags()
    return _stamp(flags, [DEV_SRC, OPS_HDR, os.path.join(b.CSRC, "bn254_arith.hpp")])


def _dev_unit(unit):
    """one translation unit of the device module: family 0 .. 4 (its kernel and launch), or "run" (the runner)"""
    obj = os.path.join(OUT, f"dev_{unit}.o")
    _run(_dev_flags(unit) + ["-c", DEV_SRC, "-o", obj], f"tests/bn254_edge_dev.hip ({unit})")
    return obj


def build(force=False):
    """both host programs and the device module; the module's six translation units are compiled side by side"""
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(max_workers=8) as ex:
        jobs = [ex.submit(build_host, False, force), ex.submit(build_host, True, force)]
        stamp = _dev_stamp()
        if force or not _fresh(DEV, stamp):
            objs = list(ex.map(_dev_unit, DEV_UNITS))
            _run(_dev_link_flags() + ["-o", DEV] + objs, os.path.basename(DEV))
            _done(DEV, stamp)
        for j in jobs:
            j.result()
    return OUT


def host_program(sanitized):
    """the host program of the tree's present sources: build_host() costs nothing while its stamp matches (so nothing is compiled
    where build() made it from the same sources, a copy of the tree included) and rebuilds after an edit of the header"""
    return build_host(sanitized)


def dev_path():
    """the device module build() made; never compiled from a test (hipcc's minutes belong to build())"""
    assert _fresh(DEV, _dev_stamp()), (f"{DEV} is missing or was built from other sources or flags: run build() "
                                       "(__graft_entry__.build() compiles the edge-operand device module)")
    return DEV


def run_host(family, records, workdir, sanitized=False, program=None):
    """records through the host program as an ordinary child process -> (result rows, the result file's bytes)"""
    records = np.ascontiguousarray(records, dtype=np.uint32)
    assert records.shape[1] == WORDS_IN[family]
    tag = FAMILY_NAMES[family] + ("_san" if sanitized else "")
    fin, fout = os.path.join(str(workdir), tag + ".in"), os.path.join(str(workdir), tag + ".out")
    with open(fin, "wb") as f:
        f.write(np.array([MAGIC, family, len(records), records.shape[1]], dtype="<u4").tobytes())
        f.write(records.astype("<u4").tobytes())
    r = subprocess.run([program or host_program(sanitized), fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{tag}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    raw = open(fout, "rb").read()
    assert len(raw) == 4 * len(records) * WORDS_OUT[family], f"{tag}: result file of {len(raw)} bytes"
    return np.frombuffer(raw, dtype="<u4").reshape(len(records), WORDS_OUT[family]).astype(np.uint32), raw


_dev = None


def run_dev(family, records):
    """records through the device module: one launch -> result rows"""
    global _dev
    if _dev is None:
        _dev = C.CDLL(dev_path())
        _dev.bn254_edge_run.restype = C.c_int
        _dev.bn254_edge_run.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    records = np.ascontiguousarray(records, dtype=np.uint32)
    assert records.shape[1] == WORDS_IN[family]
    out = np.zeros((len(records), WORDS_OUT[family]), np.uint32)
    e = _dev.bn254_edge_run(family, records.ctypes.data, len(records), out.ctypes.data)
    assert e == 0, f"bn254_edge_run({FAMILY_NAMES[family]}): HIP error {e}"
    return out
