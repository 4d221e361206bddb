"""Definition-level restatement of the synthetic circuit of include/bx_prover.h ("The synthetic circuit"), written from that text
and sharing no code with the library: the code cells, the data witness (free cells, permuted copies, derived columns), the grand
products for a given beta, every constraint in mixing order, and the check quotient over the 4N domain for ARBITRARY evaluation
matrices.

Arithmetic is numpy uint64 on Montgomery words (a word is x * 2^32 mod P, canonical in [0, P)): the Montgomery product of two words is
a * b * 2^-32 mod P, and a * b % P * RINV % P fits 64 bits.  Everything is vectorised over rows / domain points; an element of
Fp4 = Fp[X]/(X^4 + 11) is a trailing axis of 4 words.  The constraints are written once over a small field interface, so the same text
evaluates them on base-field cells (trace rows, the 4N evaluations) and on ext-field tap values (the verifier's point Z).
"""
import numpy as np

P = 2013265921
R = (1 << 32) % P  # the Montgomery word of 1
RINV = pow(R, P - 2, P)
GOLDEN = 0x9E3779B97F4A7C15
CODE_SEED = 0x434F4E54524F4C21  # "CONTROL!"
NOISE_TWEAK = 0x5A4B4E4F49534521
M64 = (1 << 64) - 1
DEFAULT_TERMS, DEFAULT_DEGREE = 64, 4
POOL = 16
_P, _RINV = np.uint64(P), np.uint64(RINV)


def encode(x):
    return x % P * R % P


def decode(w):
    return int(w) * RINV % P


def splitmix64(x):
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word_column(seed, col, rows):
    """word(seed, col, r) = splitmix64(seed ^ (col << 32 | r)) >> 33, minus P if >= P, for r in `rows`"""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed & M64) ^ (np.uint64(col << 32) | rows.astype(np.uint64))) + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    v = z >> np.uint64(33)
    return np.where(v >= _P, v - _P, v)


# ---- the two fields (Montgomery words, uint64 arrays) ----
def _u64(a):
    return np.asarray(a, np.uint64)


class Base:
    """Fp: arrays of words"""
    @staticmethod
    def const(word, like):
        return np.full(np.shape(like), word, np.uint64)

    @staticmethod
    def add(a, b):
        return (_u64(a) + _u64(b)) % _P

    @staticmethod
    def sub(a, b):
        return (_u64(a) + _P - _u64(b)) % _P

    @staticmethod
    def mul(a, b):
        return _u64(a) * _u64(b) % _P * _RINV % _P

    @staticmethod
    def to_ext(a):
        a = _u64(a)
        out = np.zeros(a.shape + (4,), np.uint64)
        out[..., 0] = a
        return out


class Ext:
    """Fp4 = Fp[X] / (X^4 + 11): arrays of words with a trailing axis of 4"""
    ELEVEN = np.uint64(encode(11))

    @staticmethod
    def const(word, like):
        out = np.zeros(np.shape(like), np.uint64)
        out[..., 0] = word
        return out

    add = Base.add
    sub = Base.sub

    @staticmethod
    def mul(a, b):
        a, b = np.broadcast_arrays(_u64(a), _u64(b))
        prod = [np.zeros(a.shape[:-1], np.uint64) for _ in range(7)]
        for i in range(4):
            for j in range(4):
                prod[i + j] = prod[i + j] + Base.mul(a[..., i], b[..., j])  # at most 4 words < 2^31 each
        out = np.zeros(a.shape, np.uint64)
        for k in range(4):
            out[..., k] = prod[k] % _P
            if k < 3:  # X^(k+4) = -11 X^k
                out[..., k] = Base.sub(out[..., k], Base.mul(Ext.ELEVEN, prod[k + 4] % _P))
        return out

    @staticmethod
    def to_ext(a):
        return _u64(a)


def ext_scale(e, b):
    """ext (.., 4) times base (..)"""
    return Base.mul(_u64(e), _u64(b)[..., None])


def ext_pow(a, n):
    r, a = Ext.const(R, np.zeros(4)), _u64(a)
    while n:
        if n & 1:
            r = Ext.mul(r, a)
        a = Ext.mul(a, a)
        n >>= 1
    return r


# ---- shape rules ----
class Shape:
    def __init__(self, po2, wc, wd, wa, T=0, G=0):
        self.po2, self.wc, self.wd, self.wa = po2, wc, wd, wa
        self.T, self.G = T or DEFAULT_TERMS, G or DEFAULT_DEGREE
        self.N = 1 << po2
        self.Z = min(1994, self.N // 4)
        self.A = self.active_rows = self.N - self.Z
        self.F = (wd + 1) // 2  # ceil(w_data / 2) free columns
        self.J = wd - self.F
        self.E = wa // 4
        self.pairs = sum(1 for p in range(max(self.E, self.F)) if 2 * p + 1 < self.E and 4 * p + 3 < self.F) if wc >= 2 else 0
        self.globals = 2 if wc >= 2 else 1
        self.constraints = self.J + self.E + self.pairs + self.globals

    def acc_src(self, e):
        p = e // 2
        if p < self.pairs:
            return 4 * p + 2 + e % 2
        return e % self.F

    def csel_col(self, i):
        """the code column behind csel(i), None for the constant 1"""
        return 2 + i % (self.wc - 2) if self.wc >= 3 else None

    @staticmethod
    def slot1_back(j):
        return 1 if j % 8 == 0 else 2 if j % 8 == 4 else 0

    @staticmethod
    def pool_idx(t, f):
        return (7 * t + 3 * f + (t // 4) * f + t // 16) % 16

    def perm(self, p, rows):
        return (rows.astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345 + p)) % np.uint64(self.A)

    def taps(self, group, col):
        if group == 1 and col % 8 == 0:
            return [0, 1]
        if group == 1 and col % 8 == 4:
            return [0, 1, 2]
        if group == 2 and col < 4 * self.E:
            return [0, 1]
        return [0]


def pool_sources(sh, j):
    """the 16 pool entries of derived column F + j as (group, col, back); group None = the constant 1"""
    def csel(i):
        c = sh.csel_col(i)
        return (None, 0, 0) if c is None else (0, c, 0)

    src = [(1, j, 0), (1, j, sh.slot1_back(j)), (1, (j + 1) % sh.F, 0), (1, (j + 2) % sh.F, 0)]
    for s in range(1, 9):
        src.append((1, sh.F + j - s, 0) if j >= s else csel(s - j - 1))
    src += [csel(j + q) for q in range(4)]
    assert len(src) == POOL
    return src


def cons_sum(sh, pool, field=Base):
    """sum_{t<T} prod_{f<G} pool[idx(t, f)] for a pool of 16 field elements (arrays)"""
    total = field.const(0, pool[0])
    for t in range(sh.T):
        prod = _u64(pool[sh.pool_idx(t, 0)])
        for f in range(1, sh.G):
            prod = field.mul(prod, pool[sh.pool_idx(t, f)])
        total = field.add(total, prod)
    return total


# ---- the witness ----
def code_columns(sh):
    """(w_code, N) words: first, last, then the control words"""
    rows = np.arange(sh.N)
    code = np.zeros((sh.wc, sh.N), np.uint64)
    code[0][0] = R
    if sh.wc >= 2:
        code[1][sh.A - 1] = R
    for c in range(2, sh.wc):
        code[c] = word_column(CODE_SEED, c, rows)
    return code.astype(np.uint32)


def data_columns(sh, seed, noise_seed=None):
    """(w_data, N) words and the public words (g_0[, g_1])"""
    if noise_seed is None:
        noise_seed = splitmix64(seed ^ NOISE_TWEAK)
    gseed, nseed = (seed + 2 * GOLDEN) & M64, (noise_seed + 2 * GOLDEN) & M64
    act, noise = np.arange(sh.A), np.arange(sh.A, sh.N)
    code = code_columns(sh).astype(np.uint64)
    data = np.zeros((sh.wd, sh.N), np.uint64)
    for c in range(sh.F):
        data[c][:sh.A] = word_column(gseed, c, act)
        data[c][sh.A:] = word_column(nseed, c, noise)
    for p in range(sh.pairs):
        data[4 * p + 3][sh.perm(p, act).astype(np.int64)] = data[4 * p + 2][:sh.A]
    for j in range(sh.J):
        data[sh.F + j] = cons_sum(sh, [_cells((code, data), src, 1) for src in pool_sources(sh, j)])
    g = (int(data[0][0]), int(data[sh.wd - 1][sh.A - 1]))[:sh.globals]
    return data.astype(np.uint32), g


def _cells(groups, src, step):
    """the array of cells a source names: column `col` of `group`, `back` rows back (cyclic; one row = `step` points)"""
    group, col, back = src
    if group is None:
        return np.full(groups[1].shape[1], R, np.uint64)
    return np.roll(_u64(groups[group][col]), back * step)


def betas(sh, mix):
    """beta_e = beta^(floor(e / 2) + 1), (E, 4)"""
    return np.array([ext_pow(mix, e // 2 + 1) for e in range(sh.E)], np.uint64).reshape(sh.E, 4)


def accum_columns(sh, seed, data, mix):
    """(w_accum, N) words: the E grand products for the challenge `mix` (4 words), then the noise columns"""
    accum = np.zeros((sh.wa, sh.N), np.uint64)
    if sh.E:
        fac = np.zeros((sh.E, sh.N, 4), np.uint64) + betas(sh, mix)[:, None, :]
        for e in range(sh.E):
            fac[e, :, 0] = Base.add(fac[e, :, 0], data[sh.acc_src(e)])
        run = Ext.const(R, np.zeros((sh.E, 4)))
        for r in range(sh.N):
            run = Ext.mul(run, fac[:, r])
            accum[:4 * sh.E, r] = run.reshape(-1)  # component k of accumulator e in column 4e + k
    fseed = ((seed + 3 * GOLDEN) & M64) ^ ((int(mix[0]) << 32) | int(mix[1]))
    for c in range(4 * sh.E, sh.wa):
        accum[c] = word_column(fseed, c, np.arange(sh.N))
    return accum.astype(np.uint32)


# ---- constraints ----
def constraint_values(sh, tap, mix, g, field, memo=None):
    """The constraints in mixing order from tap(group, col, back) -> element of `field` (Base: cells; Ext: tap values at Z), mix the 4
    words of beta, g the public words.  The first J and the boundary constraints are elements of `field`, the accumulator and closing
    constraints ext; all are returned as ext arrays.  `memo`: a dict the caller keeps for ONE set of tap values — the first J
    constraints depend on nothing else and are computed once for it."""
    one = None

    def cell(src):
        nonlocal one
        if src[0] is None:
            if one is None:
                one = field.const(R, tap(0, 0, 0))
            return one
        return tap(*src)

    def acc(e, back):  # sum_k X^k * column 4e + k
        total = 0
        for k in range(4):
            xk = np.zeros(4, np.uint64)
            xk[k] = R
            total = Ext.add(total, Ext.mul(xk, field.to_ext(tap(2, 4 * e + k, back))))
        return total

    memo = {} if memo is None else memo
    if "derived" not in memo:
        memo["derived"] = [field.to_ext(field.sub(tap(1, sh.F + j, 0), cons_sum(sh, [cell(s) for s in pool_sources(sh, j)], field))) for j in range(sh.J)]
    out = list(memo["derived"])
    first = field.to_ext(tap(0, 0, 0))
    last = field.to_ext(tap(0, 1, 0)) if sh.wc >= 2 else None
    ext_one = Ext.const(R, first)
    bs = betas(sh, mix)
    for e in range(sh.E):
        prev = Ext.add(first, Ext.mul(Ext.sub(ext_one, first), acc(e, 1)))
        fac = Ext.add(bs[e], field.to_ext(tap(1, sh.acc_src(e), 0)))
        out.append(Ext.sub(acc(e, 0), Ext.mul(prev, fac)))
    for p in range(sh.pairs):
        out.append(Ext.mul(last, Ext.sub(acc(2 * p + 1, 0), acc(2 * p, 0))))
    out.append(Ext.mul(first, Ext.sub(field.to_ext(tap(1, 0, 0)), Ext.const(int(g[0]), first))))
    if sh.wc >= 2:
        out.append(Ext.mul(last, Ext.sub(field.to_ext(tap(1, sh.wd - 1, 0)), Ext.const(int(g[1]), first))))
    assert len(out) == sh.constraints
    return out


def mixed(sh, tap, poly_mix, mix, g, field, memo=None):
    """sum_i poly_mix^i C_i (ext)"""
    total, cur = 0, Ext.const(R, np.zeros(4))
    for cons in constraint_values(sh, tap, mix, g, field, memo):
        total = Ext.add(total, Ext.mul(cur, cons))
        cur = Ext.mul(cur, _u64(poly_mix))
    return total


def cell_tap(groups, step):
    """tap reader over whole matrices: every row (step 1) or every point of the 4N domain (step 4: one row back is four points back)"""
    return lambda group, col, back: _cells(groups, (group, col, back), step)


def row_constraints(sh, code, data, accum, mix, g):
    """every constraint on every trace row: a list of (N, 4) arrays"""
    return constraint_values(sh, cell_tap((code, data, accum), 1), mix, g, Base)


def check_quotient(sh, ecode, edata, eacc, poly_mix, mix, g, memo=None):
    """The four ext planes (4, 4N) of sum_i poly_mix^i C_i(x) / ((3x)^N - 1) over x = w_4N^row, from ANY three evaluation matrices
    (w, 4N) of words.  (3x)^N = 3^N w_4^(row mod 4) takes four values.  `memo` as in constraint_values: one dict per set of matrices."""
    dom = 4 * sh.N
    tot = mixed(sh, cell_tap((ecode, edata, eacc), 4), poly_mix, mix, g, Base, memo)
    w4, t3n = pow(137, 1 << 25, P), pow(3, sh.N, P)
    zinv = np.array([encode(pow((t3n * pow(w4, m, P) - 1) % P, P - 2, P)) for m in range(4)], np.uint64)
    return np.ascontiguousarray(ext_scale(tot, zinv[np.arange(dom) % 4]).T).astype(np.uint32)


# ---- what the tests run: every shape rule of the text is hit by one of these ----
SHAPES = [
    (1, 1, 1),      # one global, no selectors, J = 0, E = 0
    (2, 5, 4),      # `last` present, csel is the constant one, F = 3
    (3, 4, 6),      # F = 2: the pool's free columns wrap; noise accum columns
    (16, 24, 16),   # pairs > 0; taps one and two rows back; the ring of eight derived columns full
    (5, 17, 9),     # odd everything
]
# the four (T, G) the library compiles its constraint sum for, then three that take its run-time form
KNOBS = [(64, 4), (48, 3), (16, 3), (8, 2), (5, 2), (64, 5), (1, 1)]
