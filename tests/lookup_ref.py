"""Definition-level restatement of the lookup circuit of include/bx_lookup.h ("The lookup circuit"), written from that text and
sharing no code with the library: the code cells, the data witness with the segment's cell records applied, the multiplicities, the
LogUp running sums for a given alpha, every constraint on a trace row, the mixed constraint polynomial from tap values and the
check quotient over the 4N domain.

Field arithmetic is tests/logup_ref.py's (Python ints; lists of 4 for Fp4 = Fp[X]/(X^4 + 11)).  Whole columns are generated with
numpy (uint64, wrapping like the C arithmetic of splitmix64) so that a 2^17-row trace stays cheap; everything that is a constraint
is evaluated on Python ints.  Words on the ABI are Montgomery words x * 2^32 mod P.
"""
import numpy as np

import logup_ref as lr

P = lr.P
GOLDEN = 0x9E3779B97F4A7C15
CODE_SEED = 0x4C4F4F4B55502121  # "LOOKUP!!"
NOISE_TWEAK = 0x5A4B4E4F49534521
M64 = (1 << 64) - 1
MAX_RECORDS = 65536


def splitmix64(x):
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(seed, col, row):
    v = splitmix64(seed ^ ((col << 32) | row)) >> 33
    return v - P if v >= P else v


def word_column(seed, col, rows):
    """word(seed, col, r) for r in `rows` (a numpy array of row indices)"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed & M64) ^ (np.uint64(col << 32) | rows.astype(np.uint64))
        z = x + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    v = z >> np.uint64(33)
    return np.where(v >= P, v - np.uint64(P), v)


def encode_arr(vals):
    return ((np.asarray(vals, np.uint64) % np.uint64(P)) << np.uint64(32)) % np.uint64(P)


class Shape:
    def __init__(self, po2, w_code, w_data, w_accum):
        self.po2, self.wc, self.wd, self.wa = po2, w_code, w_data, w_accum
        self.N = 1 << po2
        self.Z = min(1994, self.N // 4)
        self.A = self.N - self.Z
        self.b = min(15, po2 - 1)
        self.B = 1 << self.b
        self.V = min((w_data - 1) // 3 if w_data else 0, ((w_accum // 4) - 1) // 2 if w_accum >= 4 else 0)
        self.S = 2 * self.V + 1
        self.constraints = 3 * self.V + 4

    def limb_col(self, s):
        return 3 * (s // 2) + 1 + s % 2


def normalize(po2, w_code, w_data, w_accum, cons_terms=0, cons_degree=0):
    """None when the shape is a legal one, else why not (the knobs stay 0)"""
    if cons_terms or cons_degree:
        return "knobs"
    if not 9 <= po2 <= 24:
        return "po2"
    if w_code < 3:
        return "w_code"
    sh = Shape(po2, w_code, w_data, w_accum)
    if sh.V == 0:
        return "no value column"
    if sh.V > 63:
        return "too many value columns"
    return None


def taps(sh, group, col):
    return [0, 1] if group == 2 and col < 4 * sh.S else [0]


def n_globals(sh):
    return 2


def code_columns(sh):
    """(w_code, N) Montgomery words"""
    rows = np.arange(sh.N)
    code = np.zeros((sh.wc, sh.N), np.uint64)
    code[0][0] = lr.encode(1)
    code[1][sh.A - 1] = lr.encode(1)
    code[2][:sh.B] = encode_arr(rows[:sh.B])
    for c in range(3, sh.wc):
        code[c] = word_column(CODE_SEED, c, rows)
    return code.astype(np.uint32)


def decode_records(payload, sh):
    """payload bytes -> [(col, row, value)], or ValueError naming what is wrong"""
    if len(payload) % 12:
        raise ValueError("not a whole number of 12-byte cell records")
    recs = [tuple(int.from_bytes(payload[k + 4 * q:k + 4 * q + 4], "little") for q in range(3)) for k in range(0, len(payload), 12)]
    if len(recs) > MAX_RECORDS:
        raise ValueError("more than 65536 cell records")
    for col, row, value in recs:
        if col >= 3 * sh.V or row >= sh.A or value >= P:
            raise ValueError("out of bounds")
    return recs


def data_columns(sh, seed, noise_seed=None, records=()):
    """(w_data, N) Montgomery words and the two public words (g_0, g_1)"""
    if noise_seed is None:
        noise_seed = splitmix64(seed ^ NOISE_TWEAK)
    gseed, nseed = (seed + 2 * GOLDEN) & M64, (noise_seed + 2 * GOLDEN) & M64
    act, noise = np.arange(sh.A), np.arange(sh.A, sh.N)
    data = np.zeros((sh.wd, sh.N), np.uint64)
    for c in range(sh.wd):
        data[c][sh.A:] = word_column(nseed, c, noise)  # the v_j are overwritten below
    mont_b = lr.encode(sh.B)
    for j in range(sh.V):
        lo = word_column(gseed, 3 * j + 1, act) % np.uint64(sh.B)
        hi = word_column(gseed, 3 * j + 2, act) % np.uint64(sh.B) if j % 2 == 0 else np.zeros(sh.A, np.uint64)
        data[3 * j][:sh.A] = encode_arr(lo + np.uint64(sh.B) * hi)
        data[3 * j + 1][:sh.A] = encode_arr(lo)
        data[3 * j + 2][:sh.A] = encode_arr(hi)
        # noise rows: v = lo + B * hi in the field (Montgomery words: word * mont_b * 2^-32)
        nlo, nhi = data[3 * j + 1][sh.A:], data[3 * j + 2][sh.A:]
        data[3 * j][sh.A:] = (nlo + nhi * np.uint64(mont_b) % np.uint64(P) * np.uint64(lr.R_INV) % np.uint64(P)) % np.uint64(P)
    for c in range(3 * sh.V + 1, sh.wd):
        data[c][:sh.A] = word_column(gseed, c, act)
    for col, row, value in records:  # in order: the last record of a cell wins
        assert col < 3 * sh.V and row < sh.A and value < P
        data[col][row] = lr.encode(value)
    # multiplicities: how many (limb column, active row) cells hold the value r, for r < B
    counts = np.zeros(sh.B, np.uint64)
    for s in range(2 * sh.V):
        vals = data[sh.limb_col(s)][:sh.A] * np.uint64(lr.R_INV) % np.uint64(P)
        counts += np.bincount(vals[vals < sh.B].astype(np.int64), minlength=sh.B).astype(np.uint64)
    data[3 * sh.V][:sh.B] = encode_arr(counts)
    data[3 * sh.V][sh.B:sh.A] = 0
    return data.astype(np.uint32), (int(data[0][0]), int(data[0][sh.A - 1]))


def accum_columns(sh, seed, code, data, alpha_words):
    """(w_accum, N) Montgomery words: the 2V + 1 running sums for the challenge alpha (4 Montgomery words), then the filler"""
    alpha = [int(w) for w in alpha_words]
    den = np.zeros((sh.S, sh.N, 4), np.uint64)
    den[:, :, 1:] = np.array(alpha[1:], np.uint64)
    mults = np.full((sh.S, sh.N), lr.encode(1), np.uint64)
    for s in range(2 * sh.V):
        den[s, :, 0] = (np.uint64(alpha[0] + P) - data[sh.limb_col(s)].astype(np.uint64)) % np.uint64(P)
    den[2 * sh.V, :, 0] = (np.uint64(alpha[0] + P) - code[2].astype(np.uint64)) % np.uint64(P)
    mults[2 * sh.V] = (np.uint64(P) - data[3 * sh.V].astype(np.uint64)) % np.uint64(P)
    sums = lr.logup_accumulate_big(den.astype(np.uint32).ravel(), mults.astype(np.uint32).ravel(), sh.S).reshape(sh.S, sh.N, 4)
    accum = np.zeros((sh.wa, sh.N), np.uint64)
    for s in range(sh.S):
        for k in range(4):
            accum[4 * s + k] = sums[s, :, k]
    fseed = ((seed + 3 * GOLDEN) & M64) ^ ((alpha[0] << 32) | alpha[1])
    for c in range(4 * sh.S, sh.wa):
        accum[c] = word_column(fseed, c, np.arange(sh.N))
    return accum.astype(np.uint32)


# ---- constraints (Python ints; an ext element is a list of 4 values) ----
def ext(x):
    return [x % P, 0, 0, 0]


def f4_sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def constraint_values(sh, tap, alpha, g):
    """The 3V + 4 constraints, in mixing order, from tap(group, col, back) -> ext value; alpha an ext value, g the two public VALUES."""
    def run(s, back):
        return [tap(2, 4 * s + k, back) for k in range(4)]

    def as_ext(parts):  # sum_k X^k * part_k with ext parts
        r = [0, 0, 0, 0]
        for k, part in enumerate(parts):
            xk = [0, 0, 0, 0]
            xk[k] = 1
            r = lr.f4_add(r, lr.f4_mul(xk, part))
        return r

    first, last, table = tap(0, 0, 0), tap(0, 1, 0), tap(0, 2, 0)
    not_first = f4_sub(ext(1), first)
    out = []
    for j in range(sh.V):
        v, lo, hi = tap(1, 3 * j, 0), tap(1, 3 * j + 1, 0), tap(1, 3 * j + 2, 0)
        out.append(f4_sub(f4_sub(v, lo), lr.f4_scale(hi, sh.B)))
    total = [0, 0, 0, 0]
    for s in range(sh.S):
        cur, back = as_ext(run(s, 0)), as_ext(run(s, 1))
        step = f4_sub(cur, lr.f4_mul(not_first, back))
        total = lr.f4_add(total, cur)
        if s < 2 * sh.V:
            out.append(f4_sub(lr.f4_mul(step, f4_sub(alpha, tap(1, sh.limb_col(s), 0))), ext(1)))
        else:
            out.append(lr.f4_add(lr.f4_mul(step, f4_sub(alpha, table)), tap(1, 3 * sh.V, 0)))
    out.append(lr.f4_mul(last, total))
    v0 = tap(1, 0, 0)
    out.append(lr.f4_mul(first, f4_sub(v0, ext(g[0]))))
    out.append(lr.f4_mul(last, f4_sub(v0, ext(g[1]))))
    assert len(out) == sh.constraints
    return out


def mixed(sh, tap, poly_mix, alpha, g):
    """sum_i poly_mix^i C_i"""
    acc, cur = [0, 0, 0, 0], [1, 0, 0, 0]
    for cons in constraint_values(sh, tap, alpha, g):
        acc = lr.f4_add(acc, lr.f4_mul(cur, cons))
        cur = lr.f4_mul(cur, poly_mix)
    return acc


def row_tap(groups, n, r):
    """tap reader over trace rows: groups = (code, data, accum) matrices of VALUES (lists or arrays), row r, cyclic"""
    return lambda g, c, back: ext(int(groups[g][c][(r - back) % n]))


def decode_matrix(words):
    return (np.asarray(words, np.uint64) * np.uint64(lr.R_INV) % np.uint64(P))


def row_constraints(sh, code, data, accum, alpha_words, g_words, r):
    """every constraint on trace row r (matrices of Montgomery words)"""
    groups = (decode_matrix(code), decode_matrix(data), decode_matrix(accum))
    return constraint_values(sh, row_tap(groups, sh.N, r), [lr.decode(int(w)) for w in alpha_words], [lr.decode(int(w)) for w in g_words])


def check_quotient(sh, ecode, edata, eacc, poly_mix_words, alpha_words, g_words):
    """The four ext planes (4, 4N) of sum_i poly_mix^i C_i(x) / ((3x)^N - 1) over x = w_4N^row from the 4N evaluations (Montgomery
    words in and out); one row back is four domain points back."""
    dom = 4 * sh.N
    groups = (decode_matrix(ecode), decode_matrix(edata), decode_matrix(eacc))
    pm, alpha = [lr.decode(int(w)) for w in poly_mix_words], [lr.decode(int(w)) for w in alpha_words]
    g = [lr.decode(int(w)) for w in g_words]
    w4, t3n = pow(137, 1 << 25, P), pow(3, sh.N, P)
    zinv = [pow((t3n * pow(w4, m, P) - 1) % P, P - 2, P) for m in range(4)]
    out = np.zeros((4, dom), np.uint32)
    for i in range(dom):
        tap = lambda grp, c, back, i=i: ext(int(groups[grp][c][(i - 4 * back) % dom]))
        tot = lr.f4_scale(mixed(sh, tap, pm, alpha, g), zinv[i % 4])
        for k in range(4):
            out[k][i] = lr.encode(tot[k])
    return out
