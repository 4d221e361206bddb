"""Definition-level reference of the RATIO step of accumulate programs (include/bx_program.h, "Accumulate programs"), on top of
tests/acc_program_ref.py, whose conventions it keeps: every fp var is a whole column of PLAIN field values, (N,) base or (N, 4) ext, a
tap `back` rows back is the column rolled, the Fp4 inverse is a^(P^4 - 2) (0 -> 0), and the running products are plain loops.

    RATIO s a b      sequence s is acc_s[r] = prod_{j <= r} fp[a](j) / fp[b](j); a and b are base or ext, a base value is promoted; a
                     zero denominator contributes the factor 0, so the sequence is 0 from that row on.         (BX_CONS_RATIO = 16)

Order: all SUMs are numbered below all PRODs, all PRODs below all RATIOs.

Also here: the named programs the tests run and a seeded random-program generator that follows the order rule.
"""
import numpy as np

import acc_program_ref as ref

P, U, _P = ref.P, ref.U, ref._P
OP_RATIO = 16  # BX_CONS_RATIO
WIDTHS, N_GLOBALS = ref.WIDTHS, ref.N_GLOBALS
ZERO_VALUE = ref.ZERO_VALUE


class Program(ref.Program):
    def ratio(self, s, a, b):
        self.steps.append((OP_RATIO, int(s), int(a), int(b), 0))

    def sequences(self):
        """{s: is it a sum}, over all three kinds"""
        return {st[1]: st[0] == ref.OP_SUM for st in self.steps if st[0] in (ref.OP_SUM, ref.OP_PROD, OP_RATIO)}

    def ratios(self):
        return sum(1 for st in self.steps if st[0] == OP_RATIO)


def evaluate(prog, po2, code, data, globals_, mix):
    """-> (4 S, N) uint32 Montgomery words: accum columns [0, 4 S)"""
    n = 1 << po2
    groups = [ref.decode(np.asarray(code, np.uint32).reshape(-1, n)), ref.decode(np.asarray(data, np.uint32).reshape(-1, n))]
    g, mx = ref.decode(list(globals_) + [0]), ref.decode(mix)
    fp, terms = [], {}
    for op, a, b, c, d in prog.steps:
        if op == ref.OP_CONST:
            fp.append(np.full(n, a, U))
        elif op == ref.OP_CONST_EXT:
            fp.append(np.tile(np.array([a, b, c, d], U), (n, 1)))
        elif op == ref.OP_GET:
            group, col, back = prog.taps[a]
            fp.append(np.roll(groups[group][col], back))
        elif op == ref.OP_GET_GLOBAL:
            fp.append(np.full(n, g[b] if a == 0 else mx[b], U))
        elif op in (ref.OP_ADD, ref.OP_SUB, ref.OP_MUL):
            x, y = fp[a], fp[b]
            if x.ndim != y.ndim:
                x, y = ref._lift(x), ref._lift(y)
            if op == ref.OP_ADD:
                fp.append((x + y) % _P)
            elif op == ref.OP_SUB:
                fp.append((x + _P - y) % _P)
            else:
                fp.append(ref.f4_mul(x, y) if x.ndim == 2 else x * y % _P)
        elif op == ref.OP_SUM:
            assert fp[b].ndim == 1 and a not in terms
            terms[a] = (True, ref.f4_mul(ref._lift(fp[b]), ref.f4_inv(ref._lift(fp[c]))))
        elif op == ref.OP_PROD:
            assert a not in terms
            terms[a] = (False, ref._lift(fp[b]))
        elif op == OP_RATIO:
            assert a not in terms
            terms[a] = (False, ref.f4_mul(ref._lift(fp[b]), ref.f4_inv(ref._lift(fp[c]))))
        else:
            raise ValueError(f"op {op} does not belong in an accumulate program")
    S = len(terms)
    assert sorted(terms) == list(range(S))
    out = np.zeros((4 * S, n), U)
    for s in range(S):
        is_sum, t = terms[s]
        rows = t.tolist()
        acc = [0, 0, 0, 0] if is_sum else [1, 0, 0, 0]
        for r in range(n):
            acc = [(x + y) % P for x, y in zip(acc, rows[r])] if is_sum else ref._mul_int(acc, rows[r])
            for k in range(4):
                out[4 * s + k][r] = acc[k]
    return (out * U(ref.R) % _P).astype(np.uint32)


# ---- programs ----
def one_ratio_program():
    p = Program(N_GLOBALS)
    p.ratio(0, p.get(1, 0, 0), p.get(1, 1, 0))
    return p


def every_ratio_form_program():
    """base / base, base / ext, ext / base, ext / ext; globals, mix components, backs 0 / 1 / 3, code and data taps"""
    p = Program(N_GLOBALS)
    alpha = p.alpha()
    x, xb, xbb = p.get(1, 0, 0), p.get(1, 0, 1), p.get(1, 1, 3)
    c, cb = p.get(0, 2, 0), p.get(0, 0, 3)
    g0, g1 = p.global_(0), p.global_(1)
    p.ratio(0, p.add(x, g0), p.add(p.mul(xbb, cb), g1))                          # base / base
    p.ratio(1, p.mul(xb, p.mix(2)), p.sub(alpha, c))                            # base / ext
    p.ratio(2, p.sub(alpha, xbb), p.add(c, p.get(1, 5, 1)))                     # ext / base
    p.ratio(3, p.mul(p.sub(alpha, x), g1), p.add(alpha, p.const_ext(1, 2, 3, 4)))  # ext / ext
    return p


def all_three_kinds_program():
    """2 SUM, 2 PROD, 2 RATIO"""
    p = Program(N_GLOBALS)
    alpha = p.alpha()
    x, y, c = p.get(1, 0, 0), p.get(1, 1, 1), p.get(0, 1, 0)
    p.sum_(0, p.const(1), p.sub(alpha, x))
    p.sum_(1, y, p.add(x, p.global_(0)))
    p.prod(2, p.sub(alpha, y))
    p.prod(3, p.add(c, x))
    p.ratio(4, p.sub(alpha, x), p.sub(alpha, y))
    p.ratio(5, p.add(x, c), p.add(y, p.global_(1)))
    return p


def ratio_zero_denominator_program():
    """sequence 0: a base denominator (data column 4) - ZERO_VALUE, zero on ONE planted row; sequence 1: an ext denominator
    (alpha times (data column 6 - ZERO_VALUE)), zero on one planted row.  planted_zero_rows says where."""
    p = Program(N_GLOBALS)
    alpha = p.alpha()
    zv = p.const(ZERO_VALUE)
    p.ratio(0, p.get(1, 0, 0), p.sub(p.get(1, 4, 0), zv))
    p.ratio(1, p.sub(alpha, p.get(1, 1, 0)), p.mul(alpha, p.sub(p.get(1, 6, 0), zv)))
    p.zero_cols = (4, 6)
    return p


def planted_zero_rows(n):
    """ratio_zero_denominator: (the row on which data column 4 holds ZERO_VALUE, the row on which data column 6 does)"""
    return n // 2, 3 * n // 4


def plant_zero_rows(prog, data, n):
    """make data columns 4 and 6 hold ZERO_VALUE exactly on their planted row (any other cell that holds it is moved off it)"""
    zero = ref.encode(ZERO_VALUE)
    for col, row in zip(prog.zero_cols, planted_zero_rows(n)):
        data[col][data[col] == zero] = ref.encode(ZERO_VALUE + 1)
        data[col][row] = zero


def permutation_program():
    """(alpha - a) / (alpha - b): a, b = data columns 0, 1; the last row is 1 iff b is a permutation of a (up to the challenge)"""
    p = Program(0)
    alpha = p.alpha()
    p.ratio(0, p.sub(alpha, p.get(1, 0, 0)), p.sub(alpha, p.get(1, 1, 0)))
    return p


PROGRAMS = {
    "one_ratio": one_ratio_program,
    "every_ratio_form": every_ratio_form_program,
    "all_three_kinds": all_three_kinds_program,
    "ratio_zero_denominator": ratio_zero_denominator_program,
    "permutation": permutation_program,
}
# (sequences, sums, ratios) of each: what info() and ratios() must say
COUNTS = {"one_ratio": (1, 0, 1), "every_ratio_form": (4, 0, 4), "all_three_kinds": (6, 2, 2), "ratio_zero_denominator": (2, 0, 2), "permutation": (1, 0, 1)}


def random_program(seed, steps, widths=WIDTHS, n_globals=N_GLOBALS, sums=2, prods=2, ratios=3, backs=(0, 1, 3), window=6, far=0.03):
    """about `steps` steps in the manner of acc_program_ref.random_program, then sums, products and ratios in that order of numbers"""
    rng = np.random.default_rng([seed, steps, 16])
    p = Program(n_globals)

    def leaf():
        k = rng.integers(0, 12)
        if k < 1:
            return p.const(int(rng.integers(0, P)))
        if k < 2:
            return p.const_ext(*[int(v) for v in rng.integers(0, P, 4)])
        if k < 3:
            return p.global_(int(rng.integers(0, n_globals)))
        if k < 5:
            return p.mix(int(rng.integers(0, 4)))
        if k < 8:
            return p.get(0, int(rng.integers(0, widths[0])), int(rng.choice(backs)))
        return p.get(1, int(rng.integers(0, widths[1])), int(rng.choice(backs)))

    def pick():
        if rng.random() < far:
            return int(rng.integers(0, p.n_fp))
        return p.n_fp - 1 - int(rng.integers(0, min(window, p.n_fp)))

    leaf(), leaf()
    while len(p.steps) < steps:
        if rng.random() < 0.3:
            leaf()
        else:
            [p.add, p.sub, p.mul][int(rng.integers(0, 3))](pick(), pick())
    order = []  # the defining steps may come in any order of steps: only the NUMBERS are ordered
    for s in range(sums):
        order.append(("sum", s))
    for s in range(sums, sums + prods):
        order.append(("prod", s))
    for s in range(sums + prods, sums + prods + ratios):
        order.append(("ratio", s))
    for k in rng.permutation(len(order)):
        kind, s = order[int(k)]
        if kind == "sum":
            p.sum_(s, p.const(1 + s), pick())
        elif kind == "prod":
            p.prod(s, pick())
        else:
            p.ratio(s, pick(), pick())
    return p
