"""Definition-level reference of accumulate programs (include/bx_program.h, "Accumulate programs"), written from that text and sharing
no code with the library: numpy and Python integers, following the header's table literally.  Every fp var is a whole column of its
own — (N,) for a base var, (N, 4) for an ext var — of PLAIN field values (Montgomery words are decoded on the way in and encoded on
the way out, so nothing here knows the library's arithmetic).  A tap `back` rows back is the column rolled by `back` (cyclic).  The
Fp4 inverse is a^(P^4 - 2) by square and multiply, which sends 0 to 0 (the HAL's rule); running sums and products are plain loops.

Also here: a seeded random-program generator that respects the rules (m of a SUM is base, sequences 0 .. S-1 each once, sums before
products), the named programs the tests run, and the lookup circuit's accumulate stage written as an accumulate program from the
text of include/bx_lookup.h ("accum").
"""
import numpy as np

P = 2013265921
U = np.uint64
R = (1 << 32) % P
R_INV = pow(1 << 32, -1, P)
_P = U(P)
BETA = 11  # Fp4 = Fp[X] / (X^4 + 11)

(OP_CONST, OP_CONST_EXT, OP_GET, OP_GET_GLOBAL, OP_ADD, OP_SUB, OP_MUL, OP_TRUE, OP_AND_EQZ, OP_AND_COND, OP_SET, OP_SUM, OP_PROD) = range(13)  # enum bx_cons_op
MAX_NARROW, MAX_WIDE, MAX_SEQS = 32, 24, 1024  # BX_CONS_MAX_NARROW, BX_CONS_MAX_WIDE, BX_ACC_MAX_SEQS


def encode(x):
    return int(x) % P * R % P


def decode(words):
    return np.asarray(words, U) * U(R_INV) % _P


class Program:
    """steps: (op, a, b, c, d); taps: (group, col, back); ext[v]: is fp var v ext-typed"""

    def __init__(self, n_globals=0):
        self.n_globals = n_globals
        self.steps, self.taps, self._tap_index, self.ext = [], [], {}, []
        self.planted = None  # (data column, plain value): rows on which that column is made to hold the value (zero_denominator)

    @property
    def n_fp(self):
        return len(self.ext)

    def _fp(self, ext, op, a=0, b=0, c=0, d=0):
        self.steps.append((op, int(a), int(b), int(c), int(d)))
        self.ext.append(bool(ext))
        return len(self.ext) - 1

    def const(self, a):
        return self._fp(False, OP_CONST, a)

    def const_ext(self, a, b, c, d):
        return self._fp(True, OP_CONST_EXT, a, b, c, d)

    def tap(self, group, col, back=0):
        key = (int(group), int(col), int(back))
        if key not in self._tap_index:
            self._tap_index[key] = len(self.taps)
            self.taps.append(key)
        return self._tap_index[key]

    def get(self, group, col, back=0):
        return self._fp(False, OP_GET, self.tap(group, col, back))

    def global_(self, index):
        return self._fp(False, OP_GET_GLOBAL, 0, index)

    def mix(self, component):
        return self._fp(False, OP_GET_GLOBAL, 1, component)

    def add(self, a, b):
        return self._fp(self.ext[a] or self.ext[b], OP_ADD, a, b)

    def sub(self, a, b):
        return self._fp(self.ext[a] or self.ext[b], OP_SUB, a, b)

    def mul(self, a, b):
        return self._fp(self.ext[a] or self.ext[b], OP_MUL, a, b)

    def sum_(self, s, m, d):
        self.steps.append((OP_SUM, int(s), int(m), int(d), 0))

    def prod(self, s, a):
        self.steps.append((OP_PROD, int(s), int(a), 0, 0))

    def sequences(self):
        """{s: is it a sum}"""
        return {st[1]: st[0] == OP_SUM for st in self.steps if st[0] in (OP_SUM, OP_PROD)}

    def kept(self):
        """the distinct (group, col) of the tap list in order of first appearance"""
        out = []
        for g, c, _ in self.taps:
            if (g, c) not in out:
                out.append((g, c))
        return out

    def alpha(self):
        """the ext challenge rebuilt from the four base components of `mix`: sum_k X^k mix_k"""
        a = self.mix(0)
        for k in range(1, 4):
            a = self.add(a, self.mul(self.const_ext(*[1 if q == k else 0 for q in range(4)]), self.mix(k)))
        return a


# ---- plain Fp4 over numpy columns (N, 4) ----
def _lift(v):
    if v.ndim == 2:
        return v
    out = np.zeros((v.shape[0], 4), U)
    out[:, 0] = v
    return out


def f4_mul(a, b):
    """(N, 4) x (N, 4): schoolbook, X^4 = -11"""
    out = np.zeros_like(a)
    for i in range(4):
        for j in range(4):
            t = a[:, i] * b[:, j] % _P
            if i + j >= 4:
                out[:, i + j - 4] = (out[:, i + j - 4] + _P - t * U(BETA) % _P) % _P
            else:
                out[:, i + j] = (out[:, i + j] + t) % _P
    return out


def f4_inv(a):
    """a^(P^4 - 2), row by row at once; 0 -> 0"""
    e = P ** 4 - 2
    result = np.zeros_like(a)
    result[:, 0] = 1
    base = a.copy()
    while e:
        if e & 1:
            result = f4_mul(result, base)
        base = f4_mul(base, base)
        e >>= 1
    return result


def _mul_int(a, b):
    out = [0, 0, 0, 0]
    for i in range(4):
        for j in range(4):
            t = a[i] * b[j]
            if i + j >= 4:
                out[i + j - 4] -= BETA * t
            else:
                out[i + j] += t
    return [v % P for v in out]


def evaluate(prog, po2, code, data, globals_, mix):
    """-> (4 S, N) uint32 Montgomery words: accum columns [0, 4 S) for `code` (w_code, N), `data` (w_data, N), the public words and
    the four words of `mix`"""
    n = 1 << po2
    groups = [decode(np.asarray(code, np.uint32).reshape(-1, n)), decode(np.asarray(data, np.uint32).reshape(-1, n))]
    g, mx = decode(list(globals_) + [0]), decode(mix)
    fp, terms = [], {}
    for op, a, b, c, d in prog.steps:
        if op == OP_CONST:
            fp.append(np.full(n, a, U))
        elif op == OP_CONST_EXT:
            fp.append(np.tile(np.array([a, b, c, d], U), (n, 1)))
        elif op == OP_GET:
            group, col, back = prog.taps[a]
            fp.append(np.roll(groups[group][col], back))  # row r reads row (r - back) mod N
        elif op == OP_GET_GLOBAL:
            fp.append(np.full(n, g[b] if a == 0 else mx[b], U))
        elif op in (OP_ADD, OP_SUB, OP_MUL):
            x, y = fp[a], fp[b]
            if x.ndim != y.ndim:
                x, y = _lift(x), _lift(y)
            if op == OP_ADD:
                fp.append((x + y) % _P)
            elif op == OP_SUB:
                fp.append((x + _P - y) % _P)
            else:
                fp.append(f4_mul(x, y) if x.ndim == 2 else x * y % _P)
        elif op == OP_SUM:
            assert fp[b].ndim == 1, "m of a SUM is a base value"
            assert a not in terms
            terms[a] = (True, f4_mul(_lift(fp[b]), f4_inv(_lift(fp[c]))))
        elif op == OP_PROD:
            assert a not in terms
            terms[a] = (False, _lift(fp[b]))
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
            acc = [(x + y) % P for x, y in zip(acc, rows[r])] if is_sum else _mul_int(acc, rows[r])
            for k in range(4):
                out[4 * s + k][r] = acc[k]
    return (out * U(R) % _P).astype(np.uint32)


# ---- programs ----
WIDTHS = (3, 8)  # code and data columns the named programs tap within
N_GLOBALS = 2
ZERO_VALUE = 5  # zero_denominator: a_r - ZERO_VALUE is zero on the planted rows


def planted_rows(n):
    """rows on which zero_denominator's column holds ZERO_VALUE: the first two, the last, and every fifth from row 2"""
    return sorted({0, 1, n - 1} | set(range(2, n, 5)))


def random_program(seed, steps, widths=WIDTHS, n_globals=N_GLOBALS, sums=3, prods=2, backs=(0, 1, 3), window=6, far=0.03):
    """about `steps` steps; operands come from the last `window` vars (few live values) and now and then from anywhere"""
    rng = np.random.default_rng([seed, steps])
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
    for s in range(sums):
        m = p.get(1, int(rng.integers(0, widths[1])), int(rng.choice(backs))) if s % 2 else p.const(1 + s)
        p.sum_(s, m, pick())
    for s in range(sums, sums + prods):
        p.prod(s, pick())
    return p


def one_sum_program():
    p = Program(N_GLOBALS)
    p.sum_(0, p.const(1), p.get(1, 0, 0))
    return p


def one_prod_program():
    p = Program(N_GLOBALS)
    p.prod(0, p.get(1, 0, 0))
    return p


def every_form_program():
    """base and ext denominators, base and ext factors, globals, mix components, backs 0 / 1 / 3, code and data taps, an ext var used
    twice, a base var used by two sequences"""
    p = Program(N_GLOBALS)
    alpha = p.alpha()
    x, xb, xbb = p.get(1, 0, 0), p.get(1, 0, 1), p.get(1, 1, 3)
    c, cb = p.get(0, 2, 0), p.get(0, 0, 3)
    g0, g1 = p.global_(0), p.global_(1)
    p.sum_(0, p.const(1), p.sub(alpha, x))                                   # 1 / (alpha - a): ext denominator
    p.sum_(1, p.sub(p.const(0), xb), p.sub(alpha, c))                        # -m / (alpha - t)
    p.sum_(2, p.mul(x, g0), p.add(p.mul(xbb, cb), g1))                       # base denominator
    p.sum_(3, xb, p.mul(p.sub(alpha, xbb), p.sub(p.get(1, 5, 1), alpha)))    # ext x ext, base - ext
    p.prod(4, p.sub(alpha, x))                                               # ext factor
    p.prod(5, p.add(x, p.mul(c, p.mix(2))))                                  # base factor
    p.prod(6, p.mul(p.add(alpha, p.const_ext(1, 2, 3, 4)), g1))              # ext + ext, ext x base
    return p


def narrow_limit_program(extra=0):
    """MAX_NARROW + extra base values live at once: that many loads, then a chain that names each of them"""
    p = Program(N_GLOBALS)
    live = [p.get(1, k % 3, k % 4) if k % 5 else p.const(k + 1) for k in range(MAX_NARROW + extra)]
    acc = live[0]
    for v in live[1:]:
        acc = p.add(p.mul(acc, v), v)
    p.sum_(0, p.const(1), acc)
    p.prod(1, acc)
    return p


def wide_limit_program(extra=0):
    """MAX_WIDE + extra ext values live at once"""
    p = Program(N_GLOBALS)
    alpha = p.alpha()  # its temporaries die before the loads below
    live = [alpha] + [p.add(p.const_ext(k + 1, k + 2, 0, 1), p.get(1, k % 3, k % 4)) for k in range(MAX_WIDE + extra - 1)]
    acc = live[0]
    for v in live[1:]:
        acc = p.add(p.mul(acc, v), v)
    p.sum_(0, p.get(0, 1, 0), acc)
    p.prod(1, acc)
    return p


def zero_denominator_program():
    """a base denominator a_r - ZERO_VALUE that is zero on planted_rows, and an ext one that is zero on the same rows: those terms
    contribute zero"""
    p = Program(N_GLOBALS)
    d = p.sub(p.get(1, 4, 0), p.const(ZERO_VALUE))
    p.sum_(0, p.get(1, 2, 0), d)
    p.sum_(1, p.const(1), p.mul(d, p.alpha()))  # an ext denominator that is zero on the same rows
    p.prod(2, p.add(d, p.get(1, 4, 1)))
    p.planted = (4, ZERO_VALUE)
    return p


PROGRAMS = {
    "one_sum": one_sum_program,
    "one_prod": one_prod_program,
    "every_form": every_form_program,
    "narrow_limit": narrow_limit_program,
    "wide_limit": wide_limit_program,
    "zero_denominator": zero_denominator_program,
    "steps_700": lambda: random_program(700, 700),
}


# ---- the lookup circuit's accumulate stage (include/bx_lookup.h, "accum") ----
def lookup_program(V):
    """S = 2V + 1 running sums: s < 2V the limb column a_s = data column 3 (s // 2) + 1 + s % 2, denominator alpha - a_s(r),
    multiplicity 1; s = 2V the table t = code column 2, denominator alpha - t(r), multiplicity -m(r) with m = data column 3V"""
    p = Program(2)
    alpha, one = p.alpha(), p.const(1)
    for s in range(2 * V):
        p.sum_(s, one, p.sub(alpha, p.get(1, 3 * (s // 2) + 1 + s % 2, 0)))
    p.sum_(2 * V, p.sub(p.const(0), p.get(1, 3 * V, 0)), p.sub(alpha, p.get(0, 2, 0)))
    return p
