"""Definition-level reference for constraint programs (include/bx_program.h, "Values"): plain numpy on canonical integers, no code
shared with the library.

* `Program`: a step list in the header's shape — tuples (op, a, b, c, d) with the header's op numbers, a tap list, n_globals, ret —
  built with the same method names as the library's builder so that a circuit is written once.
* `evaluate`: the interpreter, following the header's table literally: two unbounded var lists, every fp var an element of
  Fp4 = Fp[X]/(X^4 + 11) (a base value is (v, 0, 0, 0)), every mix var a pair (tot, mul) whose mul IS computed.  Values are
  (4, n) arrays: n = 4N domain points for the prover's side, n = 1 for the verifier's point.
* `check_planes`: evaluate over the domain x = w_4N^row and divide by (3x)^N - 1.
* `random_program`: seeded generator; `lookup_program`, `square_program`, `narrow_limit_program`, `wide_limit_program`,
  `both_limits_program`.
"""
import numpy as np

P = 2013265921
U = np.uint64
R_INV = pow(1 << 32, -1, P)
(CONST, CONST_EXT, GET, GET_GLOBAL, ADD, SUB, MUL, TRUE, AND_EQZ, AND_COND) = range(10)  # enum bx_cons_op
MAX_DEGREE, MAX_NARROW, MAX_WIDE = 5, 32, 24  # BX_CONS_MAX_*


def encode(x):
    """canonical integers -> Montgomery words"""
    return ((np.asarray(x, U) % U(P)) << U(32)) % U(P)


def decode(m):
    return (np.asarray(m, U) * U(R_INV)) % U(P)


# ---- Fp4 on (4, n) uint64 arrays of canonical integers ----
def bmul(a, b):
    return (a * b) % U(P)


def e_base(v, n):
    out = np.zeros((4, n), U)
    out[0] = v
    return out


def e_add(a, b):
    return (a + b) % U(P)


def e_sub(a, b):
    return (a + U(P) - b) % U(P)


def e_mul(a, b):
    nb = U(P - 11)
    s = lambda *t: sum(t) % U(P)  # noqa: E731 - each term is already below P
    return np.stack([
        s(bmul(a[0], b[0]), bmul(nb, s(bmul(a[1], b[3]), bmul(a[2], b[2]), bmul(a[3], b[1])))),
        s(bmul(a[0], b[1]), bmul(a[1], b[0]), bmul(nb, s(bmul(a[2], b[3]), bmul(a[3], b[2])))),
        s(bmul(a[0], b[2]), bmul(a[1], b[1]), bmul(a[2], b[0]), bmul(nb, bmul(a[3], b[3]))),
        s(bmul(a[0], b[3]), bmul(a[1], b[2]), bmul(a[2], b[1]), bmul(a[3], b[0]))])


class Program:
    def __init__(self, n_globals=0):
        self.n_globals, self.steps, self.taps, self._tap_index = n_globals, [], [], {}
        self.n_fp = self.n_mix = 0
        self.ret = None

    def _fp(self, *s):
        self.steps.append(tuple(s) + (0,) * (5 - len(s)))
        self.n_fp += 1
        return self.n_fp - 1

    def _mix(self, *s):
        self.steps.append(tuple(s) + (0,) * (5 - len(s)))
        self.n_mix += 1
        return self.n_mix - 1

    def const(self, a):
        return self._fp(CONST, a)

    def const_ext(self, a, b, c, d):
        return self._fp(CONST_EXT, a, b, c, d)

    def tap(self, group, col, back=0):
        key = (group, col, back)
        if key not in self._tap_index:
            self._tap_index[key] = len(self.taps)
            self.taps.append(key)
        return self._tap_index[key]

    def get(self, group, col, back=0):
        return self._fp(GET, self.tap(group, col, back))

    def global_(self, i):
        return self._fp(GET_GLOBAL, 0, i)

    def mix(self, k):
        return self._fp(GET_GLOBAL, 1, k)

    def add(self, a, b):
        return self._fp(ADD, a, b)

    def sub(self, a, b):
        return self._fp(SUB, a, b)

    def mul(self, a, b):
        return self._fp(MUL, a, b)

    def true(self):
        return self._mix(TRUE)

    def and_eqz(self, x, y):
        return self._mix(AND_EQZ, x, y)

    def and_cond(self, x, cond, inner):
        return self._mix(AND_COND, x, cond, inner)

    def done(self, ret=None):
        self.ret = self.n_mix - 1 if ret is None else ret
        return self


def evaluate(prog, tap_value, n, poly_mix, mix, globals_):
    """mix[ret].tot as a (4, n) array.  tap_value(group, col, back) -> (4, n) or (n,) canonical; poly_mix, mix: 4 canonical
    integers; globals_: canonical integers."""
    fp, mx = [], []
    pm = np.array(poly_mix, U).reshape(4, 1) * np.ones((1, n), U)
    for op, a, b, c, d in prog.steps:
        if op == CONST:
            fp.append(e_base(U(a), n))
        elif op == CONST_EXT:
            fp.append(np.array([a, b, c, d], U).reshape(4, 1) * np.ones((1, n), U))
        elif op == GET:
            v = np.asarray(tap_value(*prog.taps[a]), U)
            fp.append(v.copy() if v.ndim == 2 else e_base(v, n))
        elif op == GET_GLOBAL:
            fp.append(e_base(U(int(globals_[b]) if a == 0 else int(mix[b])), n))
        elif op == ADD:
            fp.append(e_add(fp[a], fp[b]))
        elif op == SUB:
            fp.append(e_sub(fp[a], fp[b]))
        elif op == MUL:
            fp.append(e_mul(fp[a], fp[b]))
        elif op == TRUE:
            mx.append((np.zeros((4, n), U), e_base(U(1), n)))
        elif op == AND_EQZ:
            tot, mul = mx[a]
            mx.append((e_add(tot, e_mul(mul, fp[b])), e_mul(mul, pm)))
        elif op == AND_COND:
            tot, mul = mx[a]
            itot, imul = mx[c]
            mx.append((e_add(tot, e_mul(e_mul(fp[b], itot), mul)), e_mul(mul, imul)))
        else:
            raise ValueError(op)
    return mx[prog.ret][0]


def vanishing_inverses(po2):
    """1 / ((3x)^N - 1) on x = w_4N^row takes four values, by row mod 4: (3x)^N = 3^N w_4^(row mod 4), w_4 = 137^(2^25)"""
    t3n, w4 = pow(3, 1 << po2, P), pow(137, 1 << 25, P)
    return np.array([pow((t3n * pow(w4, m, P) - 1) % P, -1, P) for m in range(4)], U)


def check_planes(prog, po2, evals, poly_mix_w, mix_w, globals_w):
    """The four check planes as Montgomery words, (4, 4N).  evals = three (width, 4N) arrays of Montgomery words; poly_mix_w, mix_w,
    globals_w: Montgomery words, as the library's entry point takes them."""
    dom = 4 << po2
    canon = [decode(e) for e in evals]

    def tap_value(group, col, back):
        return np.roll(canon[group][col], 4 * back)  # row - 4 back mod 4N

    tot = evaluate(prog, tap_value, dom, decode(poly_mix_w).tolist(), decode(mix_w).tolist(), decode(np.array(globals_w, U)).tolist() if len(globals_w) else [])
    zi = vanishing_inverses(po2)[np.arange(dom) % 4]
    return encode(bmul(tot, zi[None, :])).astype(np.uint32)


def at_point(prog, tap_words, poly_mix_w, mix_w, globals_w):
    """The verifier's side: tap_words(group, col, back) -> 4 Montgomery words; -> 4 Montgomery words"""
    def tap_value(group, col, back):
        return decode(np.array(tap_words(group, col, back), U)).reshape(4, 1)

    tot = evaluate(prog, tap_value, 1, decode(poly_mix_w).tolist(), decode(mix_w).tolist(), decode(np.array(globals_w, U)).tolist() if len(globals_w) else [])
    return [int(v) for v in encode(tot[:, 0])]


# ---- programs ----
def random_program(seed, steps, widths=(3, 5, 8), backs=(0, 1, 3), n_taps=12, nesting=0, ext_share=0.3, pressure=8, n_globals=2):
    """A seeded random program of about `steps` steps.  taps: n_taps distinct (group, col, back) within `widths`; nesting: depth of the
    AND_COND chains (0 = none); ext_share: how often a leaf is an ext constant (which then spreads through the arithmetic);
    pressure: operands are drawn from the last `pressure` fp vars, which is what bounds the live values (keep it <= 16: both slot
    files hold more).  Degrees are tracked so that nothing exceeds 5.  The result always takes in an ext-valued constraint, so
    that all four planes of the output are populated."""
    rng = np.random.default_rng([seed, steps])
    p = Program(n_globals)
    tap_pool = set()
    while len(tap_pool) < n_taps:
        g = int(rng.integers(0, 3))
        tap_pool.add((g, int(rng.integers(0, widths[g])), int(rng.choice(backs))))
    tap_pool = sorted(tap_pool)
    deg = []  # per fp var

    def leaf():
        k = rng.random()
        if k < ext_share:
            deg.append(0)
            return p.const_ext(*[int(v) for v in rng.integers(0, P, 4)])
        if k < ext_share + 0.1:
            deg.append(0)
            return p.const(int(rng.integers(0, P)))
        if k < ext_share + 0.2:
            deg.append(0)
            return p.global_(int(rng.integers(0, n_globals))) if (n_globals and rng.random() < 0.5) else p.mix(int(rng.integers(0, 4)))
        deg.append(1)
        return p.get(*tap_pool[int(rng.integers(0, len(tap_pool)))])

    def recent():
        return int(rng.integers(max(0, p.n_fp - pressure), p.n_fp))

    def arith():
        a, b = recent(), recent()
        op = int(rng.integers(0, 3))
        if op == 2 and deg[a] + deg[b] <= MAX_DEGREE:
            deg.append(deg[a] + deg[b])
            return p.mul(a, b)
        deg.append(max(deg[a], deg[b]))
        return p.add(a, b) if op == 0 else p.sub(a, b)

    def chain(depth):
        """a mix var: AND_EQZ links, and AND_COND links down to `depth`; -> (mix var, its degree)"""
        m, mdeg = p.true(), 0
        for _ in range(int(rng.integers(1, 4))):
            for _ in range(int(rng.integers(1, 5))):
                leaf() if rng.random() < 0.4 else arith()
            y = recent()
            if depth > 0 and rng.random() < 0.6:
                inner, ideg = chain(depth - 1)
                cond = next((v for v in range(p.n_fp - 1, max(-1, p.n_fp - 1 - pressure), -1) if deg[v] + ideg <= MAX_DEGREE), None)
                if cond is None:
                    deg.append(0)
                    cond = p.const(int(rng.integers(1, P)))
                m, mdeg = p.and_cond(m, cond, inner), max(mdeg, deg[cond] + ideg)
            else:
                m, mdeg = p.and_eqz(m, y), max(mdeg, deg[y])
        return m, mdeg

    for _ in range(3):
        leaf()
    top = p.true()
    while len(p.steps) < steps:
        for _ in range(int(rng.integers(1, 6))):
            leaf() if rng.random() < 0.35 else arith()
        if nesting and rng.random() < 0.3:
            inner, ideg = chain(nesting - 1)
            cond = next((v for v in range(p.n_fp - 1, max(-1, p.n_fp - 1 - pressure), -1) if deg[v] + ideg <= MAX_DEGREE), None)
            if cond is None:
                deg.append(0)
                cond = p.const(int(rng.integers(1, P)))
            top = p.and_cond(top, cond, inner)
        else:
            top = p.and_eqz(top, recent())
    # the closing constraint: ext constant * tap + tap (ext x base, ext + base), so the result is ext-valued whatever came before
    e = p.const_ext(*[int(v) for v in rng.integers(1, P, 4)])
    t = p.get(*tap_pool[0])
    top = p.and_eqz(top, p.add(p.mul(e, t), p.get(*tap_pool[-1])))
    return p.done(top)


def one_constraint_program():
    p = Program(0)
    e = p.const_ext(5, 6, 7, 8)
    return p.done(p.and_eqz(p.true(), p.add(p.mul(p.get(1, 0, 0), e), p.get(2, 7, 3))))


def every_form_program():
    """every arithmetic step in its base x base, ext x base, base x ext and ext x ext form, both types of y and of cond, and AND_COND
    three deep; degree 5 exactly"""
    p = Program(2)
    b0, b1, b2 = p.get(0, 0, 0), p.get(1, 4, 1), p.get(2, 7, 3)
    e0, e1 = p.const_ext(1, 2, 3, 4), p.const_ext(P - 1, 0, 5, P - 2)
    g, a = p.global_(1), p.mix(2)
    bb = [p.add(b0, b1), p.sub(b1, b2), p.mul(b0, b2)]
    eb = [p.add(e0, b0), p.sub(e0, b1), p.mul(e1, b2)]
    be = [p.add(b0, e1), p.sub(b1, e0), p.mul(b2, e0)]
    ee = [p.add(eb[0], be[0]), p.sub(eb[1], be[1]), p.mul(eb[2], be[2])]
    top = p.true()
    for v in bb + eb + be + ee + [p.add(g, a), p.mul(p.mul(bb[2], bb[2]), b1)]:  # the last has degree 5
        top = p.and_eqz(top, v)
    # three deep: innermost two constraints (base y, ext y), wrapped by a base cond, an ext cond, a base cond
    m3 = p.and_eqz(p.and_eqz(p.true(), bb[0]), eb[0])
    m2 = p.and_eqz(p.and_cond(p.and_eqz(p.true(), b2), b0, m3), ee[0])
    m1 = p.and_cond(p.and_eqz(p.true(), be[1]), eb[1], m2)
    top = p.and_cond(top, b1, m1)
    top = p.and_eqz(top, ee[2])
    return p.done(top)


def narrow_limit_program(extra=0):
    """needs exactly MAX_NARROW (+ extra) live base values: that many taps are fetched before the first is used"""
    p = Program(0)
    n = MAX_NARROW + extra
    vals = [p.get(k % 3, (k // 3) % 3, k // 9) for k in range(n)]
    e = p.const_ext(3, 1, 4, 1)
    s = vals[0]
    for v in vals[1:]:
        s = p.add(s, v)
    return p.done(p.and_eqz(p.true(), p.mul(e, s)))


def wide_limit_program(extra=0):
    """needs exactly MAX_WIDE (+ extra) live wide values: the result's tot, one ext constant and MAX_WIDE - 2 ext products"""
    p = Program(0)
    top = p.true()
    e = p.const_ext(2, 7, 1, 8)
    vals = [p.mul(p.get(k % 3, (k // 3) % 3, k // 9), e) for k in range(MAX_WIDE - 2 + extra)]
    s = e
    for v in vals:
        s = p.add(s, v)
    return p.done(p.and_eqz(top, s))


def both_limits_program():
    """needs exactly MAX_NARROW live base values and then exactly MAX_WIDE live wide values: the two phases of the programs above in
    one program, so that both slot files, and with them the kernel's LDS, are at their ceiling together"""
    p = Program(0)
    top = p.true()
    e = p.const_ext(2, 7, 1, 8)
    base = [p.get(k % 3, (k // 3) % 3, k // 9) for k in range(MAX_NARROW)]
    s = base[0]
    for v in base[1:]:
        s = p.add(s, v)
    top = p.and_eqz(top, p.mul(e, s))
    vals = [p.mul(p.get(k % 3, (k // 3) % 3, k // 9), e) for k in range(MAX_WIDE - 2)]
    s = e
    for v in vals:
        s = p.add(s, v)
    return p.done(p.and_eqz(top, s))


def square_program():
    """tests/test_circuit_plugin_gpu.py's circuit: data[1] = data[0]^2 + code[0] * data[0](r-1) + data[0](r-3), and
    first * (data[0] - g) with first = code[1]"""
    p = Program(1)
    d0, d0b, d0b3, d1 = p.get(1, 0, 0), p.get(1, 0, 1), p.get(1, 0, 3), p.get(1, 1, 0)
    c0, first, g = p.get(0, 0, 0), p.get(0, 1, 0), p.global_(0)
    c = p.sub(p.sub(p.sub(d1, p.mul(d0, d0)), p.mul(c0, d0b)), d0b3)
    top = p.and_eqz(p.true(), c)
    return p.done(p.and_eqz(top, p.mul(first, p.sub(d0, g))))


def lookup_program(po2, widths):
    """The lookup circuit's constraints from the text of include/bx_lookup.h ("constraints, in mixing order"), for a shape."""
    wc, wd, wa = widths
    V = min((wd - 1) // 3, (wa // 4 - 1) // 2)
    B = 1 << min(15, po2 - 1)
    p = Program(2)
    xk = [None] + [p.const_ext(*[1 if i == k else 0 for i in range(4)]) for k in (1, 2, 3)]  # X, X^2, X^3

    def ext_of(words):  # sum_k X^k * words[k]
        r = words[0]
        for k in (1, 2, 3):
            r = p.add(r, p.mul(xk[k], words[k]))
        return r

    alpha = ext_of([p.mix(k) for k in range(4)])
    first, last, table = p.get(0, 0), p.get(0, 1), p.get(0, 2)
    not_first = p.sub(p.const(1), first)
    bconst = p.const(B)
    top = p.true()
    # 1. v_j - lo_j - B hi_j
    for j in range(V):
        top = p.and_eqz(top, p.sub(p.sub(p.get(1, 3 * j), p.get(1, 3 * j + 1)), p.mul(bconst, p.get(1, 3 * j + 2))))
    # 2., 3. the running sums; 4. needs their total
    total = None
    one = p.const(1)
    for s in range(2 * V + 1):
        cur = ext_of([p.get(2, 4 * s + k, 0) for k in range(4)])
        back = ext_of([p.get(2, 4 * s + k, 1) for k in range(4)])
        step = p.sub(cur, p.mul(not_first, back))
        total = cur if total is None else p.add(total, cur)
        if s < 2 * V:
            a_s = p.get(1, 3 * (s // 2) + 1 + s % 2)
            top = p.and_eqz(top, p.sub(p.mul(step, p.sub(alpha, a_s)), one))
        else:
            top = p.and_eqz(top, p.add(p.mul(step, p.sub(alpha, table)), p.get(1, 3 * V)))
    top = p.and_eqz(top, p.mul(last, total))
    v0 = p.get(1, 0)
    top = p.and_eqz(top, p.mul(first, p.sub(v0, p.global_(0))))
    top = p.and_eqz(top, p.mul(last, p.sub(v0, p.global_(1))))
    return p.done(top)
