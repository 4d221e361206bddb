"""Definition-level reference of witness programs (include/bx_program.h, "Witness programs"), written from that text and sharing no
code with the library: numpy, following the header's table literally.  Every fp var is a whole column of N words of its own (no slot
file, no forwarding: after a SET the column is in the data matrix and a GET with back 0 reads it from there), a tap `back` rows back
is the column rolled by `back` (cyclic).  Words are Montgomery words, canonical in [0, P).

Also here: a seeded random-program generator that respects the three derived-column rules (a derived column is read only with back
0 and only after its SET; a column is SET once), the named programs the tests run, and the synthetic circuit's derive stage written
as a witness program from the formulas of include/bx_prover.h ("The synthetic circuit").
"""
import numpy as np

P = 2013265921
U = np.uint64
R = (1 << 32) % P
R_INV = pow(1 << 32, -1, P)
_P, _RINV = U(P), U(R_INV)

(OP_CONST, OP_CONST_EXT, OP_GET, OP_GET_GLOBAL, OP_ADD, OP_SUB, OP_MUL, OP_TRUE, OP_AND_EQZ, OP_AND_COND, OP_SET) = range(11)  # enum bx_cons_op
MAX_NARROW = 32  # BX_CONS_MAX_NARROW


def encode(x):
    return int(x) % P * R % P


class Program:
    """steps: (op, a, b); taps: (group, col, back); cells: (global index, data column, row)"""

    def __init__(self):
        self.steps, self.taps, self.cells, self._tap_index = [], [], [], {}
        self.n_fp = 0

    def _fp(self, op, a=0, b=0):
        self.steps.append((op, int(a), int(b)))
        self.n_fp += 1
        return self.n_fp - 1

    def const(self, a):
        return self._fp(OP_CONST, a)

    def tap(self, group, col, back=0):
        key = (int(group), int(col), int(back))
        if key not in self._tap_index:
            self._tap_index[key] = len(self.taps)
            self.taps.append(key)
        return self._tap_index[key]

    def get(self, group, col, back=0):
        return self._fp(OP_GET, self.tap(group, col, back))

    def add(self, a, b):
        return self._fp(OP_ADD, a, b)

    def sub(self, a, b):
        return self._fp(OP_SUB, a, b)

    def mul(self, a, b):
        return self._fp(OP_MUL, a, b)

    def set(self, col, var):
        self.steps.append((OP_SET, int(col), int(var)))

    def global_cell(self, index, col, row):
        self.cells.append((int(index), int(col), int(row)))

    def derived(self):
        return [s[1] for s in self.steps if s[0] == OP_SET]


def evaluate(prog, po2, code, data):
    """-> the data matrix (w_data, N) after the program has run on `code` (w_code, N) and `data`; the inputs are left unchanged"""
    n = 1 << po2
    groups = [np.asarray(code, np.uint32).reshape(-1, n), np.array(data, np.uint32).reshape(-1, n)]
    fp = []
    for op, a, b in prog.steps:
        if op == OP_CONST:
            fp.append(np.full(n, encode(a), U))
        elif op == OP_GET:
            group, col, back = prog.taps[a]
            fp.append(np.roll(groups[group][col], back).astype(U))  # row r reads row (r - back) mod N
        elif op == OP_ADD:
            fp.append((fp[a] + fp[b]) % _P)
        elif op == OP_SUB:
            fp.append((fp[a] + _P - fp[b]) % _P)
        elif op == OP_MUL:
            fp.append(fp[a] * fp[b] % _P * _RINV % _P)
        elif op == OP_SET:
            groups[1][a] = fp[b].astype(np.uint32)
        else:
            raise ValueError(f"op {op} does not belong in a witness program")
    return groups[1]


def globals_of(prog, data):
    return {g: int(data[col][row]) for g, col, row in prog.cells}


# ---- programs ----
def random_program(seed, steps, widths=(3, 8), derived=(3, 5, 6, 7), backs=(0, 1, 3), window=6, far=0.05):
    """about `steps` steps over code width widths[0] and data width widths[1]; the columns of `derived` are SET in that order at even
    distances, every other data column is free.  Operands come from the last `window` vars (few live values) and now and then from anywhere."""
    rng = np.random.default_rng([seed, steps])
    p = Program()
    free = [c for c in range(widths[1]) if c not in derived]
    done = []  # derived columns already SET
    set_every = max(steps // len(derived), 3)

    def leaf():
        k = rng.integers(0, 10)
        if k < 1:
            return p.const(int(rng.integers(0, P)))
        if k < 4:
            return p.get(0, int(rng.integers(0, widths[0])), int(rng.choice(backs)))
        if k < 6 and done:
            return p.get(1, int(rng.choice(done)), 0)  # forwarded: derived, back 0, after its SET
        return p.get(1, int(rng.choice(free)), int(rng.choice(backs)))

    def pick():
        if rng.random() < far:
            return int(rng.integers(0, p.n_fp))
        return p.n_fp - 1 - int(rng.integers(0, min(window, p.n_fp)))

    leaf(), leaf()
    while len(done) < len(derived):
        for _ in range(set_every - 1):
            if rng.random() < 0.3:
                leaf()
            else:
                [p.add, p.sub, p.mul][int(rng.integers(0, 3))](pick(), pick())
        col = derived[len(done)]
        p.set(col, p.n_fp - 1)
        done.append(col)
    return p


def one_set_program():
    p = Program()
    p.set(3, p.mul(p.get(1, 0, 0), p.get(0, 1, 1)))
    return p


def every_form_program():
    """every step kind and operand shape: a constant, code and data taps at backs 0, 1 and 3, both operands the same var, a SET of a
    var that lives on, a var SET into two columns, and a forwarded value used three columns later"""
    p = Program()
    x, xb, xbb = p.get(1, 0, 0), p.get(1, 0, 1), p.get(1, 1, 3)
    c, k = p.get(0, 2, 1), p.const(P - 1)
    v3 = p.add(p.mul(x, x), p.mul(c, xb))
    p.set(3, v3)
    v5 = p.sub(p.add(v3, xbb), p.mul(k, x))  # v3 lives on after its SET
    p.set(5, v5)
    p.set(6, p.sub(xb, p.get(0, 0, 3)))
    f3 = p.get(1, 3, 0)  # forwarded, three SETs after column 3's
    p.set(7, p.add(p.mul(f3, f3), p.get(1, 5, 0)))
    p.set(2, f3)  # the forwarded value stored once more
    p.global_cell(0, 7, 1)
    return p


def narrow_limit_program(extra=0):
    """MAX_NARROW + extra values live at once: that many loads, then a sum that names each of them"""
    p = Program()
    live = [p.get(1, k % 3, k % 4) if k % 5 else p.const(k + 1) for k in range(MAX_NARROW + extra)]
    acc = live[0]
    for v in live[1:]:
        acc = p.add(p.mul(acc, v), v)
    p.set(7, acc)
    return p


PROGRAMS = {
    "one_set": one_set_program,
    "steps_40": lambda: random_program(40, 40),
    "steps_700": lambda: random_program(700, 700),
    "every_form": every_form_program,
    "narrow_limit": narrow_limit_program,  # 32 slots: the whole 32 KiB of LDS
}
WIDTHS = (3, 8)


# ---- the synthetic circuit's derive stage (include/bx_prover.h, "The synthetic circuit") ----
def synthetic_derive_program(w_code, w_data, T, G):
    """data[F+j][r] = sum_{t<T} prod_{f<G} pool_j[idx(t,f)] for j < J = w_data - F, F = ceil(w_data / 2), with the 16-entry pool
        [ u = data[j][r],  ub = data[j][r-1] if j % 8 == 0, data[j][r-2] if j % 8 == 4, else u,  data[(j+1) mod F][r],  data[(j+2) mod F][r],
          p_1 .. p_8 with p_s = data[F+j-s][r] (csel(s-j-1)[r] when j < s),  csel(j)[r] .. csel(j+3)[r] ]
    csel(i) = code column 2 + i mod (w_code - 2) when w_code >= 3, else the constant 1; idx(t,f) = (7t + 3f + floor(t/4) f + floor(t/16)) mod 16."""
    F = (w_data + 1) // 2
    p = Program()
    for j in range(w_data - F):
        got = {}

        def cell(group, col, back=0):
            if (group, col, back) not in got:
                got[group, col, back] = p.const(1) if group is None else p.get(group, col, back)
            return got[group, col, back]

        def csel(i):
            return cell(0, 2 + i % (w_code - 2)) if w_code >= 3 else cell(None, 0)

        pool = [cell(1, j), cell(1, j, 1 if j % 8 == 0 else 2 if j % 8 == 4 else 0), cell(1, (j + 1) % F), cell(1, (j + 2) % F)]
        pool += [cell(1, F + j - s) if j >= s else csel(s - j - 1) for s in range(1, 9)]
        pool += [csel(j + q) for q in range(4)]
        total = None
        for t in range(T):
            prod = pool[(7 * t + t // 16) % 16]
            for f in range(1, G):
                prod = p.mul(prod, pool[(7 * t + 3 * f + (t // 4) * f + t // 16) % 16])
            total = prod if total is None else p.add(total, prod)
        p.set(F + j, total)
    return p
