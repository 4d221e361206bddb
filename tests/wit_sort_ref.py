"""Definition-level reference of a witness program's sorted columns (include/bx_program.h, "sorted columns"), written from that text
and sharing no code with the library: the per-row part is tests/wit_program_ref.py's, a sort decodes its key columns with Python
integers, masks them, applies a stable argsort key by key from the least significant key to the most significant one, and gathers;
the counts of tests/wit_count_ref.py run after the sorts.  Words are Montgomery words, canonical in [0, P).

Also here: the named sort programs the tests run, the helper that hands a program to the library's builder, and key columns."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wit_count_ref as cref  # noqa: E402
import wit_program_ref as ref  # noqa: E402

P, U = ref.P, np.uint64
encode, encode_words = ref.encode, cref.encode_words
POISON = P - 1
MAX_SORTS, MAX_COLS, MAX_KEYS, MAX_BITS = 8, 16, 4, 64  # BX_WIT_MAX_SORTS, _SORT_COLS, _SORT_KEYS, _SORT_BITS
WIDTHS = ref.WIDTHS


def decode_ints(words):
    """Montgomery words -> the integers they stand for, with Python integers (no fixed-width arithmetic)"""
    return [int(w) * ref.R_INV % P for w in np.asarray(words).reshape(-1).tolist()]


class Program(cref.Program):
    """a witness program with a count list and a sort list: sorts = [(keys [(col, bits)], payload [col], dests [col], rows)]"""

    def __init__(self):
        super().__init__()
        self.sorts = []

    def sort(self, keys, payload=(), dests=(), rows=0):
        self.sorts.append(([(int(c), int(b)) for c, b in keys], [int(c) for c in payload], [int(c) for c in dests], int(rows)))

    def dest_cols(self):
        return [c for s in self.sorts for c in s[2]]

    def written(self):
        """every column the run writes: SET columns, dests and count columns"""
        return self.derived() + self.dest_cols() + self.count_cols()


def permutation(keys, rows, data):
    """pi of one sort: the stable sort of rows [0, rows) by the masked key tuple, ties by ascending row"""
    pi = np.arange(rows)
    for col, bits in reversed(keys):  # least significant key first; every step is stable, so earlier steps break the ties
        k = np.array([v & ((1 << bits) - 1) for v in decode_ints(data[col, :rows])], np.int64)
        pi = pi[np.argsort(k[pi], kind="stable")]
    return pi


def evaluate(prog, po2, code, data):
    """-> the data matrix (w_data, N) after the per-row program, then the sorts, then the counts; the inputs are left unchanged"""
    n = 1 << po2
    out = ref.evaluate(prog, po2, code, data)
    for keys, payload, dests, rows in getattr(prog, "sorts", []):
        rows = rows or n
        pi = permutation(keys, rows, out)
        gathered = [out[c, :rows][pi].copy() for c in [c for c, _ in keys] + payload]
        for d, g in zip(dests, gathered):
            out[d, :rows] = g
    tail = cref.Program()  # the counts alone, over what the sorts left
    tail.counts = list(getattr(prog, "counts", []))
    return cref.evaluate(tail, po2, code, out)


def to_builder(prog):
    b = cref.to_builder(prog)
    for keys, payload, dests, rows in getattr(prog, "sorts", []):
        b.sort(keys, payload, dests, rows)
    return b


def compile_ref(prog):
    return to_builder(prog).compile()


# ---- key columns ----
KEY_PATTERNS = ("equal", "ascending", "descending", "mod3", "random")


def key_column(kind, n, seed=0):
    """N Montgomery words: "equal" every cell 5, "ascending" r, "descending" N - 1 - r, "mod3" r mod 3, "random" uniform over the full 31 bits
    (values below P)"""
    r = np.arange(n, dtype=U)
    if kind == "equal":
        v = np.full(n, 5, U)
    elif kind == "ascending":
        v = r
    elif kind == "descending":
        v = U(n - 1) - r
    elif kind == "mod3":
        v = r % U(3)
    elif kind == "random":
        v = np.random.default_rng([seed, n]).integers(0, P, n).astype(U)
    else:
        raise ValueError(kind)
    return encode_words(v)


def random_columns(shape, seed=0):
    return np.random.default_rng([seed, *shape]).integers(0, P, shape, dtype=np.uint32)


# ---- programs ----
def sort_program(bits, n_payload, rows=0):
    """one sort over data width 2 (k + n_payload): keys are columns 0 .. k-1, payload the next n_payload, dests the second half"""
    k = len(bits)
    w = k + n_payload
    p = Program()
    p.sort([(c, b) for c, b in enumerate(bits)], list(range(k, w)), list(range(w, 2 * w)), rows)
    return p, 2 * w


# over WIDTHS = (3, 8): free data columns 0, 1, 2, 4
def set_key_program(rows=0):
    """column 3 = column 0 * code column 1 one row back (SET) is the key; columns 1 and 2 ride along; dests 5, 6, 7"""
    p = Program()
    p.set(3, p.mul(p.get(1, 0, 0), p.get(0, 1, 1)))
    p.sort([(3, 31)], [1, 2], [5, 6, 7], rows)
    p.global_cell(0, 5, 0)
    return p


def sorted_count_program(bins, rows=0):
    """a dest as a count's source: column 5 = column 0 sorted by its low 8 bits, counted into column 6 together with the free column 1"""
    p = Program()
    p.sort([(0, 8)], [], [5], rows)
    p.count(6, [5, 1], bins, rows)
    return p


def two_sorts_program(rows_a=0, rows_b=0):
    """two sorts in one program over overlapping sources, after a per-row part that SETs column 4: columns (0, 1) by the low 13 bits of 0
    -> (5, 6); columns (1, 2) by (9 bits of 1, 4 bits of 2) -> (7, 3)"""
    p = Program()
    p.set(4, p.mul(p.get(1, 0, 1), p.get(0, 1, 0)))
    p.sort([(0, 13)], [1], [5, 6], rows_a)
    p.sort([(1, 9), (2, 4)], [], [7, 3], rows_b)
    return p


# ---- a sorted range check: every value of a = data column 0 lies in [0, B) ----
RC_B, RC_BITS, RC_WIDTHS, RC_TAIL = 200, 8, (2, 4, 4), 8  # bits = ceil(log2 B); the last RC_TAIL rows are the base's own


def range_programs(po2, rows=None, dests=(2, 3)):
    """code: first, last.  data: a, a tag p (free), b, q = (a, p) sorted by a (dests).  accum: ONE ratio sequence
    z(r) = prod_{j <= r} (alpha - a - beta p) / (alpha - b - beta q) with beta = alpha^2 (`mix` is one ext challenge).
    constraints: first b = 0; last (b - (B - 1)) = 0; (1 - first) (b - b_-1) (b - b_-1 - 1) = 0; the z recurrence; last (z - 1) = 0.
    They hold iff b rises from 0 to B - 1 in steps of 0 or 1 and (b, q) is a permutation of (a, p): then every a lies in [0, B).
    Only rows [0, rows) are sorted, rows = N - RC_TAIL unless given: the base fills the tail of all four columns itself, a = b = B - 1
    and q = p there, so b stays sorted over all N rows and the two multisets still agree — the dests' rows at or above `rows` are part
    of the witness and must be left alone."""
    import acc_ratio_ref
    import cons_program_ref

    rows = (1 << po2) - RC_TAIL if rows is None else rows
    p = cons_program_ref.Program(0)
    xk = [None] + [p.const_ext(*[1 if i == k else 0 for i in range(4)]) for k in (1, 2, 3)]

    def ext_of(words):
        r = words[0]
        for k in (1, 2, 3):
            r = p.add(r, p.mul(xk[k], words[k]))
        return r

    alpha = ext_of([p.mix(k) for k in range(4)])
    beta = p.mul(alpha, alpha)
    first, last = p.get(0, 0), p.get(0, 1)
    not_first = p.sub(p.const(1), first)
    a, tag, b, q = (p.get(1, c) for c in range(4))
    step = p.sub(b, p.get(1, 2, 1))
    z = ext_of([p.get(2, k, 0) for k in range(4)])
    z_back = ext_of([p.get(2, k, 1) for k in range(4)])
    fa = p.sub(p.sub(alpha, a), p.mul(beta, tag))
    fb = p.sub(p.sub(alpha, b), p.mul(beta, q))
    top = p.and_eqz(p.true(), p.mul(first, b))
    top = p.and_eqz(top, p.mul(last, p.sub(b, p.const(RC_B - 1))))
    top = p.and_eqz(top, p.mul(not_first, p.mul(step, p.sub(step, p.const(1)))))
    top = p.and_eqz(top, p.sub(p.mul(z, fb), p.mul(p.add(p.mul(not_first, z_back), first), fa)))
    top = p.and_eqz(top, p.mul(last, p.sub(z, p.const(1))))
    cons = p.done(top)

    acc = acc_ratio_ref.Program(0)
    al = acc.alpha()
    be = acc.mul(al, al)
    acc.ratio(0, acc.sub(acc.sub(al, acc.get(1, 0, 0)), acc.mul(be, acc.get(1, 1, 0))), acc.sub(acc.sub(al, acc.get(1, 2, 0)), acc.mul(be, acc.get(1, 3, 0))))

    wit = Program()
    wit.sort([(0, RC_BITS)], [1], list(dests), rows)
    return cons, acc, wit


def range_code(po2):
    n = 1 << po2
    code = np.zeros((RC_WIDTHS[0], n), np.uint32)
    code[0][0] = code[1][n - 1] = encode(1)
    return code


def range_free_columns(po2, seed, cheat=False):
    """what the base fills: a (every value of [0, B) at least once, the padding; the rest uniform below B; B - 1 on the tail rows) and
    the tags p on all rows, and the tail rows of b and q; the sorted rows of b and q hold poison"""
    n = 1 << po2
    rows = n - RC_TAIL
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.arange(RC_B), rng.integers(0, RC_B, rows - RC_B)])
    rng.shuffle(a)
    a = np.concatenate([a, np.full(RC_TAIL, RC_B - 1)])
    if cheat:
        a[5] = RC_B + 1  # sorts last among the sorted rows: b ends above B - 1 and steps down into the tail
    data = np.full((RC_WIDTHS[1], n), POISON, np.uint32)
    data[0] = encode_words(a)
    data[1] = rng.integers(0, P, n, dtype=np.uint32)
    data[2:, rows:] = data[:2, rows:]
    return data


HOST_PROGRAMS = {
    "one_key_8": lambda n: (sort_program((8,), 1)[0], 4),
    "one_key_31_rows": lambda n: (sort_program((31,), 2, rows=n - 1)[0], 6),
    "two_keys": lambda n: (sort_program((24, 20), 0)[0], 4),
    "four_keys": lambda n: (sort_program((16, 16, 16, 16), 1, rows=max(n - 3, 1))[0], 10),
    "one_bit": lambda n: (sort_program((1,), 15)[0], 32),
    "set_key": lambda n: (set_key_program(), 8),
    "sorted_count": lambda n: (sorted_count_program(min(3, n)), 8),
    "two_sorts": lambda n: (two_sorts_program(rows_a=n - 1), 8),
}
