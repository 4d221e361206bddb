"""Definition-level reference of a witness program's multiplicity columns (include/bx_program.h, "multiplicity columns"), written from
that text and sharing no code with the library: the per-row part is tests/wit_program_ref.py's, a count is np.bincount over the
decoded cells of its source columns.  Words are Montgomery words, canonical in [0, P).

Also here: the named programs the tests run, the helpers that hand a program to the library's builder and make columns, and the
lookup circuit's count (V values, two limbs each, B bins, A active rows)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wit_program_ref as ref  # noqa: E402

P, U = ref.P, np.uint64
encode = ref.encode
POISON = P - 1
MAX_COUNTS, MAX_SOURCES, MAX_BINS = 16, 64, 1 << 24  # BX_WIT_MAX_COUNTS, BX_WIT_MAX_COUNT_SOURCES, BX_WIT_MAX_COUNT_BINS


def decode_words(words):
    """Montgomery words -> the integers they stand for"""
    return np.asarray(words, U) * U(ref.R_INV) % U(P)


def encode_words(values):
    return (np.asarray(values, U) % U(P) * U(ref.R) % U(P)).astype(np.uint32)


class Program(ref.Program):
    """a witness program with a count list: counts = [(col, sources, bins, rows)]"""

    def __init__(self):
        super().__init__()
        self.counts = []

    def count(self, col, sources, bins, rows=0):
        self.counts.append((int(col), [int(s) for s in sources], int(bins), int(rows)))

    def count_cols(self):
        return [c[0] for c in self.counts]

    def written(self):
        """every column the run writes: SET columns and count columns"""
        return self.derived() + self.count_cols()


def evaluate(prog, po2, code, data):
    """-> the data matrix (w_data, N) after the per-row program and then the counts, in list order; the inputs are left unchanged"""
    n = 1 << po2
    out = ref.evaluate(prog, po2, code, data)
    for col, sources, bins, rows in prog.counts:
        rows = rows or n
        values = decode_words(out[sources, :rows]).reshape(-1)
        c = np.bincount(values[values < bins].astype(np.int64), minlength=bins)  # a cell that holds no value below B is not counted
        m = np.zeros(rows, U)
        m[:bins] = c  # bins <= rows by the rules: a broken rule shows as a shape error
        out[col, :rows] = encode_words(m)
    return out


def in_range_cells(prog, k, po2, data_after):
    """how many cells count k looks at hold a value below its bins"""
    col, sources, bins, rows = prog.counts[k]
    rows = rows or (1 << po2)
    return int(np.sum(decode_words(data_after[sources, :rows]) < bins))


def to_builder(prog):
    from wit_program_cases import to_builder as base

    b = base(prog)
    for col, sources, bins, rows in getattr(prog, "counts", []):
        b.count(col, sources, bins, rows)
    return b


def compile_ref(prog):
    return to_builder(prog).compile()


# ---- columns ----
def source_columns(kind, shape, bins, seed=0):
    """a (columns, N) matrix of Montgomery words: "same" every cell the value bins - 1, "mod" row r holds r mod bins (all distinct within
    a wave when bins >= 64), "random" uniform values of which about three quarters lie below bins, "above" every value >= bins"""
    w, n = shape
    rng = np.random.default_rng([seed, w, n, bins])
    if kind == "same":
        v = np.full(shape, bins - 1, U)
    elif kind == "mod":
        v = np.broadcast_to(np.arange(n, dtype=U) % U(bins), shape)
    elif kind == "random":
        v = rng.integers(0, bins + max(bins // 3, 1), shape).astype(U)
    elif kind == "above":
        v = rng.integers(bins, P, shape).astype(U)
    else:
        raise ValueError(kind)
    return encode_words(v)


# ---- programs over WIDTHS = (3, 8): free data columns 0, 1, 2, 4 ----
WIDTHS = ref.WIDTHS


def counts_only_program(bins, rows=0, sources=(0, 1), col=6):
    p = Program()
    p.count(col, sources, bins, rows)
    return p


def set_source_program(bins, rows=0):
    """column 3 = column 0 + column 1 (SET), counted together with the free column 2 into column 6; public word 0 is m(0)"""
    p = Program()
    p.set(3, p.add(p.get(1, 0, 0), p.get(1, 1, 0)))
    p.set(5, p.mul(p.get(1, 3, 0), p.get(0, 1, 1)))
    p.count(6, [3, 2], bins, rows)
    p.global_cell(0, 6, 0)
    return p


def two_counts_program(bins_a, bins_b, rows_a=0, rows_b=0):
    """two counts in one program, over overlapping sources, with different bins and rows; and a per-row part"""
    p = Program()
    p.set(3, p.mul(p.get(1, 0, 1), p.get(1, 4, 0)))
    p.count(6, [0, 1], bins_a, rows_a)
    p.count(7, [1, 2, 4], bins_b, rows_b)
    return p


def wide_program(n_sources, bins, rows=0):
    """data width n_sources + 1: every column but the last is a source, the last the multiplicities"""
    p = Program()
    p.count(n_sources, list(range(n_sources)), bins, rows)
    return p


def lookup_count(V, bins, rows):
    """the built-in lookup circuit's multiplicity column as a count: the limbs of value j are data columns 3j+1 and 3j+2, m is 3V"""
    p = Program()
    p.count(3 * V, [3 * j + k for j in range(V) for k in (1, 2)], bins, rows)
    return p
