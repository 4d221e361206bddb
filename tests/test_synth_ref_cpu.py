"""CPU: the reference of the synthetic circuit (tests/synth_ref.py, written from include/bx_prover.h) stands on its own feet — every
constraint vanishes on every row of its own honest trace, and a changed cell breaks the constraints that read it — and agrees with the
library's host-only `constraints_at` entry of bx_synthetic_circuit() (the verifier's polynomial) on random ext tap values.  Only then
is it used as the yardstick of the device stages (tests/test_synth_stages_gpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as ref  # noqa: E402
from extreme_words import EDGE, MONT_ONE, NAMES, pattern, patterns  # noqa: E402

from boundless_amd.circuit import MAX_TAPS, TapReader, _TAP_AT, synthetic_circuit  # noqa: E402
from boundless_amd.prover import SegmentParams  # noqa: E402

P = ref.P
PO2 = 6
MIX = [ref.encode(v) for v in (123456789, 987654321, 55555, 1234567)]
CASES = [(w, ref.KNOBS[0]) for w in ref.SHAPES] + [(w, tg) for w in ((16, 24, 16), (5, 17, 9)) for tg in ref.KNOBS[1:]]


def honest(widths, knobs, seed=7, noise_seed=None):
    sh = ref.Shape(PO2, *widths, *knobs)
    code = ref.code_columns(sh)
    data, g = ref.data_columns(sh, seed, noise_seed)
    return sh, code, data, ref.accum_columns(sh, seed, data, MIX), g


def nonzero(sh, code, data, accum, g):
    """{(constraint index, row)} of the constraints that do not vanish"""
    return {(i, int(r)) for i, c in enumerate(ref.row_constraints(sh, code, data, accum, MIX, g)) for r in np.nonzero(c.any(axis=-1))[0]}


def test_the_pattern_generator_makes_what_its_names_say():
    assert EDGE == [0, 1, P - 1, P // 2, P // 2 + 1, P // 2 - 1, MONT_ONE, P - MONT_ONE] and MONT_ONE == (1 << 32) % P
    got = dict(patterns((3, 5), seed=1))
    assert list(got) == list(NAMES) and all(a.dtype == np.uint32 and a.shape == (3, 5) for a in got.values())
    assert (got["all_half"] == P // 2).all() and (got["all_half1"] == P // 2 + 1).all() and (got["all_pm1"] == P - 1).all()
    assert got["alt_half"][1].tolist() == [P // 2, P // 2 + 1, P // 2, P // 2 + 1, P // 2]
    assert got["alt_half_rows"][:, 2].tolist() == [P // 2, P // 2 + 1, P // 2]
    assert set(got["edge_mix"].ravel().tolist()) <= set(EDGE) and (got["random"] < P).all()
    assert set(pattern("edge_mix", 4096, 2).tolist()) == set(EDGE)
    assert np.array_equal(pattern("random", 7, 3), pattern("random", (7,), 3)) and not np.array_equal(pattern("random", 7, 3), pattern("random", 7, 4))


@pytest.mark.parametrize("widths,knobs", CASES)
def test_every_constraint_vanishes_on_every_row_of_an_honest_trace(widths, knobs):
    sh, code, data, accum, g = honest(widths, knobs, noise_seed=(5 if widths == (5, 17, 9) else None))
    assert (sh.N, sh.A) == (64, 48) and len(g) == sh.globals and sh.constraints == sh.J + sh.E + sh.pairs + sh.globals
    assert all(a.max(initial=0) < P for a in (code, data, accum))
    assert nonzero(sh, code, data, accum, g) == set()
    for p in range(sh.pairs):  # a permuted copy multiplies up to the same grand product over the active rows
        assert sorted(data[4 * p + 3][:sh.A].tolist()) == sorted(data[4 * p + 2][:sh.A].tolist())
        assert np.array_equal(accum[8 * p:8 * p + 4, sh.A - 1], accum[8 * p + 4:8 * p + 8, sh.A - 1])


def test_the_shape_rules_of_the_text():
    sh = ref.Shape(PO2, 16, 24, 16)
    assert (sh.F, sh.J, sh.E, sh.pairs, sh.globals, sh.T, sh.G) == (12, 12, 4, 2, 2, 64, 4)
    assert [sh.acc_src(e) for e in range(4)] == [2, 3, 6, 7]
    sh = ref.Shape(PO2, 5, 17, 9, 5, 2)
    assert (sh.F, sh.J, sh.E, sh.pairs, sh.T, sh.G) == (9, 8, 2, 1, 5, 2) and [sh.acc_src(e) for e in range(2)] == [2, 3]
    sh = ref.Shape(PO2, 3, 4, 6)
    assert (sh.F, sh.J, sh.E, sh.pairs) == (2, 2, 1, 0) and sh.acc_src(0) == 0 and sh.csel_col(5) == 2
    sh = ref.Shape(PO2, 1, 1, 1)
    assert (sh.F, sh.J, sh.E, sh.pairs, sh.globals, sh.constraints) == (1, 0, 0, 0, 1, 1) and sh.csel_col(0) is None
    assert ref.Shape(12, 16, 24, 16).Z == 1024 and ref.Shape(20, 16, 24, 16).Z == 1994
    assert [ref.Shape.pool_idx(t, f) for t, f in ((0, 0), (1, 0), (0, 1), (4, 1), (16, 0), (63, 4))] == [0, 7, 3, 0, 1, (441 + 12 + 60 + 3) % 16]


def test_a_changed_cell_breaks_the_constraints_that_read_it_and_no_other():
    sh, code, data, accum, g = honest((16, 24, 16), (64, 4))
    row = 20
    bad = data.copy()
    bad[sh.F + 11][row] = (int(bad[sh.F + 11][row]) + 1) % P  # the last derived column: read by its own constraint alone
    assert nonzero(sh, code, bad, accum, g) == {(11, row)}
    bad = data.copy()
    bad[sh.F + 3][row] = (int(bad[sh.F + 3][row]) + 1) % P  # a derived column in the ring of the eight that follow
    got = nonzero(sh, code, bad, accum, g)
    assert (3, row) in got and {i for i, _ in got} <= set(range(3, 12)) and {r for _, r in got} == {row}
    bad = data.copy()
    bad[4][row] = (int(bad[4][row]) + 1) % P  # free column 4: pool slot 1 of derived column 4 reads it two rows back
    got = nonzero(sh, code, bad, accum, g)
    assert (4, row + 2) in got and (4, row) in got and {r for _, r in got} <= {row, row + 2}
    bad = accum.copy()
    bad[5][row] = (int(bad[5][row]) + 1) % P  # accumulator 1: its own step at this row and at the next
    assert nonzero(sh, code, data, bad, g) == {(sh.J + 1, row), (sh.J + 1, row + 1)}
    bad = accum.copy()
    bad[4][sh.A - 1] = (int(bad[4][sh.A - 1]) + 1) % P  # ... at the last active row the closing constraint of pair 0 as well
    assert nonzero(sh, code, data, bad, g) == {(sh.J + 1, sh.A - 1), (sh.J + 1, sh.A), (sh.J + sh.E, sh.A - 1)}
    assert nonzero(sh, code, data, accum, ((g[0] + 1) % P, g[1])) == {(sh.constraints - 2, 0)}
    assert nonzero(sh, code, data, accum, (g[0], (g[1] + 1) % P)) == {(sh.constraints - 1, sh.A - 1)}


@pytest.mark.parametrize("widths,knobs", CASES)
def test_constraints_at_of_the_library_equals_the_reference_on_random_taps(widths, knobs):
    sh = ref.Shape(PO2, *widths, *knobs)
    rng = np.random.default_rng([widths[1], knobs[0], knobs[1]])
    vals = {}

    def tap_value(g, c, back):
        assert back in sh.taps(g, c), (g, c, back)
        return vals.setdefault((g, c, back), rng.integers(0, P, 4, dtype=np.uint64))

    def at(_ctx, g, c, back, out):
        for k, v in enumerate(tap_value(g, c, back)):
            out[k] = int(v)
        return None

    ops = synthetic_circuit().contents
    shape = SegmentParams(PO2, *widths, *knobs)
    backs = (C.c_uint32 * MAX_TAPS)()
    for grp, width in enumerate(widths):
        for c in range(width):
            assert list(backs[:ops.taps(None, C.byref(shape), grp, c, backs)]) == sh.taps(grp, c)
    assert ops.n_globals(None, C.byref(shape)) == sh.globals
    reader = TapReader(None, _TAP_AT(at))
    pm, mix, gl = (rng.integers(0, P, 4, dtype=np.uint64) for _ in range(3))
    words = lambda v: (C.c_uint32 * len(v))(*[int(x) for x in v])
    out = (C.c_uint32 * 4)()
    msg = ops.constraints_at(None, C.byref(shape), C.byref(reader), words(pm), words(mix), words(gl[:2]), out)
    assert not msg, C.cast(msg, C.c_char_p).value
    asked = set(vals)
    want = ref.mixed(sh, tap_value, pm, mix, gl[:2], ref.Ext)
    assert list(out) == [int(w) for w in want]
    assert set(vals) == asked  # the reference reads the taps the library reads, and both only taps of the columns' tap sets
