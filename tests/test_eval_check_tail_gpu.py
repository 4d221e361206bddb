"""GPU: the tail of the synthetic circuit's eval_check (csrc/circuit.hip: the accumulator, permutation-pair and boundary constraints on
the lazy ext arithmetic of csrc/lazy_ext.hpp) at the benchmark's counts, against the reference of tests/synth_ref.py bit for bit.

The eval_check tests of tests/test_synth_stages_gpu.py stop at E = 4 accumulators and two pairs; here the table's eval_check runs with
E = 16 and eight pairs (24 terms of the weighted accumulator: every fold period of its seven chains several times over), with one
accumulator and no pair, without the `last` selector (no pair, one boundary constraint) and with no ext-valued term at all, on
arbitrary evaluation matrices filled from tests/extreme_words.py — all +-P/2 in all three groups included — under a random and the
all -P/2 pair of mixes.  Every check word is canonical and equal to the reference's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as ref  # noqa: E402
from extreme_words import EDGE, pattern  # noqa: E402
from test_synth_stages_gpu import FILLS, HALF1, Stages, assert_same_matrix  # noqa: E402

from boundless_amd.hal import HipHal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
# (po2, widths, knobs) -> (E, pairs, globals) the shape has.  The wide shapes run at po2 = 6 (256 domain points, one workgroup: the
# Python reference takes 2.5 s there and 5 s at po2 = 8), the narrow ones at po2 = 8 (four workgroups); the taps one row back wrap
# across the domain's end in both
CASES = [
    (6, (16, 64, 64), (64, 4), (16, 8, 2)),   # the benchmark's counts through the compiled walk
    (6, (16, 64, 64), (48, 3), (16, 8, 2)),
    (8, (16, 8, 4), (64, 4), (1, 0, 2)),      # one accumulator, no pair
    (8, (1, 9, 8), (64, 4), (2, 0, 1)),       # no `last` selector: no pair, one boundary constraint
    (8, (16, 8, 3), (64, 4), (0, 0, 2)),      # nothing but base-valued terms
    (6, (16, 64, 64), (5, 2), (16, 8, 2)),    # the run-time kernel <0, 0> shares the tail
]


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.mark.parametrize("po2,widths,knobs,counts", CASES, ids=[f"{w[0]}-{w[1]}-{w[2]}-T{k[0]}G{k[1]}" for _, w, k, _ in CASES])
def test_eval_check_tail_is_the_references_quotient_at_the_benchmarks_counts(hal, po2, widths, knobs, counts):
    st = Stages(hal, po2, widths, knobs)
    try:
        sh = st.sh
        assert (sh.E, sh.pairs, sh.globals) == counts
        dom = 4 * sh.N
        rng = np.random.default_rng([widths[1], widths[2], knobs[0]])
        for k, names in enumerate(FILLS):
            host = [pattern(name, (w, dom), seed=100 * k + q) for q, (name, w) in enumerate(zip(names, (sh.wc, sh.wd, sh.wa)))]
            dev = [hal.copy_from(np.ascontiguousarray(m.reshape(-1))) for m in host]
            g = (EDGE[k % 8], EDGE[(3 * k + 3) % 8])
            memo = {}  # of the reference, for this set of matrices
            for poly_mix, mix in ((rng.integers(0, P, 4), rng.integers(0, P, 4)), (HALF1, HALF1)):
                got = st.eval_check(*dev, poly_mix, mix, g)
                assert got.max() < P, ("eval_check: a check word is not canonical", names)
                want = ref.check_quotient(sh, *host, poly_mix, mix, g, memo)
                assert_same_matrix(f"eval_check {names} poly_mix {list(poly_mix)} mix {list(mix)} g {g}", got, want)
    finally:
        st.close()
