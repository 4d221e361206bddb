"""GPU: the constraint sums (csrc/circuit_dev.hpp: cons_sum<TT, GG>, a 64-bit chain per sum, folded hi * R + lo and reduced once at
the end) inside witness_derive_kernel and eval_check_kernel, whose walk over the derived columns keeps the pool centred from one
cell to the next (DerivedRegs<true>).  The shapes are those where the walk's length, its wrap of the free columns and its sources
differ, at the flagship knobs (64, 4), and the smallest shape that reaches everything the constraint loop does at every compiled knob
pair plus one that takes the run-time form:

  widths        F   J   code columns   what it exercises
  (3, 34, 8)    17  17  1 selector     two full runs of eight cells and one more; F odd; back-taps at j = 0, 4, 8, 12, 16
  (5, 16, 8)    8   8   3 selectors    exactly eight cells
  (5, 9, 8)     5   4   3 selectors    fewer than eight cells; the free columns wrap inside the three initial loads' successors
  (2, 22, 8)    11  11  2 (no csel)    csel_col = -1: the constant one enters the pool as a centred word
  (1, 7, 4)     4   3   1 (no csel)    no `last` selector, one public word
  (5, 22, 8)    11  11  3 selectors    F odd and J no multiple of 8: the ring ends part-filled, back-taps j % 8 = 0, 4 twice and once
  (4, 16, 8)    8   8   2 selectors    both back-taps, a full ring, free columns that wrap, all 16 pool slots filled from a column:
                                       at (64, 4), (48, 3), (16, 3), (8, 2) and (5, 2), which has no specialisation

At po2 8 (four workgroups, taps that wrap): witgen against tests/synth_ref.py, and eval_check on matrices whose every cell is P/2 or
P/2 + 1 (centred +-P/2: with every entry +P/2 all terms of a sum have one sign and a chain reaches the largest value its plan allows)
and on one of uniformly random canonical words, each under a random poly_mix / mix and under the all-(P/2 + 1) one.  And whole proofs
at po2 9 (the smallest size the prover accepts), seal and roots word for word against the CPU oracle's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as ref  # noqa: E402
from extreme_words import pattern  # noqa: E402
from test_synth_stages_gpu import Stages, assert_same_matrix  # noqa: E402

from boundless_amd.hal import HipHal  # noqa: E402
from oracle import oracle_lib as ol  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
HALF1 = [P // 2 + 1] * 4
KNOBS = [(64, 4), (48, 3), (16, 3), (8, 2), (5, 2)]  # the four compiled pairs; (5, 2) takes the run-time form
# (widths, knobs, seed)
PROOFS = [((4, 16, 8), k, 1100 + k[0]) for k in KNOBS] + [((5, 22, 8), (64, 4), 1522), ((3, 34, 8), (64, 4), 1822), ((3, 34, 8), (64, 4), 1923)]
# (widths, knobs, (F, J))
CASES = [((3, 34, 8), (64, 4), (17, 17)), ((5, 16, 8), (64, 4), (8, 8)), ((5, 9, 8), (64, 4), (5, 4)), ((2, 22, 8), (64, 4), (11, 11)),
         ((1, 7, 4), (64, 4), (4, 3)), ((3, 34, 8), (48, 3), (17, 17)), ((3, 34, 8), (16, 3), (17, 17)), ((3, 34, 8), (8, 2), (17, 17)),
         ((5, 22, 8), (64, 4), (11, 11))] + [((4, 16, 8), k, (8, 8)) for k in KNOBS]
# (code, data, accum): every cell +P/2; every cell -P/2; signs alternating along the points; along the columns; mixed between the
# groups (twice); uniformly random canonical words
FILLS = [("all_half",) * 3, ("all_half1",) * 3, ("alt_half",) * 3, ("alt_half_rows",) * 3, ("all_half", "all_half1", "alt_half"),
         ("alt_half_rows", "alt_half", "all_half1"), ("random",) * 3]


def _id(widths, knobs):
    return f"{'-'.join(map(str, widths))}@{knobs[0]}x{knobs[1]}"


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.mark.parametrize("widths,knobs,seed", PROOFS, ids=[f"{_id(w, k)}-seed{s}" for w, k, s in PROOFS])
def test_segment_proof_is_the_oracles(widths, knobs, seed):
    from boundless_amd.prover import HipProverServer, Segment

    po2 = 9
    srv = HipProverServer(0, po2=po2, widths=widths, terms=knobs[0], degree=knobs[1])
    try:
        receipt = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
    finally:
        srv.close()
    seal, roots = ol.prove_segment(po2, *widths, seed, terms=knobs[0], degree=knobs[1])
    assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
    assert receipt.seal.size == seal.size
    bad = np.nonzero(receipt.seal != seal)[0]
    assert bad.size == 0, f"first differing seal words at {bad[:5]}"


@pytest.mark.parametrize("widths,knobs,fj", CASES, ids=[_id(w, k) for w, k, _ in CASES])
def test_witgen_and_eval_check_on_half_p_and_random_matrices(hal, widths, knobs, fj):
    st = Stages(hal, 8, widths, knobs)
    try:
        sh = st.sh
        assert (sh.F, sh.J) == fj
        seed = 190 + widths[1] + knobs[0]
        _, data, g = st.witgen(seed)
        want_data, want_g = ref.data_columns(sh, seed)
        assert_same_matrix("witgen", data.view().reshape(sh.wd, -1), want_data)
        assert g == want_g, ("witgen: public words", g, want_g)
        dom = 4 * sh.N
        rng = np.random.default_rng([19, *widths, *knobs])
        for k, names in enumerate(FILLS):
            host = [pattern(name, (w, dom), seed=10 * k + i) for i, (name, w) in enumerate(zip(names, (sh.wc, sh.wd, sh.wa)))]
            if names[0] != "random":
                assert all(((m == P // 2) | (m == P // 2 + 1)).all() for m in host)
            assert all(m.max() < P for m in host)
            dev = [hal.copy_from(np.ascontiguousarray(m.reshape(-1))) for m in host]
            gw = (P // 2 + (k & 1), P // 2 + 1 - (k & 1))
            memo = {}  # of the reference, for this set of matrices
            for poly_mix, mix in ((rng.integers(0, P, 4), rng.integers(0, P, 4)), (HALF1, HALF1)):
                got = st.eval_check(*dev, poly_mix, mix, gw)
                assert got.max() < P, ("eval_check: a check word is not canonical", names)
                assert_same_matrix(f"eval_check {names} poly_mix {list(poly_mix)}", got, ref.check_quotient(sh, *host, poly_mix, mix, gw, memo))
    finally:
        st.close()
