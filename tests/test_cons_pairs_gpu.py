"""GPU: the pair form of the degree-4 constraint sum (csrc/circuit_dev.hpp: cons_sum<TT, 4>) inside witness_derive_kernel and
eval_check_kernel at the flagship knobs (64, 4), on a shape the column walk treats differently from the (4, 16, 8) of
test_cons_factored_gpu.py.

Widths 5,22,8: F = 11 free columns (odd, so the free columns j+1, j+2 wrap out of step with the ring), J = 11 derived columns (no
multiple of 8: the ring of previous derived columns ends part-filled and the back-taps j % 8 = 0, 4 occur twice and once), three
code selectors, one permutation pair.
  * a whole segment proof at po2 9, seal and roots word for word against the CPU oracle's;
  * at po2 8 (four workgroups, taps that wrap): witgen against tests/synth_ref.py, and eval_check on matrices whose every cell is P/2 or
    P/2 + 1 (centred +-P/2: the largest magnitudes every pair product and accumulator can meet) and on one of uniformly random
    canonical words, each under a random poly_mix / mix and under the all-(P/2 + 1) one.
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
WIDTHS = (5, 22, 8)
KNOBS = (64, 4)
HALF1 = [P // 2 + 1] * 4
# (code, data, accum): the six fills of +-P/2 of test_cons_factored_gpu.py, and uniformly random canonical words
FILLS = [("all_half",) * 3, ("all_half1",) * 3, ("alt_half",) * 3, ("alt_half_rows",) * 3, ("all_half", "all_half1", "alt_half"),
         ("alt_half_rows", "alt_half", "all_half1"), ("random",) * 3]


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def test_segment_proof_of_an_odd_shape_is_the_oracles():
    from boundless_amd.prover import HipProverServer, Segment

    po2, seed = 9, 1522
    srv = HipProverServer(0, po2=po2, widths=WIDTHS, terms=KNOBS[0], degree=KNOBS[1])
    try:
        receipt = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
    finally:
        srv.close()
    seal, roots = ol.prove_segment(po2, *WIDTHS, seed, terms=KNOBS[0], degree=KNOBS[1])
    assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
    assert receipt.seal.size == seal.size
    bad = np.nonzero(receipt.seal != seal)[0]
    assert bad.size == 0, f"first differing seal words at {bad[:5]}"


def test_witgen_and_eval_check_of_an_odd_shape_on_half_p_and_random_matrices(hal):
    st = Stages(hal, 8, WIDTHS, KNOBS)
    try:
        sh = st.sh
        assert (sh.F, sh.J) == (11, 11)
        seed = 95
        _, data, g = st.witgen(seed)
        want_data, want_g = ref.data_columns(sh, seed)
        assert_same_matrix("witgen", data.view().reshape(sh.wd, -1), want_data)
        assert g == want_g, ("witgen: public words", g, want_g)
        dom = 4 * sh.N
        rng = np.random.default_rng([15, *WIDTHS])
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
