"""GPU: the factored constraint sum (csrc/circuit_dev.hpp: cons_sum<TT, GG> for G >= 3) inside the two kernels built on it,
witness_derive_kernel and eval_check_kernel, for every (T, G) the library compiles plus one pair that takes the run-time form.

Widths 4,16,8 are the smallest shape that reaches everything the constraint loop does: 8 derived columns (both back-taps, j % 8 = 0 and
4, and a full ring of previous derived columns), free columns that wrap, and every one of the 16 pool slots filled from a column.
  * a whole segment proof, seal and roots word for word against the CPU oracle's (po2 9: the smallest size the prover accepts);
  * witgen against the reference of tests/synth_ref.py, and eval_check on matrices whose every cell is P/2 or P/2 + 1 (centred: +P/2 and
    -P/2, the largest magnitudes every accumulator of the factored form can meet), at po2 8: four workgroups, taps that wrap.
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
WIDTHS = (4, 16, 8)
KNOBS = [(64, 4), (48, 3), (16, 3), (8, 2), (5, 2)]  # the four compiled pairs; (5, 2) has no specialisation
HALF1 = [P // 2 + 1] * 4
# (code, data, accum): every cell +P/2; every cell -P/2; signs alternating along the points; along the columns; mixed between the groups
FILLS = [("all_half",) * 3, ("all_half1",) * 3, ("alt_half",) * 3, ("alt_half_rows",) * 3, ("all_half", "all_half1", "alt_half"),
         ("alt_half_rows", "alt_half", "all_half1")]


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.mark.parametrize("knobs", KNOBS)
def test_segment_proof_is_the_oracles_for_every_compiled_knob_pair(knobs):
    from boundless_amd.prover import HipProverServer, Segment

    po2, seed = 9, 1100 + knobs[0]
    srv = HipProverServer(0, po2=po2, widths=WIDTHS, terms=knobs[0], degree=knobs[1])
    try:
        receipt = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
    finally:
        srv.close()
    seal, roots = ol.prove_segment(po2, *WIDTHS, seed, terms=knobs[0], degree=knobs[1])
    assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
    assert receipt.seal.size == seal.size
    bad = np.nonzero(receipt.seal != seal)[0]
    assert bad.size == 0, f"first differing seal words at {bad[:5]}"


@pytest.mark.parametrize("knobs", KNOBS)
def test_witgen_and_eval_check_on_matrices_of_half_p(hal, knobs):
    st = Stages(hal, 8, WIDTHS, knobs)
    try:
        sh = st.sh
        seed = 31 + knobs[0]
        _, data, g = st.witgen(seed)
        want_data, want_g = ref.data_columns(sh, seed)
        assert_same_matrix("witgen", data.view().reshape(sh.wd, -1), want_data)
        assert g == want_g, ("witgen: public words", g, want_g)
        dom = 4 * sh.N
        rng = np.random.default_rng([knobs[0], knobs[1]])
        for k, names in enumerate(FILLS):
            host = [pattern(name, (w, dom), seed=k) for name, w in zip(names, (sh.wc, sh.wd, sh.wa))]
            assert all(((m == P // 2) | (m == P // 2 + 1)).all() for m in host)
            dev = [hal.copy_from(np.ascontiguousarray(m.reshape(-1))) for m in host]
            gw = (P // 2 + (k & 1), P // 2 + 1 - (k & 1))
            memo = {}  # of the reference, for this set of matrices
            for poly_mix, mix in ((rng.integers(0, P, 4), rng.integers(0, P, 4)), (HALF1, HALF1)):
                got = st.eval_check(*dev, poly_mix, mix, gw)
                assert got.max() < P, ("eval_check: a check word is not canonical", names)
                assert_same_matrix(f"eval_check {names} poly_mix {list(poly_mix)}", got, ref.check_quotient(sh, *host, poly_mix, mix, gw, memo))
    finally:
        st.close()
