"""GPU: the synthetic circuit (include/bx_prover.h, csrc/circuit.hip) stage by stage through its bx_circuit_ops entries, against the
reference of tests/synth_ref.py (anchored on the CPU by tests/test_synth_ref_cpu.py).

witgen / accumulate: word for word the reference's matrices, for every shape rule and every (T, G) the library compiles its constraint
sum for (witness_derive_kernel<TT, GG>) plus three that take the run-time form.  eval_check: the reference's quotient on the honest
committed evaluations, and on ARBITRARY evaluation matrices filled from tests/extreme_words.py — eval_check takes any matrices, so
this is where every one of the 16 pool entries of the compiled cons_sum<TT, GG> is +-P/2 at once (the largest magnitudes of the
centred arithmetic of circuit_dev.hpp / lazy_ext.hpp; circuit.hip leaves its multiply-adds to the compiler).  A mismatch names the
stage, the column or plane, and the row or point.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as ref  # noqa: E402
from extreme_words import EDGE, EXTREME, pattern  # noqa: E402

from boundless_amd.circuit import synthetic_circuit  # noqa: E402
from boundless_amd.hal import BxBuf, HalError, HipHal  # noqa: E402
from boundless_amd.prover import Segment, SegmentParams  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
PO2 = 9  # 2048 domain points: 8 workgroups, the taps one and two rows back wrap across workgroup and domain ends
MIX = [ref.encode(v) for v in (123456789, 987654321, 55555, 1234567)]
POLY_MIX = [ref.encode(v) for v in (1111, 2222222, 333, 444444444)]
BIG, ODD = (16, 24, 16), (5, 17, 9)
_SET_NOISE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint64)


def _text(msg):
    return C.cast(msg, C.c_char_p).value.decode() if msg else None


class Stages:
    """The synthetic circuit's table driven entry by entry on one ctx"""

    def __init__(self, hal, po2, widths, knobs):
        self.hal, self.ops = hal, synthetic_circuit().contents
        self.shape = SegmentParams(po2, *widths, *knobs)
        msg = self.ops.normalize(None, C.byref(self.shape))  # (0, 0) -> the default knobs
        assert not msg, _text(msg)
        self.sh = ref.Shape(po2, *widths, *knobs)
        assert (self.shape.cons_terms, self.shape.cons_degree) == (self.sh.T, self.sh.G)
        self.state = C.c_void_p()
        msg = self.ops.create(None, hal.ctx, C.byref(self.shape), C.byref(self.state))
        assert not msg, _text(msg)

    def close(self):
        self.hal.sync()
        self.ops.destroy(None, self.state)

    def witgen(self, seed, noise_seed=None, seg_po2=None):
        """-> (code, data) device buffers and the public words; seg_po2: what the segment's header says, if not the shape's po2"""
        sh = self.sh
        code, data = self.hal.alloc(sh.N * sh.wc), self.hal.alloc(sh.N * sh.wd)
        msg = self.ops.code_group(None, self.state, self.hal.ctx, code.raw)
        assert not msg, _text(msg)
        if noise_seed is not None:
            _SET_NOISE(self.ops.set_noise_seed)(None, self.state, noise_seed)
        blob = Segment(index=0, po2=sh.po2 if seg_po2 is None else seg_po2, seed=seed).to_bytes()
        seg = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        g = (C.c_uint32 * 2)()
        msg = self.ops.witgen(None, self.state, self.hal.ctx, code.raw, data.raw, seg, len(blob), BxBuf(None, 0), g)
        if msg:
            raise HalError(_text(msg))
        return code, data, tuple(int(v) for v in g[:sh.globals])

    def accumulate(self, mix=MIX):
        accum = self.hal.alloc(self.sh.N * self.sh.wa)
        msg = self.ops.accumulate(None, self.state, self.hal.ctx, accum.raw, (C.c_uint32 * 4)(*[int(v) for v in mix]))
        assert not msg, _text(msg)
        return accum

    def eval_check(self, ecode, edata, eacc, poly_mix, mix, g):
        """device buffers of the three (w, 4N) evaluation matrices -> the four check planes (4, 4N) on the host"""
        check = self.hal.alloc(16 * self.sh.N)
        gw = (C.c_uint32 * 2)(*[int(v) for v in g])
        msg = self.ops.eval_check(None, self.state, self.hal.ctx, check.raw, ecode.raw, edata.raw, eacc.raw, (C.c_uint32 * 4)(*[int(v) for v in poly_mix]),
                                  (C.c_uint32 * 4)(*[int(v) for v in mix]), gw)
        assert not msg, _text(msg)
        return check.view().reshape(4, 4 * self.sh.N).copy()


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def assert_same_matrix(stage, got, want):
    """bit-exact, and on a mismatch the first differing (column or plane, row or point)"""
    assert got.shape == want.shape, (stage, got.shape, want.shape)
    if not np.array_equal(got, want):
        col, row = (int(v[0]) for v in np.nonzero(got != want))
        pytest.fail(f"{stage}: {int((got != want).sum())} words differ, first at (column/plane {col}, row/point {row}): got {int(got[col][row])}, "
                    f"want {int(want[col][row])}")


# ---- witgen and accumulate ----
def _witness_equals_reference(hal, po2, widths, knobs, seed, noise_seed=None):
    st = Stages(hal, po2, widths, knobs)
    try:
        sh = st.sh
        code, data, g = st.witgen(seed, noise_seed)
        accum = st.accumulate()
        want_data, want_g = ref.data_columns(sh, seed, noise_seed)
        assert_same_matrix("code_group", code.view().reshape(sh.wc, -1), ref.code_columns(sh))
        assert_same_matrix("witgen", data.view().reshape(sh.wd, -1), want_data)
        assert g == want_g, ("witgen: public words", g, want_g)
        assert_same_matrix("accumulate", accum.view().reshape(sh.wa, -1), ref.accum_columns(sh, seed, want_data, MIX))
    finally:
        st.close()


@pytest.mark.parametrize("widths", ref.SHAPES)
def test_witgen_and_accumulate_are_the_references_words_for_every_shape_rule(hal, widths):
    _witness_equals_reference(hal, PO2, widths, (0, 0), seed=1000 + widths[1])  # (0, 0): the default knobs, (64, 4)


@pytest.mark.parametrize("knobs", ref.KNOBS)
def test_witgen_and_accumulate_are_the_references_words_for_every_knob_pair(hal, knobs):
    _witness_equals_reference(hal, PO2, BIG, knobs, seed=77 + knobs[0])


def test_witgen_with_a_given_noise_seed_and_in_a_single_workgroup(hal):
    _witness_equals_reference(hal, PO2, BIG, (64, 4), seed=5, noise_seed=0xFEEDFACE12345678)
    _witness_equals_reference(hal, PO2, ODD, (48, 3), seed=6, noise_seed=1)
    _witness_equals_reference(hal, 6, BIG, (64, 4), seed=7)  # 64 rows: one 256-lane workgroup, a quarter of it idle in witgen


def test_a_refused_segment_uses_up_the_noise_seed_given_for_it(hal):
    """set_noise_seed is for the NEXT witgen, accepted or refused (bx_circuit.h): after a segment of the wrong po2 the following witgen
    draws its ZK rows from the default generator, not from the seed given for the refused one."""
    st = Stages(hal, PO2, BIG, (0, 0))
    try:
        with pytest.raises(HalError, match=f"was created for po2 {PO2}"):
            st.witgen(31, noise_seed=0xDEC0DE5EED, seg_po2=PO2 + 1)
        _, data, g = st.witgen(31)
        want_data, want_g = ref.data_columns(st.sh, 31)
        assert_same_matrix("witgen after a refused segment", data.view().reshape(st.sh.wd, -1), want_data)
        assert g == want_g
    finally:
        st.close()


# ---- eval_check on the honest committed evaluations ----
@pytest.mark.parametrize("po2,knobs", [(PO2, k) for k in ref.KNOBS] + [(6, (64, 4))])
def test_eval_check_is_the_references_quotient_on_an_honest_trace(hal, po2, knobs):
    """The committed 4N evaluations of an honest trace (interpolate, coset shift, 4x evaluation: the HAL's own entry points) through
    the table's eval_check: the 16 check columns are the quotient the reference computes point by point."""
    st = Stages(hal, po2, BIG, knobs)
    try:
        sh = st.sh
        code, data, g = st.witgen(4242)
        accum = st.accumulate()
        evals = []
        for buf, width in ((code, sh.wc), (data, sh.wd), (accum, sh.wa)):
            hal.batch_interpolate_ntt(buf, width)
            hal.zk_shift(buf, width)
            ev = hal.alloc(4 * sh.N * width)
            hal.batch_expand_into_evaluate_ntt(ev, buf, width, 2)
            evals.append(ev)
        got = st.eval_check(*evals, POLY_MIX, MIX, g)
        host = [e.view().reshape(w, 4 * sh.N) for e, w in zip(evals, (sh.wc, sh.wd, sh.wa))]
        assert_same_matrix("eval_check (honest trace)", got, ref.check_quotient(sh, *host, POLY_MIX, MIX, g))
        assert got.any()  # a quotient, not the zero polynomial: the constraints vanish on the trace domain only
    finally:
        st.close()


# ---- eval_check on arbitrary matrices ----
# (code, data, accum) patterns: each pattern in all three groups at once — with all_half / all_half1 / alt_half every pool entry, every
# constraint value's operands and every accumulator tap are +-P/2 — then each extreme pattern in the data group alone between random
# neighbours, then three mixtures
FILLS = ([(n, n, n) for n in EXTREME + ("random",)] + [("random", n, "random") for n in EXTREME] +
         [("all_half", "all_half1", "alt_half"), ("alt_half_rows", "alt_half", "all_pm1"), ("edge_mix", "all_half", "all_half1")])
HALF1 = [P // 2 + 1] * 4


@pytest.mark.parametrize("knobs", ref.KNOBS)
@pytest.mark.parametrize("widths", [BIG, ODD])
def test_eval_check_is_the_references_quotient_on_extreme_matrices(hal, widths, knobs):
    st = Stages(hal, PO2, widths, knobs)
    try:
        sh = st.sh
        dom = 4 * sh.N
        rng = np.random.default_rng([widths[1], knobs[0], knobs[1]])
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
