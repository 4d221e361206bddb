"""GPU: the lookup circuit (include/bx_lookup.h, csrc/lookup.hip) against the reference of tests/lookup_ref.py and the host verifier.

Stages through the bx_circuit_ops entries directly (witgen, accumulate, eval_check: word for word the reference's matrices), whole
proofs through bx_prove_segment_bytes / bx_verify_segment_with_circuit, soundness through the segment's cell records (a false
witness reaches the prover through the public interface; the prover emits a seal and the verifier decides), the kept code
commitment, and the sha-256 suite.  tests/plain_hal.py drives the synthetic circuit only (ph_create takes no circuit table), so the
trait-level driver is not compared here.
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import logup_ref as lr  # noqa: E402
import lookup_ref as ref  # noqa: E402

from boundless_amd.circuit import encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import BxBuf, HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, SegmentParams, lookup_control_id_host, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
ALPHA = [lr.encode(v) for v in (123456789, 987654321, 55555, 1234567)]
POLY_MIX = [lr.encode(v) for v in (1111, 2222222, 333, 444444444)]
# V = 1 without filler; V = 7 with filler in every group; a w_accum that is no multiple of 4; b capped at 15 (B < N/2)
SHAPES = [(9, (3, 4, 12)), (12, (16, 32, 64)), (12, (16, 32, 30)), (17, (3, 7, 20))]
_SET_NOISE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint64)


def _text(msg):
    return C.cast(msg, C.c_char_p).value.decode() if msg else None


class Stages:
    """The lookup circuit's table driven entry by entry on one ctx"""

    def __init__(self, hal, po2, widths):
        self.hal, self.ops = hal, lookup_circuit().contents
        self.sh = ref.Shape(po2, *widths)
        self.shape = SegmentParams(po2, *widths, 0, 0)
        self.state = C.c_void_p()
        msg = self.ops.create(None, hal.ctx, C.byref(self.shape), C.byref(self.state))
        assert not msg, _text(msg)

    def close(self):
        self.hal.sync()
        self.ops.destroy(None, self.state)

    def witgen(self, seed, payload=b"", noise_seed=None):
        """-> (code, data) device buffers and the two public words; raises HalError with witgen's message"""
        sh = self.sh
        code, data = self.hal.alloc(sh.N * sh.wc), self.hal.alloc(sh.N * sh.wd)
        assert not self.ops.code_group(None, self.state, self.hal.ctx, code.raw)
        if noise_seed is not None:
            _SET_NOISE(self.ops.set_noise_seed)(None, self.state, noise_seed)
        blob = Segment(index=0, po2=sh.po2, seed=seed, payload=payload).to_bytes()
        seg = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        g = (C.c_uint32 * 2)()
        msg = self.ops.witgen(None, self.state, self.hal.ctx, code.raw, data.raw, seg, len(blob), BxBuf(None, 0), g)
        if msg:
            raise HalError(_text(msg))
        return code, data, (int(g[0]), int(g[1]))

    def accumulate(self, alpha=ALPHA):
        accum = self.hal.alloc(self.sh.N * self.sh.wa)
        msg = self.ops.accumulate(None, self.state, self.hal.ctx, accum.raw, (C.c_uint32 * 4)(*alpha))
        assert not msg, _text(msg)
        return accum


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def _reference(sh, seed, records=(), noise_seed=None):
    code = ref.code_columns(sh)
    data, g = ref.data_columns(sh, seed, noise_seed=noise_seed, records=records)
    return code, data, g, ref.accum_columns(sh, seed, code, data, ALPHA)


def _stages_equal_reference(hal, po2, widths, seed, records=(), noise_seed=None):
    st = Stages(hal, po2, widths)
    try:
        code, data, g = st.witgen(seed, encode_cell_records(records), noise_seed)
        accum = st.accumulate()
        want_code, want_data, want_g, want_accum = _reference(st.sh, seed, records, noise_seed)
        assert np.array_equal(code.view().reshape(st.sh.wc, -1), want_code)
        assert np.array_equal(data.view().reshape(st.sh.wd, -1), want_data)
        assert g == want_g
        assert np.array_equal(accum.view().reshape(st.sh.wa, -1), want_accum)
    finally:
        st.close()


# ---- stages ----
@pytest.mark.parametrize("po2,widths", SHAPES)
def test_witgen_and_accumulate_are_the_references_words(hal, po2, widths):
    _stages_equal_reference(hal, po2, widths, seed=1000 + po2, noise_seed=(77 if po2 == 12 else None))


@pytest.mark.parametrize("lookback,hist_lds", [(0, 1), (1, 0)])
def test_the_other_scan_and_the_other_histogram_give_the_same_words(hal, lookback, hist_lds):
    hal.set_tunable("scan_lookback", lookback)
    hal.set_tunable("lookup_hist_lds", hist_lds)
    try:
        _stages_equal_reference(hal, 12, (16, 32, 64), seed=5)
    finally:
        hal.set_tunable("scan_lookback", 1)
        hal.set_tunable("lookup_hist_lds", 1)


@pytest.mark.parametrize("hist_lds", [1, 0])
def test_records_that_move_1000_limbs_onto_one_bin(hal, hist_lds):
    sh = ref.Shape(12, 16, 32, 64)
    rng = np.random.default_rng(3)
    cells = {(int(3 * j + 1 + k), int(r)) for j, k, r in zip(rng.integers(0, sh.V, 1500), rng.integers(0, 2, 1500), rng.integers(0, sh.A, 1500))}
    records = [(c, r, 77) for c, r in sorted(cells)[:1000]]
    records += [records[0][:2] + (5,), records[0][:2] + (77,)]  # a cell named three times: the last record wins
    assert len(records) == 1002
    hal.set_tunable("lookup_hist_lds", hist_lds)
    try:
        _stages_equal_reference(hal, 12, (16, 32, 64), seed=6, records=records)
    finally:
        hal.set_tunable("lookup_hist_lds", 1)


@pytest.mark.parametrize("po2,widths", [(9, (3, 4, 12)), (10, (4, 7, 20))])
def test_eval_check_is_the_references_quotient(hal, po2, widths):
    """The committed 4N evaluations of an honest trace (interpolate, coset shift, 4x evaluation: the HAL's own entry points) go
    through the table's eval_check; the 16 check columns are the quotient the reference computes point by point."""
    st = Stages(hal, po2, widths)
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
        check = hal.alloc(16 * sh.N)
        msg = st.ops.eval_check(None, st.state, hal.ctx, check.raw, evals[0].raw, evals[1].raw, evals[2].raw, (C.c_uint32 * 4)(*POLY_MIX),
                                (C.c_uint32 * 4)(*ALPHA), (C.c_uint32 * 2)(*g))
        assert not msg, _text(msg)
        host = [e.view().reshape(w, 4 * sh.N) for e, w in zip(evals, (sh.wc, sh.wd, sh.wa))]
        want = ref.check_quotient(sh, host[0], host[1], host[2], POLY_MIX, ALPHA, g)
        assert np.array_equal(check.view().reshape(4, 4 * sh.N), want)
    finally:
        st.close()


@pytest.mark.parametrize("name", extreme_words.NAMES)
def test_eval_check_is_the_references_quotient_on_extreme_matrices(hal, name):
    """eval_check takes any evaluation matrices: filled with the words of largest magnitude for the centred arithmetic
    (tests/extreme_words.py), the ext x ext product step * den of every running-sum constraint sees +-P/2 on both sides — with
    alpha = (0, h, h', h) and limbs of -P/2 every word of den is +-P/2."""
    po2, widths = 9, (3, 4, 12)
    st = Stages(hal, po2, widths)
    try:
        sh = st.sh
        dom = 4 * sh.N
        host = [extreme_words.pattern(name, (w, dom), seed=q) for q, w in enumerate(widths)]
        dev = [hal.copy_from(np.ascontiguousarray(m.reshape(-1))) for m in host]
        half = extreme_words.HALF
        for poly_mix, alpha, g in ((POLY_MIX, ALPHA, (half, half + 1)), ([half + 1] * 4, [0, half, half + 1, half], (P - 1, half))):
            check = hal.alloc(16 * sh.N)
            msg = st.ops.eval_check(None, st.state, hal.ctx, check.raw, dev[0].raw, dev[1].raw, dev[2].raw, (C.c_uint32 * 4)(*poly_mix),
                                    (C.c_uint32 * 4)(*alpha), (C.c_uint32 * 2)(*g))
            assert not msg, _text(msg)
            got = check.view().reshape(4, dom)
            want = ref.check_quotient(sh, host[0], host[1], host[2], poly_mix, alpha, g)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{len(bad)} check words differ, first at (plane, point) {tuple(bad[0])}; alpha {alpha}"
    finally:
        st.close()


def test_witgen_refuses_bad_payloads_by_message(hal):
    st = Stages(hal, 12, (16, 32, 64))
    try:
        sh = st.sh
        with pytest.raises(HalError, match="whole number of 12-byte cell records"):
            st.witgen(1, b"\0" * 13)
        with pytest.raises(HalError, match=r"cell record 1 \(col 1, row %d, value %d\) is out of bounds" % (sh.A, sh.B)):
            st.witgen(1, encode_cell_records([(0, 0, 1), (1, sh.A, sh.B)]))  # a limb = B in a noise row is not patchable
        with pytest.raises(HalError, match="out of bounds"):
            st.witgen(1, encode_cell_records([(3 * sh.V, 0, 1)]))  # the multiplicity column
        with pytest.raises(HalError, match="out of bounds"):
            st.witgen(1, encode_cell_records([(0, 0, P)]))
        with pytest.raises(HalError, match="more than 65536 cell records"):
            st.witgen(1, encode_cell_records([(0, 0, 1)] * 65537))
    finally:
        st.close()


# ---- whole proofs ----
def _server(po2, widths, hal=None, hashfn=None):
    return HipProverServer(0, po2=po2, widths=widths, hal=hal, circuit="lookup", hashfn=hashfn)


@pytest.mark.parametrize("po2,widths", SHAPES)
def test_a_lookup_seal_is_accepted_by_its_circuit_and_by_no_other(po2, widths):
    srv = _server(po2, widths)
    try:
        r = srv.prove_segment(Segment(index=0, po2=po2, seed=31 + po2))
        assert r.seal[:6].tolist() == [po2, *widths, 0, 0]
        assert r.seal.size == srv.lib.bx_prover_seal_words(srv.handle)
        verify_seal(r.seal, circuit="lookup")
        with pytest.raises(HalError):
            verify_seal(r.seal, circuit="synthetic")
        with pytest.raises(HalError):
            verify_seal(r.seal)  # plain bx_verify_segment
        sh = ref.Shape(po2, *widths)
        _, g = ref.data_columns(sh, 31 + po2)
        assert r.public_words().tolist() == list(g)
        if po2 == 12:  # two noise seeds: two different accepted seals of the same statement
            a = srv.prove_segment(Segment(index=0, po2=po2, seed=31 + po2, noise_seed=1))
            b = srv.prove_segment(Segment(index=0, po2=po2, seed=31 + po2, noise_seed=2))
            assert not np.array_equal(a.seal, b.seal) and np.array_equal(a.public_words(), b.public_words())
            verify_seal(a.seal, circuit="lookup")
            verify_seal(b.seal, circuit="lookup")
    finally:
        srv.close()


def test_three_provers_in_flight_on_three_contexts():
    srvs = [_server(12, (16, 32, 64)) for _ in range(3)]
    seals, errs = [None] * 3, []

    def work(k):
        try:
            for i in range(2):
                seals[k] = srvs[k].prove_segment(Segment(index=i, po2=12, seed=900 + k)).seal
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errs.append(e)

    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for s in seals:
            verify_seal(s, circuit="lookup")
        assert not np.array_equal(seals[0], seals[1])
    finally:
        for s in srvs:
            s.close()


# ---- soundness through the payload ----
def test_the_verifier_decides_what_the_records_made_of_the_witness():
    po2, widths = 12, (16, 32, 64)
    sh = ref.Shape(po2, *widths)
    srv = _server(po2, widths)

    def prove(records):
        return srv.prove_segment(Segment(index=0, po2=po2, seed=8, payload=encode_cell_records(records)))

    try:
        # consistent in-range records for (v_0, lo_0, hi_0) at row 0: accepted, and g_0 is the new value
        r = prove([(0, 0, 7 + sh.B * 9), (1, 0, 7), (2, 0, 9)])
        verify_seal(r.seal, circuit="lookup")
        assert int(r.public_words()[0]) == lr.encode(7 + sh.B * 9)
        # a limb = B with v matched: every local constraint holds, the running sums do not close
        data, _ = ref.data_columns(sh, 8)
        hi = lr.decode(int(data[2][50]))
        r = prove([(1, 50, sh.B), (0, 50, sh.B + sh.B * hi)])
        with pytest.raises(HalError, match="constraint identity"):
            verify_seal(r.seal, circuit="lookup")
        # v alone changed
        r = prove([(0, 50, 12345)])
        with pytest.raises(HalError, match="constraint identity"):
            verify_seal(r.seal, circuit="lookup")
        # what is not a record of the witness is a witgen error
        with pytest.raises(HalError, match="out of bounds"):
            prove([(1, sh.A, sh.B)])
        with pytest.raises(HalError, match="out of bounds"):
            prove([(3 * sh.V, 0, 1)])
        verify_seal(prove([]).seal, circuit="lookup")  # the prover is still good after the errors
    finally:
        srv.close()


# ---- the kept code commitment ----
def test_the_code_group_is_committed_once_and_the_seals_do_not_change():
    po2, widths = 12, (16, 32, 64)
    seals = {}
    for once in (1, 0):
        hal = HipHal(0)
        hal.set_tunable("code_commit_once", once)
        srv = _server(po2, widths, hal=hal)
        try:
            if once:  # before the first proof
                assert np.array_equal(srv.control_id(), lookup_control_id_host(po2, widths[0]))
            hal.profile_enable(True)
            seg = Segment(index=0, po2=po2, seed=21, noise_seed=4)
            seals[once] = [srv.prove_segment(seg).seal, srv.prove_segment(seg).seal]
            assert hal.profile_report().get("lookup_code", {"calls": 0})["calls"] == (0 if once else 2)
            hal.profile_enable(False)
        finally:
            srv.close()
            hal.close()
    assert np.array_equal(seals[1][0], seals[1][1]) and np.array_equal(seals[1][0], seals[0][0]) and np.array_equal(seals[0][0], seals[0][1])
    verify_seal(seals[1][0], circuit="lookup")


# ---- sha-256 ----
def test_a_sha256_lookup_seal_verifies_without_a_context_under_its_suite_only():
    srv = _server(10, (16, 32, 64), hashfn="sha-256")
    try:
        r = srv.prove_segment(Segment(index=0, po2=10, seed=3))
        assert np.array_equal(r.roots[0], lookup_control_id_host(10, 16, "sha-256"))
        verify_seal(r.seal, circuit="lookup", hashfn="sha-256")
        with pytest.raises(HalError):
            verify_seal(r.seal, circuit="lookup", hashfn="poseidon2")
        with pytest.raises(HalError):
            verify_seal(r.seal, hashfn="sha-256")  # not the synthetic circuit's
    finally:
        srv.close()
