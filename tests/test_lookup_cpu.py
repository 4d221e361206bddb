"""CPU: the lookup circuit (include/bx_lookup.h) — the reference of tests/lookup_ref.py stands on its own feet, and the host half
of the library's table (normalize, taps, n_globals, constraints_at, check_code, the host control IDs) agrees with it.

The reference alone: on an honest trace every constraint vanishes on every row (noise rows included) and the running sums close;
a limb moved out of the table (with its value patched to match) breaks the closing constraint and nothing else; a value changed
alone breaks its decomposition constraint and nothing else.  The library: `constraints_at` through ctypes with a Python tap reader
equals the reference's polynomial on random tap values; the control IDs equal the definition-level commitment (the oracle's NTT
and Poseidon2 for "poseidon2", tests/sha256_ref.py for "sha-256").  Payload decoding is checked here for the reference alone; the
library's own messages come out of witgen, which needs a ctx, and are checked by message in tests/test_lookup_gpu.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logup_ref as lr  # noqa: E402
import lookup_ref as ref  # noqa: E402
import sha256_ref  # noqa: E402

from boundless_amd.circuit import MAX_TAPS, TapReader, _TAP_AT, encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402
from boundless_amd.prover import SegmentParams, lookup_control_id_host, synthetic_control_id_host  # noqa: E402
from oracle import oracle_lib as ol  # noqa: E402

P = ref.P
ALPHA = [lr.encode(v) for v in (123456789, 987654321, 55555, 1234567)]


def ops():
    return lookup_circuit().contents


def honest(po2=9, widths=(3, 4, 12), seed=7, records=()):
    sh = ref.Shape(po2, *widths)
    code = ref.code_columns(sh)
    data, g = ref.data_columns(sh, seed, records=records)
    accum = ref.accum_columns(sh, seed, code, data, ALPHA)
    return sh, code, data, accum, g


def nonzero(sh, code, data, accum, g):
    """{(constraint index, row)} of the constraints that do not vanish"""
    bad = set()
    for r in range(sh.N):
        for i, c in enumerate(ref.row_constraints(sh, code, data, accum, ALPHA, g, r)):
            if any(c):
                bad.add((i, r))
    return bad


# ---- the reference alone ----
@pytest.mark.parametrize("widths", [(3, 4, 12), (5, 11, 30)])
def test_every_constraint_vanishes_on_every_row_of_an_honest_trace(widths):
    sh, code, data, accum, g = honest(9, widths)
    assert sh.B == 256 and sh.A == 384 and sh.V == (1 if widths[1] == 4 else 3)
    assert nonzero(sh, code, data, accum, g) == set()
    total = np.zeros(4, np.uint64)
    for s in range(sh.S):
        total += accum[4 * s:4 * s + 4, sh.A - 1].astype(np.uint64)
    assert not (total % P).any()  # sum_s S_s(A - 1) = 0
    # the multiplicities count every limb of the active rows once
    assert sum(lr.decode(int(w)) for w in data[3 * sh.V][:sh.B]) == 2 * sh.V * sh.A


def test_a_limb_outside_the_table_breaks_the_closing_constraint_alone():
    sh = ref.Shape(9, 3, 4, 12)
    row = 100
    _, _, data0, _, _ = honest()
    hi = lr.decode(int(data0[2][row]))
    recs = [(1, row, sh.B), (0, row, sh.B + sh.B * hi)]  # lo = B, v patched to match
    sh, code, data, accum, g = honest(records=recs)
    assert nonzero(sh, code, data, accum, g) == {(3 * sh.V + 1, sh.A - 1)}


def test_a_value_changed_alone_breaks_its_decomposition_alone():
    row = 200
    sh, code, data, accum, g = honest(records=[(0, row, 5)])
    assert nonzero(sh, code, data, accum, g) == {(0, row)}


# ---- constraints_at of the library's table against the reference's polynomial ----
@pytest.mark.parametrize("widths", [(3, 4, 12), (16, 32, 64), (3, 32, 64), (16, 4, 12)])
def test_constraints_at_equals_the_reference_on_random_taps(widths):
    sh = ref.Shape(12, *widths)
    assert sh.V in (1, 7)
    rng = np.random.default_rng(widths[0] * 100 + widths[1])
    vals = {}

    def tap_value(g, c, back):
        assert back in ref.taps(sh, g, c)
        return vals.setdefault((g, c, back), [int(v) for v in rng.integers(0, P, 4)])

    def at(_ctx, g, c, back, out):
        for k, v in enumerate(tap_value(g, c, back)):
            out[k] = lr.encode(v)
        return None

    reader = TapReader(None, _TAP_AT(at))
    shape = SegmentParams(12, *widths, 0, 0)
    pm, alpha, gl = ([int(v) for v in rng.integers(0, P, 4)] for _ in range(3))
    words = lambda v: (C.c_uint32 * len(v))(*[lr.encode(x) for x in v])
    out = (C.c_uint32 * 4)()
    msg = ops().constraints_at(None, C.byref(shape), C.byref(reader), words(pm), words(alpha), words(gl[:2]), out)
    assert not msg
    want = ref.mixed(sh, tap_value, pm, alpha, gl[:2])
    assert [lr.decode(int(w)) for w in out] == want
    assert len(vals) == 3 + 3 * sh.V + 1 + 8 * sh.S  # every tap the text names and no other


# ---- shape handling ----
@pytest.mark.parametrize("shape", [(9, 3, 4, 12), (12, 16, 32, 64), (12, 16, 32, 30), (17, 3, 7, 20), (20, 16, 256, 64), (24, 3, 190, 508),
                                   (12, 3, 3, 12), (12, 3, 4, 11), (12, 2, 4, 12), (12, 3, 193, 516), (12, 3, 4, 12, 1, 0), (12, 3, 4, 12, 0, 4),
                                   (8, 3, 4, 12)])
def test_normalize_taps_and_globals_follow_the_reference(shape):
    want = ref.normalize(*shape)
    prm = SegmentParams(*(list(shape) + [0, 0])[:6])
    msg = ops().normalize(None, C.byref(prm))
    assert (msg is None) == (want is None), (shape, want, C.cast(msg, C.c_char_p).value if msg else None)
    if want is not None:
        return
    assert (prm.cons_terms, prm.cons_degree) == (0, 0)  # 0 stays 0
    sh = ref.Shape(*shape[:4])
    assert ops().n_globals(None, C.byref(prm)) == ref.n_globals(sh) == 2
    backs = (C.c_uint32 * MAX_TAPS)()
    for g, width in enumerate(shape[1:4]):
        for c in range(width):
            k = ops().taps(None, C.byref(prm), g, c, backs)
            assert list(backs[:k]) == ref.taps(sh, g, c), (g, c)


def test_a_w_accum_that_is_no_multiple_of_4_leaves_filler_columns():
    sh = ref.Shape(12, 16, 32, 30)
    assert (sh.V, sh.S) == (3, 7)  # floor(30 / 4) = 7 ext slots
    assert ref.taps(sh, 2, 27) == [0, 1] and ref.taps(sh, 2, 28) == [0] and ref.taps(sh, 2, 29) == [0]


# ---- control IDs ----
def definition_level_id(po2, w_code, hashfn):
    """code columns -> interpolate -> coset shift -> 4x evaluation (the oracle's NTTs) -> row hashes -> tree"""
    L = ol.lib()
    n = 1 << po2
    x = np.ascontiguousarray(ref.code_columns(ref.Shape(po2, w_code, 4, 12)).reshape(-1))
    L.bxo_batch_interpolate_ntt(x, w_code, n)
    L.bxo_zk_shift(x, w_code, n)
    ev = np.zeros(4 * n * w_code, np.uint32)
    L.bxo_batch_expand_into_evaluate_ntt(ev, x, w_code, n, 2)
    if hashfn == "sha-256":
        return sha256_ref.merkle_nodes(sha256_ref.rows_hash(ev.reshape(w_code, 4 * n)))[1]
    nodes = np.zeros(16 * 4 * n, np.uint32)
    leaves = np.zeros(8 * 4 * n, np.uint32)
    L.bxo_hash_rows(leaves, ev, 4 * n, w_code)
    nodes[8 * 4 * n:] = leaves
    size = 4 * n
    while size > 1:
        L.bxo_hash_fold(nodes, size, size // 2)
        size //= 2
    return nodes[8:16].copy()


@pytest.mark.parametrize("hashfn", ["poseidon2", "sha-256"])
@pytest.mark.parametrize("po2,w_code", [(9, 3), (10, 16)])
def test_host_control_id_equals_the_definition_level_commitment(po2, w_code, hashfn):
    got = lookup_control_id_host(po2, w_code, hashfn)
    assert np.array_equal(got, definition_level_id(po2, w_code, hashfn))
    assert not np.array_equal(got, synthetic_control_id_host(po2, w_code, hashfn))  # its own seed: never the synthetic circuit's ID
    assert np.array_equal(got, lookup_control_id_host(po2, w_code, hashfn))  # cached


def test_check_code_accepts_the_id_and_refuses_its_neighbour():
    prm = SegmentParams(9, 3, 4, 12, 0, 0)
    cid = lookup_control_id_host(9, 3)
    assert not ops().check_code(None, C.byref(prm), cid.ctypes.data_as(C.POINTER(C.c_uint32)))
    bad = cid.copy()
    bad[0] = (int(bad[0]) + 1) % P
    msg = ops().check_code(None, C.byref(prm), bad.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert msg and b"control ID" in C.cast(msg, C.c_char_p).value


def test_an_unknown_suite_name_is_refused():
    with pytest.raises(HalError, match="unknown hashfn"):
        lookup_control_id_host(9, 3, "blake2b")
    with pytest.raises(HalError, match="w_code >= 3"):
        lookup_control_id_host(9, 2)


# ---- the payload ----
def test_payload_decoding_errors_of_the_reference():
    """The REFERENCE's decoder only: the library decodes a payload inside witgen, which needs a ctx, so its messages are checked in
    tests/test_lookup_gpu.py (test_witgen_refuses_bad_payloads_by_message)."""
    sh = ref.Shape(12, 16, 32, 64)
    assert ref.decode_records(encode_cell_records([(0, 0, 5), (20, sh.A - 1, P - 1)]), sh) == [(0, 0, 5), (20, sh.A - 1, P - 1)]
    with pytest.raises(ValueError, match="whole number"):
        ref.decode_records(b"\0" * 13, sh)
    for rec in [(3 * sh.V, 0, 0), (0, sh.A, 0), (0, 0, P)]:  # the multiplicity column, a noise row, a non-canonical value
        with pytest.raises(ValueError, match="out of bounds"):
            ref.decode_records(encode_cell_records([rec]), sh)
