"""CPU: the `sha-256` hash suite's host half (csrc/sha256_suite.hpp, control_id.cpp, verify.cpp) against an independent Python
restatement (tests/sha256_ref.py) and hashlib."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sha256_ref as ref  # noqa: E402

from boundless_amd.hal import HalError  # noqa: E402
from boundless_amd.prover import VerifierContext, synthetic_control_id_host, verify_seal  # noqa: E402
from oracle import oracle_lib as ol  # noqa: E402


def test_python_compression_reproduces_hashlib():
    rng = np.random.default_rng(5)
    lengths = sorted(set(list(range(0, 201, 7)) + [55, 56, 57, 63, 64, 65, 119, 120, 128]))
    for n in lengths:
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert ref.sha256(msg) == hashlib.sha256(msg).digest(), n


def test_numpy_pair_hash_equals_the_scalar_one():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 2**32, (33, 8), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2**32, (33, 8), dtype=np.uint64).astype(np.uint32)
    got = ref.pair_hash_np(a, b)
    for i in range(33):
        assert np.array_equal(got[i], ref.pair_hash(a[i], b[i]))


def python_control_id(po2, w_code):
    """The code group's LDE through the oracle's NTT functions (read-only use), rows hashed with hashlib, the tree with pair_hash."""
    L = ol.lib()
    n = 1 << po2
    cols = ref.code_columns(po2, w_code)
    x = np.ascontiguousarray(cols.reshape(-1))
    L.bxo_batch_interpolate_ntt(x, w_code, n)
    L.bxo_zk_shift(x, w_code, n)
    ev = np.zeros(4 * n * w_code, np.uint32)
    L.bxo_batch_expand_into_evaluate_ntt(ev, x, w_code, n, 2)
    leaves = ref.rows_hash(ev.reshape(w_code, 4 * n))
    return ref.merkle_nodes(leaves)[1]


@pytest.mark.parametrize("po2", [9, 10, 11, 12])
@pytest.mark.parametrize("w_code", [2, 3, 16])
def test_host_sha256_control_id_equals_pythons(po2, w_code):
    got = synthetic_control_id_host(po2, w_code, hashfn="sha-256")
    assert np.array_equal(got, python_control_id(po2, w_code))
    assert not np.array_equal(got, synthetic_control_id_host(po2, w_code))  # not the Poseidon2 ID
    assert np.array_equal(synthetic_control_id_host(po2, w_code, hashfn="poseidon2"), ol.control_id(po2, w_code))


def test_unknown_hashfn_names_are_refused():
    seal, _ = ol.prove_segment(9, 2, 4, 4, 7)
    verify_seal(seal, hashfn="poseidon2")
    for name in ("sha256", "SHA-256", "poseidon254", "blake2b", ""):
        with pytest.raises(HalError, match="unknown hashfn"):
            verify_seal(seal, hashfn=name)
        with pytest.raises(HalError, match="unknown hashfn"):
            synthetic_control_id_host(9, 2, hashfn=name)
        with pytest.raises(HalError, match="unknown hashfn"):
            VerifierContext().add_control_id(9, np.zeros(8, np.uint32), hashfn=name)


def test_a_poseidon2_seal_is_refused_as_sha256():
    seal, _ = ol.prove_segment(9, 2, 4, 4, 7)
    with pytest.raises(HalError):
        verify_seal(seal, hashfn="sha-256")


def test_sha256_control_ids_take_any_words_and_stay_apart_from_poseidon2_ones():
    ctx = VerifierContext()
    words = np.array([0xFFFFFFFF, 0, ref.P - 1, ref.P, 2**31, 1, 2, 3], np.uint32)
    ctx.add_control_id(9, words, hashfn="sha-256")
    with pytest.raises(HalError, match="canonical"):
        ctx.add_control_id(9, words)  # a Poseidon2 ID is field elements
    assert len(ctx) == 1
