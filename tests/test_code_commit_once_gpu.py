"""GPU: the code group's commitment is made once per prover (ctx tunable `code_commit_once`, default 1), not once per proof.

The code group of the built-in circuit is a function of the shape alone (include/bx_circuit.h), so a prover runs
witgen_code -> inverse NTT + zk shift -> 4x LDE -> hash_rows -> Merkle tree for it with its first proof (or its first control ID) and
keeps the device buffers and the fetched root + top layer; later proofs skip that work.  Nothing a caller can see may change:

* seals over a sequence of proofs on one prover are the CPU oracle's, word for word, with the switch on and off;
* the work is really gone (call counts of the profiled op `witgen_code`);
* an error drops the kept commitment and the next proof is right again;
* a plug-in circuit's code_group is still called for every proof;
* the submit/prove split and several provers on several threads behave the same.

Reference for `poseidon2`: oracle/ (oracle_lib.prove_segment, oracle_lib.control_id), exact equality.  The C oracle has no SHA-256
transcript, so for `sha-256` the reference is what tests/test_sha256_suite_gpu.py holds that suite to: the library's verifier, the
independent Python replay (tests/sha256_ref.py) and the host control ID (synthetic_control_id_host) — plus exact equality with the
seals of a prover that recommits the code group for every proof (`code_commit_once` = 0, the behaviour before this switch existed).
"""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sha256_ref  # noqa: E402

from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, synthetic_control_id_host, verify_seal  # noqa: E402
from oracle import oracle_lib as ol  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(10, (16, 8, 4)), (12, (3, 17, 5)), (16, (16, 8, 4))]
SEEDS = [11, 12, 13, 14, 15]


def _hal(hashfn, once):
    h = HipHal(0, hashfn=hashfn)
    if once is not None:
        h.set_tunable("code_commit_once", once)  # read by bx_prover_create
    return h


def _calls(hal, op):
    return hal.profile_report().get(op, {"calls": 0})["calls"]


@pytest.mark.parametrize("once", [None, 1, 0], ids=["default", "once", "every-proof"])
@pytest.mark.parametrize("po2,widths", SHAPES)
def test_poseidon2_seals_over_a_sequence_are_the_oracles(po2, widths, once):
    hal = _hal("poseidon2", once)
    srv = HipProverServer(0, po2=po2, widths=widths, hal=hal)
    try:
        cid = ol.control_id(po2, widths[0])
        for i, seed in enumerate(SEEDS):
            want, _ = ol.prove_segment(po2, *widths, seed)
            r = srv.prove_segment(Segment(index=i, po2=po2, seed=seed))
            assert np.array_equal(r.seal, want), (i, seed)
            assert np.array_equal(r.roots[0], cid) and np.array_equal(srv.control_id(), cid), (i, seed)
    finally:
        srv.close()
        hal.close()


@pytest.mark.parametrize("po2,widths", SHAPES)
def test_sha256_seals_over_a_sequence_are_those_of_a_prover_that_recommits(po2, widths):
    """sha-256 has no C oracle (module docstring): verifier + independent replay + host control ID, and equality with switch off."""
    cid = synthetic_control_id_host(po2, widths[0], hashfn="sha-256")
    seals = {}
    for once in (1, 0):
        hal = _hal("sha-256", once)
        srv = HipProverServer(0, po2=po2, widths=widths, hal=hal)
        try:
            seals[once] = []
            for i, seed in enumerate(SEEDS):
                r = srv.prove_segment(Segment(index=i, po2=po2, seed=seed))
                verify_seal(r.seal, hashfn="sha-256")
                sha256_ref.replay_seal(r.seal)
                assert np.array_equal(r.roots[0], cid) and np.array_equal(srv.control_id(), cid), (once, i)
                seals[once].append(r.seal)
        finally:
            srv.close()
            hal.close()
    for a, b in zip(seals[1], seals[0]):
        assert np.array_equal(a, b)
    assert not np.array_equal(seals[1][0], seals[1][1])  # different seeds, different seals


@pytest.mark.parametrize("once,control_id_first", [(1, False), (1, True), (0, False)])
def test_the_code_group_is_generated_once_per_prover(once, control_id_first):
    po2, widths, M = 12, (16, 8, 4), 4
    hal = _hal("poseidon2", once)
    srv = HipProverServer(0, po2=po2, widths=widths, hal=hal)
    try:
        hal.profile_reset()
        hal.profile_enable(True)
        if control_id_first:  # what an agent lane does when it creates a buffer set: its first proof is already a steady-state proof
            srv.control_id()
            assert _calls(hal, "witgen_code") == 1
        for i in range(M + 1):  # one warm proof and M more
            srv.prove_segment(Segment(index=i, po2=po2, seed=50 + i))
        hal.profile_enable(False)
        assert _calls(hal, "witgen_code") == (1 if once else M + 1)
        if once:
            hal.profile_enable(True)
            before = hal.profile_report()
            assert np.array_equal(srv.control_id(), ol.control_id(po2, widths[0]))
            hal.profile_enable(False)
            after = hal.profile_report()
            assert {k: v["calls"] for k, v in after.items()} == {k: v["calls"] for k, v in before.items()}  # nothing was launched
    finally:
        srv.close()
        hal.close()


def test_errors_drop_the_kept_commitment_and_the_next_proof_is_right():
    po2, widths = 10, (4, 8, 4)
    hal = _hal("poseidon2", None)
    srv = HipProverServer(0, po2=po2, widths=widths, hal=hal)
    try:
        good = Segment(index=0, po2=po2, seed=5).to_bytes()
        want, _ = ol.prove_segment(po2, *widths, 5)
        for warm in (False, True):  # on a prover that holds no commitment yet, then on one that does
            with pytest.raises(HalError, match="Failed to deserialize segment data"):
                srv.prove_segment_bytes(good[:27])
            with pytest.raises(HalError, match="not a synthetic segment blob"):
                srv.prove_segment_bytes(b"\x00" * 64)
            with pytest.raises(HalError, match="po2 11"):
                srv.prove_segment_bytes(Segment(index=0, po2=11, seed=5).to_bytes())
            with pytest.raises(HalError, match="empty segment"):
                srv.prove_segment_bytes(b"")
            with pytest.raises(HalError, match="no segment was submitted"):
                srv.prove_submitted()
            assert np.array_equal(srv.prove_segment_bytes(good).seal, want), warm
        # an error after the prologue (witgen refuses the blob's po2) is followed by a proof that commits the code group again ...
        hal.profile_reset()
        hal.profile_enable(True)
        with pytest.raises(HalError, match="po2 11"):
            srv.prove_segment_bytes(Segment(index=0, po2=11, seed=6).to_bytes())
        for seed in (6, 7):  # ... and by one that does not
            r = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
            assert np.array_equal(r.seal, ol.prove_segment(po2, *widths, seed)[0]), seed
            assert np.array_equal(r.roots[0], ol.control_id(po2, widths[0]))
        hal.profile_enable(False)
        assert _calls(hal, "witgen_code") == 1
    finally:
        srv.close()
        hal.close()


def test_a_plugin_circuit_still_commits_its_code_group_for_every_proof():
    from test_circuit_plugin_gpu import SquareCircuit

    from boundless_amd.circuit import CircuitOps
    from boundless_amd.hal import load_library

    lib = load_library()
    po2, widths = 10, (2, 3, 2)
    circ = SquareCircuit(lib)
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, b"square-plus-back")
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        assert circ.calls == ["code_group"]
        circ.calls.clear()
        a = srv.prove_segment(Segment(index=0, po2=po2, seed=77))
        b = srv.prove_segment(Segment(index=1, po2=po2, seed=78))
        assert circ.calls == ["code_group", "witgen", "accumulate", "eval_check"] * 2
        assert np.array_equal(a.roots[0], b.roots[0]) and not np.array_equal(a.seal, b.seal)
        verify_seal(a.seal, circuit=ops, ctx=vctx)
        verify_seal(b.seal, circuit=ops, ctx=vctx)
        srv.control_id()
        assert circ.calls.count("code_group") == 3
    finally:
        srv.close()


def test_two_deep_staging_on_a_prover_that_holds_its_commitment():
    po2, widths = 12, (4, 8, 4)
    hal = _hal("poseidon2", None)
    srv = HipProverServer(0, po2=po2, widths=widths, hal=hal)
    try:
        assert np.array_equal(srv.control_id(), ol.control_id(po2, widths[0]))  # the state is valid from here on
        seeds = [100 + i for i in range(6)]
        want = [ol.prove_segment(po2, *widths, s)[0] for s in seeds]
        pad = bytes(1 << 20)
        blobs = [Segment(index=i, po2=po2, seed=s, payload=pad).to_bytes() for i, s in enumerate(seeds)]
        srv.submit_segment(blobs[0])
        srv.submit_segment(blobs[1])
        with pytest.raises(HalError, match="staging slots busy"):
            srv.submit_segment(blobs[2])
        with pytest.raises(HalError, match="still outstanding"):  # an error: drops the commitment, the next proof redoes it
            srv.prove_segment_bytes(blobs[2])
        got, errors = [], []
        slots = threading.Semaphore(0)  # a slot frees each time a proof returns

        def feeder():
            try:
                for b in blobs[2:]:
                    slots.acquire()
                    srv.submit_segment(b)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        t = threading.Thread(target=feeder)
        t.start()
        for i in range(len(blobs)):
            got.append(srv.prove_submitted(index=i).seal)
            slots.release()
        t.join()
        assert not errors
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        # both entry points on the same prover, interleaved
        assert np.array_equal(srv.prove_segment_bytes(blobs[3]).seal, want[3])
        srv.submit_segment(blobs[4])
        assert np.array_equal(srv.prove_submitted().seal, want[4])
    finally:
        srv.close()
        hal.close()


def test_three_provers_on_three_threads():
    po2, widths, lanes, per_lane = 12, (16, 8, 4), 3, 4
    want = {s: ol.prove_segment(po2, *widths, s)[0] for s in range(300, 300 + lanes * per_lane)}
    hals = [_hal("poseidon2", None) for _ in range(lanes)]
    servers = [HipProverServer(0, po2=po2, widths=widths, hal=h) for h in hals]
    got, errors = {}, []

    def lane(k):
        try:
            for j in range(per_lane):
                seed = 300 + k * per_lane + j
                got[seed] = servers[k].prove_segment(Segment(index=j, po2=po2, seed=seed)).seal
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    try:
        threads = [threading.Thread(target=lane, args=(k,)) for k in range(lanes)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert sorted(got) == sorted(want)
        for s in want:
            assert np.array_equal(got[s], want[s]), s
    finally:
        for sv in servers:
            sv.close()
        for h in hals:
            h.close()
