"""GPU parity of the whole segment-prover pipeline: the HIP prover's seal must equal the CPU oracle's, word for word."""
import numpy as np
import pytest

from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("po2,widths,seed", [
    (9, (1, 1, 1), 1),
    (10, (4, 8, 4), 1234),
    (12, (3, 17, 5), 0xB0D1E550000),
    (13, (16, 32, 8), 77),
    (15, (2, 5, 3), 99),  # smallest size that keeps the trace coefficients bit-reversed through the DEEP phase
    (16, (4, 12, 4), 0xB0D1E550001),
])
def test_seal_bit_exact_vs_oracle(po2, widths, seed):
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=po2, widths=widths)
    try:
        receipt = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
        seal, roots = ol.prove_segment(po2, *widths, seed)
        assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
        assert receipt.seal.size == seal.size
        bad = np.nonzero(receipt.seal != seal)[0]
        assert bad.size == 0, f"first differing seal word at {bad[:5]}"
        receipt.verify_integrity()  # prove.rs:53-55
        # same prover object, next segment (buffers are reused): still exact, and different from the first
        r2 = srv.prove_segment(Segment(index=1, po2=po2, seed=seed + 1))
        s2, _ = ol.prove_segment(po2, *widths, seed + 1)
        assert np.array_equal(r2.seal, s2) and not np.array_equal(r2.seal, receipt.seal)
    finally:
        srv.close()


@pytest.mark.parametrize("po2,widths,knobs,seed", [
    (21, (4, 16, 8), (0, 0), 21),      # compose.yml:67 runs segment_po2 = 21: 2^23-point LDEs
    (14, (16, 64, 16), (16, 3), 3),    # another compile-time circuit shape
    (13, (5, 33, 9), (5, 2), 8),       # knobs without a specialisation: the run-time path of cons_sum
    (12, (3, 10, 4), (64, 5), 9),      # the highest constraint degree the check polynomial admits
    (11, (2, 7, 12), (1, 1), 4),       # degenerate: every derived cell is one pool entry; three accumulators, one pair
    (10, (2, 2, 4), (0, 0), 5),        # one free and one derived data column: the pool wraps around the free columns
    (9, (3, 3, 8), (7, 3), 6),         # more accumulators than free columns allow pairs for
    (10, (40, 6, 16), (0, 0), 7),      # wide code group, narrow data group
    (22, (2, 6, 4), (0, 0), 22),       # 2^24-point LDEs
    (23, (2, 6, 4), (0, 0), 23),       # 2^25-point LDEs: pass B of the NTT at 2^13 rows (the oracle needs about a minute here)
])
def test_seal_bit_exact_vs_oracle_other_sizes_and_circuit_knobs(po2, widths, knobs, seed):
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=po2, widths=widths, terms=knobs[0], degree=knobs[1])
    try:
        receipt = srv.prove_segment(Segment(index=0, po2=po2, seed=seed))
    finally:
        srv.close()
    seal, roots = ol.prove_segment(po2, *widths, seed, terms=knobs[0], degree=knobs[1])
    assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
    assert np.array_equal(receipt.seal, seal)
    receipt.verify_integrity()


def _random_shapes(n, rng_seed):
    rng = np.random.default_rng(rng_seed)
    out = []
    for i in range(n):
        po2 = int(rng.integers(9, 15))
        widths = (int(rng.integers(1, 24)), int(rng.integers(1, 48)), int(rng.integers(1, 14)))
        knobs = (int(rng.integers(1, 65)), int(rng.integers(1, 6)))
        out.append((po2, widths, knobs, int(rng.integers(0, 2**63))))
    return out


@pytest.mark.parametrize("po2,widths,knobs,seed", _random_shapes(32, 20260927))
def test_seal_bit_exact_vs_oracle_on_random_shapes(po2, widths, knobs, seed):
    """A seeded sweep over shapes nobody chose by hand (widths that are not multiples of anything, every degree, term counts
    off the compile-time specialisations, 63-bit seeds): the seal and the roots equal the oracle's and verify."""
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=po2, widths=widths, terms=knobs[0], degree=knobs[1])
    try:
        receipt = srv.prove_segment(Segment(index=3, po2=po2, seed=seed))
    finally:
        srv.close()
    seal, roots = ol.prove_segment(po2, *widths, seed, terms=knobs[0], degree=knobs[1])
    assert np.array_equal(receipt.roots, roots), "Merkle roots differ"
    bad = np.nonzero(receipt.seal != seal)[0] if receipt.seal.size == seal.size else [-1]
    assert len(bad) == 0, f"seal differs from the oracle's at {bad[:5]} for po2={po2} widths={widths} knobs={knobs}"
    receipt.verify_integrity()


def test_the_largest_segment_at_full_width_is_one_proof_on_one_gpu():
    """po2 = 24 — risc0's largest segment, 16 M cycles — at the BASELINE widths 16/256/64: 135 GB of buffers, which is what
    288 GB of HBM is for (the reference's CUDA targets top out at 24-80 GB and split such work into smaller segments).  The CPU
    oracle would need ten minutes and as much host memory, so here the checks are the size-independent ones: the proof is
    deterministic, the CPU verifier accepts it (every Merkle opening, the constraint identity, the DEEP quotients and the FRI
    chain of a 2^26-row domain: any 32-bit index overflow in a kernel would break one of them) and rejects a flipped word."""
    import torch

    from boundless_amd.hal import HalError
    from boundless_amd.prover import HipProverServer, Segment, verify_seal

    free, _ = torch.cuda.mem_get_info(0)
    if free < 150 * 2**30:
        pytest.skip("needs 135 GB of free HBM")
    srv = HipProverServer(0, po2=24)
    try:
        a = srv.prove_segment(Segment.synthetic(0, po2=24)).seal
        b = srv.prove_segment(Segment.synthetic(0, po2=24)).seal
        c = srv.prove_segment(Segment.synthetic(1, po2=24)).seal
    finally:
        srv.close()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a[:6].tolist() == [24, 16, 256, 64, 64, 4]
    verify_seal(a)
    verify_seal(c)
    bad = a.copy()
    bad[a.size // 2] ^= 4
    with pytest.raises(HalError):
        verify_seal(bad)
    with pytest.raises(HalError, match=r"po2 must be in \[9, 24\]"):
        HipProverServer(0, po2=25, widths=(2, 2, 2))


def test_deep_phase_in_natural_and_in_bit_reversed_order_give_the_same_seal():
    """`deep_bitrev` = 0 runs upstream's order (bit-reverse every coefficient column, evaluate, mix); the default keeps the
    trace coefficients bit-reversed and reverses only the two combination polynomials.  Same seal either way."""
    from boundless_amd.hal import HipHal
    from boundless_amd.prover import HipProverServer, Segment

    seals = []
    for flag in (0, 1):
        hal = HipHal(0)
        hal._check(hal.lib.bx_set_tunable(hal.ctx, b"deep_bitrev", flag))
        srv = HipProverServer(0, po2=16, widths=(3, 9, 4), hal=hal)
        try:
            seals.append(srv.prove_segment(Segment(0, 16, 4242)).seal)
        finally:
            srv.close()
    assert np.array_equal(seals[0], seals[1])
    want, _ = ol.prove_segment(16, 3, 9, 4, 4242)
    assert np.array_equal(seals[1], want)


@pytest.mark.parametrize("po2", [10, 13, 17])
def test_challenges_drawn_on_the_device_give_the_seal_of_the_host_transcript(po2):
    """`dev_draws` = 1: the FRI challenges (which depend only on a Merkle root) are drawn by the device half of the transcript and the
    host replays them from one late read-back; 0 (default): every draw waits for its root on the host.  Same seal, equal to the oracle's
    (po2 10 has a single FRI round, 17 three)."""
    from boundless_amd.hal import HipHal
    from boundless_amd.prover import HipProverServer, Segment

    seals = []
    for flag in (0, 1):
        hal = HipHal(0)
        hal.set_tunable("dev_draws", flag)
        srv = HipProverServer(0, po2=po2, widths=(3, 9, 4), hal=hal)
        try:
            seals.append(srv.prove_segment(Segment(0, po2, 1717)).seal)
            seals.append(srv.prove_segment(Segment(1, po2, 1718)).seal)  # the device state is re-seeded by every proof
        finally:
            srv.close()
    assert np.array_equal(seals[0], seals[2]) and np.array_equal(seals[1], seals[3])
    want, _ = ol.prove_segment(po2, 3, 9, 4, 1717)
    assert np.array_equal(seals[2], want)


def test_roctx_ranges_do_not_change_the_seal():
    """bx_trace_enable: ranges only (1) and ranges + a stream drain per stage (2) give the seal of the untraced run."""
    from boundless_amd import hal as H
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=13, widths=(3, 9, 4))
    try:
        seals = []
        for level in (0, 1, 2):
            H.trace_enable(level)
            seals.append(srv.prove_segment(Segment(0, 13, 99)).seal)
    finally:
        H.trace_enable(0)
        srv.close()
    assert np.array_equal(seals[0], seals[1]) and np.array_equal(seals[0], seals[2])
    want, _ = ol.prove_segment(13, 3, 9, 4, 99)
    assert np.array_equal(seals[0], want)


def test_seal_is_deterministic_and_shape_errors():
    from boundless_amd.hal import HalError
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=11, widths=(2, 6, 2))
    try:
        a = srv.prove_segment(Segment(0, 11, 5)).seal
        b = srv.prove_segment(Segment(0, 11, 5)).seal
        assert np.array_equal(a, b)
        with pytest.raises(HalError):
            srv.prove_segment(Segment(0, 12, 5))
    finally:
        srv.close()
    with pytest.raises(HalError):
        HipProverServer(0, po2=5)


@pytest.mark.parametrize("po2,widths", [(9, (1, 1, 1)), (10, (2, 5, 8))])
def test_seal_words_is_the_size_of_the_seal_at_small_shapes(po2, widths):
    """bx_prover_seal_words is the layout's exact length (csrc/seal_layout.hpp), not a bound: the narrowest shape, and one whose data
    group has a column with three tap rows."""
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=po2, widths=widths)
    try:
        r = srv.prove_segment(Segment(index=0, po2=po2, seed=11))
        assert r.seal.size == srv.lib.bx_prover_seal_words(srv.handle)
        assert r.seal.size == ol.prove_segment(po2, *widths, 11)[0].size
    finally:
        srv.close()


@pytest.mark.parametrize("po2", [18, 20])
def test_full_size_properties(po2):
    """BASELINE shape (2^20 cycles, widths 16/256/64): the DEEP quotients divide exactly (checked inside the prover),
    the seal has the documented length and the trace roots match the oracle's Merkle roots of a small column subset."""
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=po2)
    try:
        r = srv.prove_segment(Segment.synthetic(0, po2))
        n_rounds = 0
        s = 1 << po2
        while s > 256:
            s //= 16
            n_rounds += 1
        assert r.seal[:4].tolist() == [po2, 16, 256, 64]
        r.verify_integrity()  # the full-size seal is accepted by the CPU verifier
        assert r.seal.size == srv.lib.bx_prover_seal_words(srv.handle)
        r2 = srv.prove_segment(Segment.synthetic(0, po2))
        assert np.array_equal(r.seal, r2.seal)
    finally:
        srv.close()


def test_agent_feed_loop_with_the_hip_prover():
    """tasks/prove.rs flow end to end through the native agent (bx_agent_poll_work) with two prover lanes on the GPU:
    segment blob in the hot store -> prove -> verify -> receipt stored -> segment unlinked -> task done."""
    from boundless_amd import agent as ag
    from boundless_amd.prover import Segment, verify_seal

    a = ag.Agent(prover=None, device=0, inflight=2, widths=(4, 12, 4), poll_time=0.01)
    try:
        n = 6
        for i in range(n):
            a.store.set_key_with_expiry(f"job:J:segments:{i}", ag.serialize_segment(Segment.synthetic(i, po2=12)), 600)
            a.taskdb.create_task("J", f"prove-{i}", {"Prove": {"index": i}})
        assert a.poll_work(max_idle_polls=2) == n
        assert a.store.keys() == [f"job:J:synthetic_receipts:prove-{i}" for i in range(n)]
        for i in range(n):
            rec = ag.deserialize_receipt(a.store.get(f"job:J:synthetic_receipts:prove-{i}"))
            assert rec.index == i and rec.po2 == 12
            verify_seal(rec.seal)
            want, _ = ol.prove_segment(12, 4, 12, 4, Segment.synthetic(i, po2=12).seed)
            assert np.array_equal(rec.seal, want)
        assert a.taskdb.count("done") == n
        assert f'task_operations_total{{task_name="prove",operation_type="complete",status="success"}} {n}' in a.metrics_text()
        # a second segment size on the same agent allocates a second prover per lane, lazily
        a.store.set_key_with_expiry("job:K:segments:0", ag.serialize_segment(Segment.synthetic(0, po2=10)), 600)
        a.taskdb.create_task("K", "p", {"Prove": {"index": 0}})
        assert a.poll_work(max_idle_polls=2) == 1
        rec = ag.deserialize_receipt(a.store.get("job:K:synthetic_receipts:p"))
        want, _ = ol.prove_segment(10, 4, 12, 4, Segment.synthetic(0, po2=10).seed)
        assert np.array_equal(rec.seal, want)
    finally:
        a.close()


def test_one_native_agent_over_two_device_slots_steals_work_and_stays_bit_exact():
    """bx_agent_config.n_devices on real hardware: one agent process, two "devices" (this box has one GPU, so both slots are
    ordinal 0: two independent sets of lanes, contexts and provers), 2 lanes each, all four lanes claiming from the one task db.
    BASELINE configs[2] (a batch work-stolen across the GPUs of a node) through the native queue; every seal must equal the
    oracle's and every task must be done exactly once."""
    from boundless_amd import agent as ag
    from boundless_amd.prover import Segment, verify_seal

    po2, widths, n = 12, (4, 12, 4), 16
    a = ag.Agent(prover=None, devices=[0, 0], inflight=2, widths=widths, poll_time=0.005)
    try:
        for i in range(n):
            a.store.set_key_with_expiry(f"job:B:segments:{i}", ag.serialize_segment(Segment.synthetic(i, po2=po2)), 600)
            a.taskdb.create_task("B", f"prove-{i}", {"Prove": {"index": i}})
        assert a.poll_work(max_idle_polls=3) == n
        stats = a.lane_stats()
        assert [d for d, _ in stats] == [0, 0, 0, 0] and sum(k for _, k in stats) == n
        assert sum(k for _, k in stats[:2]) > 0 and sum(k for _, k in stats[2:]) > 0, stats  # both device slots got work
        assert a.taskdb.count("done") == n
        for i in range(n):
            rec = ag.deserialize_receipt(a.store.get(f"job:B:synthetic_receipts:prove-{i}"))
            want, _ = ol.prove_segment(po2, *widths, Segment.synthetic(i, po2=po2).seed)
            assert rec.index == i and np.array_equal(rec.seal, want), f"segment {i}"
            verify_seal(rec.seal)
    finally:
        a.close()


def test_hip_prover_as_a_rest_worker_of_a_bento_api():
    """The native agent with the HIP prover as a worker of a next-gen Bento API (include/bx_rest.h): claims over
    POST /worker/gpu/tasks/claim/prove, fetches segments over GET /worker/hot/..., proves on the GPU, verifies, PUTs the
    receipts, DELETEs the segments and reports done — against the local stub of the API's worker routes."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rest_stub_server import StubServer

    from boundless_amd import agent as ag
    from boundless_amd.prover import Segment, verify_seal

    job, po2, widths, n = "0b1e55ed-0000-4000-8000-0000000000aa", 12, (4, 12, 4), 6
    srv = StubServer()
    w = ag.RestWorker(srv.url, claim_wait_secs=0)
    a = ag.Agent(prover=None, device=0, inflight=2, widths=widths, poll_time=0.01, store=w.store, taskdb=w.taskdb)
    try:
        for i in range(n):
            srv.state.hot[f"job:{job}:segments:{i}"] = (ag.serialize_segment(Segment.synthetic(i, po2=po2)), None)
            srv.state.create_task("prove", job, f"prove-{i}", {"Prove": {"index": i}}, max_retries=1)
        assert a.poll_work(max_idle_polls=2) == n
        assert [t["state"] for t in srv.state.tasks] == ["done"] * n
        assert sorted(srv.state.hot) == sorted(f"job:{job}:synthetic_receipts:prove-{i}" for i in range(n))
        for i in range(n):
            rec = ag.deserialize_receipt(srv.state.hot[f"job:{job}:synthetic_receipts:prove-{i}"][0])
            want, _ = ol.prove_segment(po2, *widths, Segment.synthetic(i, po2=po2).seed)
            assert np.array_equal(rec.seal, want)
            verify_seal(rec.seal)
    finally:
        a.close()
        w.close()
        srv.close()


def test_agent_bounds_the_shapes_it_caches_and_reports_create_errors():
    """Round-1 advisor finding: po2 came unvalidated from the blob, every distinct value allocated a buffer set per lane for
    good, and a failed allocation surfaced as "no prover".  Sizes outside [po2_min, po2_max] now fail the task with the reason,
    at most max_shapes buffer sets are cached per lane (least recently used evicted), and create errors are passed through."""
    from boundless_amd import agent as ag
    from boundless_amd.prover import Segment

    a = ag.Agent(prover=None, device=0, inflight=1, widths=(2, 6, 2), poll_time=0.005, po2_range=(9, 12), max_shapes=2)
    try:
        order = [10, 11, 12, 10, 9, 13, 8]
        for k, po2 in enumerate(order):
            a.store.set_key_with_expiry(f"job:S:segments:{k}", ag.serialize_segment(Segment.synthetic(k, po2=po2)), 600)
            a.taskdb.create_task("S", f"t{k}", {"Prove": {"index": k}})
        assert a.poll_work(max_idle_polls=2) == 5
        for k, po2 in enumerate(order):
            row = a.taskdb.task("S", f"t{k}")
            if 9 <= po2 <= 12:
                assert row.state == "done", (po2, row.error)
                rec = ag.deserialize_receipt(a.store.get(f"job:S:synthetic_receipts:t{k}"))
                want, _ = ol.prove_segment(po2, 2, 6, 2, Segment.synthetic(k, po2=po2).seed)
                assert np.array_equal(rec.seal, want)  # still exact after evictions and re-creations
            else:
                assert row.state == "failed" and "outside the sizes this agent accepts [9, 12]" in row.error, row.error
    finally:
        a.close()


def test_plain_c_consumer_of_the_abi(tmp_path):
    """Build tests/c_abi_smoke.c with gcc, link it against the in-tree library and run it on the GPU."""
    import os
    import subprocess

    from boundless_amd.hal import LIB_PATH

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_smoke")
    libdir = os.path.dirname(LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-O1", f"-I{os.path.join(root, 'include')}", os.path.join(root, "tests", "c_abi_smoke.c"),
                        f"-L{libdir}", "-lbx_hip_hal", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "c_abi_smoke ok" in r.stdout


def test_three_provers_in_flight_on_one_gpu_stay_bit_exact():
    """bench.py keeps 3 segments in flight per GPU (one prover + stream + host thread each): concurrent provers must not
    disturb each other (tables, scratch and streams are per ctx)."""
    import threading

    from boundless_amd.prover import HipProverServer, Segment

    po2, widths = 12, (4, 12, 4)
    servers = [HipProverServer(0, po2=po2, widths=widths) for _ in range(3)]
    results = {}

    def work(k):
        for j in range(3):
            seg = Segment.synthetic(index=3 * k + j, po2=po2)
            results[seg.index] = servers[k].prove_segment(seg).seal

    try:
        ts = [threading.Thread(target=work, args=(k,)) for k in range(3)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert sorted(results) == list(range(9))
        for idx, seal in results.items():
            want, _ = ol.prove_segment(po2, *widths, Segment.synthetic(idx, po2=po2).seed)
            assert np.array_equal(seal, want), f"segment {idx}"
    finally:
        for s in servers:
            s.close()


def test_zk_noise_seed_through_the_abi_matches_the_oracle():
    """bx_prove_segment_zk: the ZK rows' generator is an explicit argument (upstream's is a thread RNG, hence its unreproducible
    seals).  Same pair -> the oracle's seal word for word; another noise seed -> another seal of the same statement."""
    from boundless_amd.prover import HipProverServer, Segment

    srv = HipProverServer(0, po2=12, widths=(4, 16, 8))
    try:
        for seed, noise in ((7, 1), (7, 2), (8, 0xFFFFFFFFFFFFFFFF)):
            r = srv.prove_segment(Segment(index=0, po2=12, seed=seed, noise_seed=noise))
            want, _ = ol.prove_segment(12, 4, 16, 8, seed, noise_seed=noise)
            assert np.array_equal(r.seal, want), (seed, noise)
            r.verify_integrity()
        a = srv.prove_segment(Segment(index=0, po2=12, seed=7, noise_seed=1)).seal
        b = srv.prove_segment(Segment(index=0, po2=12, seed=7, noise_seed=2)).seal
        d = srv.prove_segment(Segment(index=0, po2=12, seed=7)).seal  # default: derived from the seed
        assert not np.array_equal(a, b) and np.array_equal(a[:8], b[:8]) and np.array_equal(a[:8], d[:8])
        assert np.array_equal(d, ol.prove_segment(12, 4, 16, 8, 7)[0])
    finally:
        srv.close()
