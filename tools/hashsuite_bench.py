"""Segment-proof rate under each hash suite (`poseidon2`, `sha-256`): what bench.py measures for the default suite, for both.

    python tools/hashsuite_bench.py [--suites poseidon2,sha-256] [--po2 20,21] [--inflight 1,3] [--steps 20] [--warmup 5]

The synthetic circuit at widths 16/256/64 (bench.py's workload), one context and one prover per lane, `inflight` lanes on one GPU.
Timing as in bench.py: every lane proves its segments with blocking `prove_segment` calls on its own thread, and the window is
closed when the last lane is done.  Every seal of the timed window is verified on the CPU afterwards under its suite (outside the
window).  Prints one JSON line stamped with `device_code_sha`.
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_case(suite, po2, inflight, steps, warmup, widths=(16, 256, 64)):
    from boundless_amd.prover import HipProverServer, Segment, verify_seal

    servers = [HipProverServer(0, po2=po2, widths=widths, hashfn=suite) for _ in range(inflight)]
    try:
        def lane(i, n, base, keep):
            sv = servers[i]
            for k in range(n):
                r = sv.prove_segment(Segment(index=base + k, po2=po2, seed=0xB0D1E550000 + 1000 * i + base + k))
                if keep is not None:
                    keep.append(r)

        def window(n, base, keep):
            ts = [threading.Thread(target=lane, args=(i, n, base, keep[i] if keep else None)) for i in range(inflight)]
            t0 = time.perf_counter()
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            return time.perf_counter() - t0

        window(warmup, 0, None)
        kept = [[] for _ in range(inflight)]
        dt = window(steps, warmup, kept)
        for rs in kept:
            for r in rs:
                assert r.hashfn == suite
                verify_seal(r.seal, hashfn=suite)
        n = steps * inflight
        return {"suite": suite, "po2": po2, "widths": list(widths), "inflight": inflight, "proofs": n, "seconds": round(dt, 4),
                "proofs_per_s": round(n / dt, 3), "ms_per_proof_per_lane": round(1000 * dt / steps, 3), "seal_words": int(kept[0][0].seal.size),
                "verified": n}
    finally:
        for sv in servers:
            sv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--suites", default="poseidon2,sha-256")
    ap.add_argument("--po2", default="20,21")
    ap.add_argument("--inflight", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from boundless_amd.build import csrc_hash, device_code_hash

    cases = []
    for po2 in [int(x) for x in a.po2.split(",")]:
        for inflight in [int(x) for x in a.inflight.split(",")]:
            for suite in a.suites.split(","):
                cases.append(run_case(suite, po2, inflight, a.steps, a.warmup))
    print(json.dumps({"device_code_sha": device_code_hash(), "csrc_sha": csrc_hash(), "tool": "tools/hashsuite_bench.py",
                      "steps": a.steps, "warmup": a.warmup, "cases": cases}))


if __name__ == "__main__":
    main()
