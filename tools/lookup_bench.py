"""Times the lookup circuit (include/bx_lookup.h) beside the synthetic circuit, on the same GPU in the same run.

    python tools/lookup_bench.py [--shapes 20:16,256,64 21:16,256,64] [--steps 20] [--warmup 3] [--out profiles/r11_lookup_circuit.json]

Per shape:
  proofs_per_s   whole proofs through bx_prove_segment_bytes with 1 and with 3 provers in flight (one ctx and one host thread each),
                 `steps` proofs per prover after `warmup`, wall clock around the threads; for circuit "lookup" and for circuit
                 "synthetic" alternating, `--runs` times each (default 3), so that a drifting clock favours neither; every run is
                 listed, with the median and the spread (max - min) / median.  The synthetic figure is the yardstick, not a target:
                 the two circuits do different work at the same widths.
  stages_ms      device time per proof of the lookup circuit's stages: the library's per-call HIP events (bx_profile_enable, in a run
                 of its own) summed over `steps` proofs and divided by `steps` — a mean, the profiler keeps no samples.
                 witgen = lookup_fill + lookup_hist + lookup_mult, accumulate = lookup_build + logup_accumulate + lookup_store,
                 and lookup_eval_check.
  histogram      the histogram KERNEL alone (the lookup_hist bracket holds that one launch; the clearing of the bins is outside
                 it) under lookup_hist_lds = 1 (per-workgroup LDS bins) and = 0 (one global atomic per limb) on the same witness,
                 and their ratio; increments = 2V * A, so increments / time is the rate to hold against the LDS atomic rate.
Written with the library's device-code stamp like the other summaries under profiles/.
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundless_amd.build import device_code_hash  # noqa: E402
from boundless_amd.hal import HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment  # noqa: E402

STAGES = ["lookup_fill", "lookup_hist", "lookup_mult", "lookup_build", "logup_accumulate", "lookup_store", "lookup_eval_check"]


def proofs_per_s(circuit, po2, widths, lanes, steps, warmup):
    srvs = [HipProverServer(0, po2=po2, widths=widths, circuit=circuit) for _ in range(lanes)]
    go = threading.Barrier(lanes + 1)
    errs = []

    def work(k):
        try:
            for i in range(warmup):
                srvs[k].prove_segment(Segment(index=i, po2=po2, seed=1000 * k + i))
            go.wait()
            for i in range(steps):
                srvs[k].prove_segment(Segment(index=i, po2=po2, seed=1000 * k + 100 + i))
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(e)
            go.abort()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(lanes)]
    for t in threads:
        t.start()
    try:
        go.wait()
    except threading.BrokenBarrierError:
        pass
    t0 = time.perf_counter()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    for s in srvs:
        s.close()
    if errs:
        raise errs[0]
    return lanes * steps / dt


def stage_times(po2, widths, steps, warmup, hist_lds):
    hal = HipHal(0)
    hal.set_tunable("lookup_hist_lds", hist_lds)
    srv = HipProverServer(0, po2=po2, widths=widths, hal=hal, circuit="lookup")
    for i in range(warmup):
        srv.prove_segment(Segment(index=i, po2=po2, seed=i))
    hal.profile_reset()
    hal.profile_enable(True)
    for i in range(steps):
        srv.prove_segment(Segment(index=i, po2=po2, seed=100 + i))
    hal.profile_enable(False)
    rep = hal.profile_report()
    srv.close()
    hal.close()
    return {name: round(rep[name]["ms"] / steps, 4) for name in STAGES if name in rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16,256,64", "21:16,256,64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per circuit and lane count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_lookup_circuit.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "report at least 20 timed proofs per prover"
    shapes = []
    for spec in a.shapes:
        po2, w = spec.split(":")
        po2, widths = int(po2), tuple(int(x) for x in w.split(","))
        n = 1 << po2
        zk = min(1994, n // 4)
        v = min((widths[1] - 1) // 3, (widths[2] // 4 - 1) // 2)
        rate = {}
        for lanes in (1, 3):
            samples = {"lookup": [], "synthetic": []}
            for _ in range(a.runs):
                for circuit in ("lookup", "synthetic"):
                    samples[circuit].append(proofs_per_s(circuit, po2, widths, lanes, a.steps, a.warmup))
            rate[f"inflight{lanes}"] = {c: {"proofs_per_s": round(statistics.median(s), 3), "runs": [round(x, 3) for x in s],
                                            "spread": round((max(s) - min(s)) / statistics.median(s), 4)} for c, s in samples.items()}
        stages = stage_times(po2, widths, a.steps, a.warmup, 1)
        plain = stage_times(po2, widths, a.steps, a.warmup, 0)
        incr = 2 * v * (n - zk)
        hist = {"increments": incr, "lds_ms": stages["lookup_hist"], "global_atomic_ms": plain["lookup_hist"],
                "ratio_global_over_lds": round(plain["lookup_hist"] / stages["lookup_hist"], 2),
                "lds_Gincr_per_s": round(incr / (stages["lookup_hist"] * 1e-3) / 1e9, 2)}
        stages["witgen"] = round(stages["lookup_fill"] + stages["lookup_hist"] + stages["lookup_mult"], 4)
        stages["accumulate"] = round(stages["lookup_build"] + stages["logup_accumulate"] + stages["lookup_store"], 4)
        shapes.append({"po2": po2, "widths": list(widths), "value_columns": v, "sequences": 2 * v + 1, "proofs_per_s": rate, "stages_ms": stages,
                       "histogram": hist})
        print(json.dumps(shapes[-1]), flush=True)
    hal = HipHal(0)
    doc = {"device_code_sha": device_code_hash(), "device": hal.device_name(), "steps": a.steps, "warmup": a.warmup,
           "runs": a.runs,
           "note": "tools/lookup_bench.py: proofs/s = provers x steps / wall time, median of `runs` alternating runs per circuit, spread = "
                   "(max - min) / median; stages_ms = mean device ms per proof from the library's per-call HIP events (a run of its own); "
                   "histogram = the histogram kernel alone under both settings of lookup_hist_lds on the same witness", "shapes": shapes}
    hal.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
