"""What a witness program's sort costs on the device (include/bx_program.h "sorted columns", csrc/wit_sort.hip), beside torch's sort.

    python tools/witsort_bench.py [--po2 20] [--widths 16 256 64] [--calls 20] [--warmup 5] [--out profiles/r28_wit_sort.json]

One process.  One sort with keys (24, 20) bits over data columns 0 and 1 and one payload column, dests 3, 4, 5, all N rows; two key
sets: uniform random cells, and every cell equal.  Per key set, after warm-up, two interleaved rounds of
  this      bx_wit_program_run of the sorts-only program: the median by HIP events on the ctx's stream of the whole call (the empty
            per-row launch, pack, six passes of four launches, gather), and the op means of bx_profile_report for
            `wit_program_sort_pack`, `wit_program_sort`, `wit_program_sort_gather`
  torch     torch.sort(stable=True) on the same packed int64 keys and three gathers by its indices, on the same device, timed by
            torch's events: the yardstick, not this code
The dests are compared with torch's gathers word for word.  Per pass the sort moves 32 bytes per row (the keys twice and the indices
once in, both out) plus the digit table; that over the pass's time is reported as a fraction of the 6.3 TB/s the HBM-bound kernels
of DESIGN §4 are held against.  No ratio is demanded of either side.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wit_sort_ref as sref  # noqa: E402

from boundless_amd import build as b  # noqa: E402
from boundless_amd.hal import HipHal  # noqa: E402

BITS = (24, 20)
HBM_BYTES_PER_S = 6.3e12


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs=3, default=[16, 256, 64])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_wit_sort.json"))
    a = ap.parse_args()
    assert a.calls >= 20 and a.calls % 2 == 0, "report a median of at least 20 calls, in two rounds"
    po2, widths = a.po2, tuple(a.widths)
    n = 1 << po2
    passes = (sum(BITS) + 7) // 8
    hal = HipHal(0)
    prog = sref.Program()
    prog.sort([(0, BITS[0]), (1, BITS[1])], [2], [3, 4, 5])
    compiled = sref.compile_ref(prog)
    loaded = compiled.load(hal)
    code, data = hal.alloc_zeroed(n * widths[0]), hal.alloc_zeroed(n * widths[1])
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(28)
    names = ("wit_program_sort_pack", "wit_program_sort", "wit_program_sort_gather")

    def run():
        loaded.run(po2, code, widths[0], data, widths[1])

    timing, same = {}, {}
    sets = {"uniform": rng.integers(0, sref.P, (3, n), dtype=np.uint32), "equal": np.full((3, n), 123456789, np.uint32)}
    sets["equal"][2] = rng.integers(0, sref.P, n, dtype=np.uint32)
    state = {}
    for name, cols in sets.items():
        v = cols[:2].astype(np.uint64) * np.uint64(pow(1 << 32, -1, sref.P)) % np.uint64(sref.P)  # the integers the key cells stand for
        packed = ((v[0] & np.uint64((1 << BITS[0]) - 1)) << np.uint64(BITS[1])) | (v[1] & np.uint64((1 << BITS[1]) - 1))
        state[name] = {"keys": torch.from_numpy(packed.astype(np.int64)).to(dev), "cols": [torch.from_numpy(c.astype(np.int64)).to(dev) for c in cols],
                       "samples": [], "torch": [], "ops": {k: {"ms": 0.0, "calls": 0} for k in names}}

    def torch_side(st):
        _, idx = torch.sort(st["keys"], stable=True)
        return [c[idx] for c in st["cols"]]

    for _ in range(2):  # interleaved, so that a drifting clock does not favour whichever ran first
        for name, cols in sets.items():
            st = state[name]
            data.slice(0, 3 * n).copy_from(cols.reshape(-1))
            for _ in range(a.warmup):
                run()
            hal.sync()
            for _ in range(a.calls // 2):
                hal.timer_start()
                run()
                st["samples"].append(hal.timer_stop())
            hal.profile_reset()
            hal.profile_enable(True)
            for _ in range(a.calls // 2):
                run()
            hal.sync()
            hal.profile_enable(False)
            rep = hal.profile_report()
            for k in names:
                st["ops"][k]["ms"] += rep[k]["ms"]
                st["ops"][k]["calls"] += rep[k]["calls"]
            for _ in range(a.warmup):
                want = torch_side(st)
            torch.cuda.synchronize()
            for _ in range(a.calls // 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                want = torch_side(st)
                e1.record()
                torch.cuda.synchronize()
                st["torch"].append(e0.elapsed_time(e1))
            got = data.slice(3 * n, 3 * n).view().reshape(3, n)
            same[name] = bool(all(np.array_equal(got[i], want[i].cpu().numpy().astype(np.uint32)) for i in range(3)))

    for name, st in state.items():
        op = {k: v["ms"] / v["calls"] for k, v in st["ops"].items()}
        assert all(v["calls"] == a.calls for v in st["ops"].values()), st["ops"]
        pass_ms = op["wit_program_sort"] / passes
        ours, ref = statistics.median(st["samples"]), statistics.median(st["torch"])
        timing[name] = {"run_call_ms_median": round(ours, 4), "run_call_ms_min": round(min(st["samples"]), 4), "run_call_ms_max": round(max(st["samples"]), 4),
                        "calls": len(st["samples"]), **{k + "_ms": round(v, 4) for k, v in op.items()},
                        "torch_sort_and_gathers_ms_median": round(ref, 4), "torch_ms_min": round(min(st["torch"]), 4), "torch_ms_max": round(max(st["torch"]), 4),
                        "this_over_torch": round(ours / ref, 3), "pass_ms": round(pass_ms, 4), "bytes_per_pass": 32 * n,
                        "pass_fraction_of_hbm_rate": round(32 * n / (pass_ms * 1e-3) / HBM_BYTES_PER_S, 4)}
    doc = {"device_code_sha": b.device_code_hash(), "device": hal.device_name(), "po2": po2, "widths": list(widths), "bits": list(BITS), "payload_columns": 1,
           "passes": passes, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "note": "tools/witsort_bench.py: per key set two interleaved rounds after warm-up; run_call = median ms of bx_wit_program_run for a sorts-only program "
                   "(HIP events on the ctx's stream: empty per-row launch, pack, the passes, gather); the wit_program_* fields are op means of bx_profile_report; "
                   "torch = torch.sort(stable=True) on the packed int64 keys plus three gathers, same device, same run; bytes_per_pass = 32 N (keys twice and "
                   "indices once in, both out), the digit table not counted; no ratio was fixed beforehand",
           "same_words": all(same.values()), "timing": timing}
    print(json.dumps({k: doc[k] for k in ("same_words", "timing")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    loaded.unload()
    hal.close()
    assert doc["same_words"], "the dests differ from torch's stable sort"


if __name__ == "__main__":
    main()
