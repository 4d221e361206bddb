"""Times the scans and inversions of an accumulate stage: bx_batch_prefix_products (grand-product argument), the five LogUp helpers
(bx_batch_invert_ext, bx_batch_invert_elem, bx_prefix_sums, bx_batch_prefix_sums, bx_logup_accumulate) and bx_batch_ratio_products
(the running product of ratios; 48 B per element: numerators, denominators, out).

    python tools/scanbench.py [--po2 20 22] [--seqs 16] [--calls 25] [--warmup 5] [--out profiles/r10_logup_scan.json]

Per shape (2^po2 rows x `seqs` sequences; 16 = w_accum / 4 of the default widths) and per entry point: ms per call (median of `calls`
calls after `warmup`, each bracketed by HIP events on the ctx's stream) and algorithmic GB/s — the bytes DESIGN.md section 4 states for
the call: 16 B in + 16 B out per ext element, 4 B more per multiplicity for the fused call, 4 B in + 4 B out per base-field word.  Each
is also given as a fraction of bx_batch_prefix_products' bytes/s at the same shape in the same run, and of the 6.3 TB/s a copy kernel
achieves.  `unfused` = bx_batch_invert_ext and bx_batch_prefix_sums timed as one bracket: what
bx_logup_accumulate replaces, less the element-wise scale between them (which has no entry point of its own), so the fused call
beating it is the conservative comparison.  Written with the library's device-code stamp like the other summaries under profiles/.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundless_amd.build import device_code_hash  # noqa: E402
from boundless_amd.hal import HipHal  # noqa: E402

P = 2013265921
ACHIEVABLE_GBPS = 6300.0


def timed(hal, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    hal.sync()
    ms = []
    for _ in range(calls):
        hal.timer_start()
        fn()
        ms.append(hal.timer_stop())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lookback", type=int, default=1, help="the scan_lookback tunable")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_logup_scan.json"))
    a = ap.parse_args()
    assert a.calls >= 20, "report a median of at least 20 calls"
    hal = HipHal(0)
    hal.set_tunable("scan_lookback", a.lookback)
    rng = np.random.default_rng(10)
    shapes = []
    for po2 in a.po2:
        n, s = 1 << po2, a.seqs
        ext = hal.copy_from(rng.integers(1, P, 4 * n * s, dtype=np.uint32))
        out = hal.alloc(4 * n * s)
        mults = hal.copy_from(rng.integers(1, P, n * s, dtype=np.uint32))
        den = hal.copy_from(rng.integers(1, P, 4 * n * s, dtype=np.uint32))  # read-only: the denominators of ratio_products
        ext_bytes, elem_bytes = 32.0 * n * s, 8.0 * n * s
        ops = {
            "batch_prefix_products": (lambda: hal.batch_prefix_products(ext, s), ext_bytes),
            "batch_prefix_sums": (lambda: hal.batch_prefix_sums(ext, s), ext_bytes),
            "prefix_sums": (lambda: hal.prefix_sums(ext), ext_bytes),  # the same buffer as ONE sequence of n * s elements
            "batch_invert_ext": (lambda: hal.batch_invert_ext(ext), ext_bytes),
            "batch_invert_elem": (lambda: hal.batch_invert_elem(mults), elem_bytes),
            "logup_accumulate": (lambda: hal.logup_accumulate(out, ext, mults, s), ext_bytes + 4.0 * n * s),
            "logup_accumulate_in_place": (lambda: hal.logup_accumulate(ext, ext, mults, s), ext_bytes + 4.0 * n * s),
            "unfused": (lambda: (hal.batch_invert_ext(ext), hal.batch_prefix_sums(ext, s)), 2 * ext_bytes),
            # 16 B of numerators and 16 B of denominators in, 16 B out: to be read beside batch_prefix_products (32 B) and logup_accumulate (36 B)
            "ratio_products": (lambda: hal.batch_ratio_products(out, ext, den, s), 48.0 * n * s),
            "ratio_products_in_place": (lambda: hal.batch_ratio_products(ext, ext, den, s), 48.0 * n * s),
        }
        # The in-place ops keep working on what the calls before them left in `ext` (running sums get inverted, inverses get summed):
        # every kernel here is free of data-dependent branches, so the words do not move the timing.
        res = {}
        # two interleaved rounds per op, so that a drifting clock does not favour whichever op ran first
        samples = {name: [] for name in ops}
        for _ in range(2):
            for name, (fn, _b) in ops.items():
                samples[name] += timed(hal, fn, (a.calls + 1) // 2, a.warmup)
        for name, (_fn, nbytes) in ops.items():
            ms = statistics.median(samples[name])
            res[name] = {"ms": round(ms, 4), "ms_min": round(min(samples[name]), 4), "calls": len(samples[name]), "alg_bytes": nbytes,
                         "alg_GBps": round(nbytes / (ms * 1e-3) / 1e9, 1)}
        ref = res["batch_prefix_products"]["alg_GBps"]
        for r in res.values():
            r["frac_of_prefix_products"] = round(r["alg_GBps"] / ref, 3)
            r["frac_of_6.3TBps"] = round(r["alg_GBps"] / ACHIEVABLE_GBPS, 3)
        fused, unfused = res["logup_accumulate"]["ms"], res["unfused"]["ms"]
        shapes.append({"po2": po2, "seqs": s, "ops": res,
                       "fused_vs_unfused": {"fused_ms": fused, "invert_plus_sums_ms": unfused, "fused_is_faster": fused < unfused,
                                            "ratio": round(fused / unfused, 3)}})
        print(json.dumps(shapes[-1]), flush=True)
        for b in (ext, out, mults, den):
            b.free()
    doc = {"device_code_sha": device_code_hash(), "device": hal.device_name(), "scan_lookback": a.lookback,
           "note": "tools/scanbench.py: median ms per call over `calls` calls (HIP events on the ctx's stream, warm-up first, two interleaved "
                   "rounds per op); alg_GBps = the call's algorithmic bytes / median; unfused = batch_invert_ext + batch_prefix_sums in one "
                   "bracket (no scale between them)", "shapes": shapes}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    hal.close()


if __name__ == "__main__":
    main()
