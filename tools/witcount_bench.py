"""What a multiplicity column from data costs against the built-in lookup circuit's hand-written histogram.

    python tools/witcount_bench.py [--po2 20] [--widths 16 256 64] [--calls 20] [--warmup 5] [--out profiles/r24_wit_count.json]

One process, the lookup circuit at the given shape (V = 7 at the default widths: 14 limb columns, B = 2^15 bins, A active rows):
  yardstick  the built-in table's witgen (bx_lookup_circuit): the `lookup_hist` and `lookup_mult` op means of bx_profile_report.  Its
             histogram reads a gathered copy of the limb columns (lookup_gather_kernel, part of `lookup_fill`), which is not counted
  count      the same multiplicity column as a witness program's count (include/bx_program.h, "multiplicity columns"): one count
             over data columns 3j+1 and 3j+2, bins = B, rows = A, col = 3V, run by bx_wit_program_run on the data group the
             built-in witgen left.  Reported: the median ms of a whole run call (HIP events on the ctx's stream; it holds the
             empty per-row launch, the clear, the histogram and the store) and the `wit_program_count` / `wit_program_count_store`
             op means of bx_profile_report
Both are measured under both settings of the ctx tunable lookup_hist_lds (1: per-workgroup LDS bins, 0: global atomics), which
selects the form of either histogram; two rounds, interleaved, warm-up first.  Before any timing the count's column is compared word
for word with the built-in one (poisoned first).  There is no pass mark: the figures say what the general histogram costs and which
form wins on this input.  Stamped with the library's device-code hash like the other summaries under profiles/.

The count as a program and the helper that hands it to the library's builder are the test suite's (tests/wit_count_ref.py): this
tool imports them from tests/ and does not run without that directory.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_ref  # noqa: E402
import wit_count_ref as cref  # noqa: E402

from boundless_amd import build as b  # noqa: E402
from boundless_amd.circuit import lookup_circuit  # noqa: E402
from boundless_amd.hal import BxBuf, HipHal  # noqa: E402
from boundless_amd.prover import Segment, SegmentParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs=3, default=[16, 256, 64])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_wit_count.json"))
    a = ap.parse_args()
    assert a.calls >= 20 and a.calls % 2 == 0, "report a median of at least 20 calls, in two rounds"
    po2, widths = a.po2, tuple(a.widths)
    n = 1 << po2
    sh = lookup_ref.Shape(po2, *widths)
    hal = HipHal(0)
    ops = lookup_circuit().contents
    shape = SegmentParams(po2, *widths, 0, 0)
    msg = ops.normalize(None, C.byref(shape))
    assert not msg, C.cast(msg, C.c_char_p).value
    state = C.c_void_p()
    msg = ops.create(None, hal.ctx, C.byref(shape), C.byref(state))
    assert not msg, C.cast(msg, C.c_char_p).value
    code, data = hal.alloc(n * widths[0]), hal.alloc(n * widths[1])
    msg = ops.code_group(None, state, hal.ctx, code.raw)
    assert not msg, C.cast(msg, C.c_char_p).value
    blob = Segment(index=0, po2=po2, seed=24).to_bytes()
    seg = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    g = (C.c_uint32 * 2)()

    def builtin():
        m = ops.witgen(None, state, hal.ctx, code.raw, data.raw, seg, len(blob), BxBuf(None, 0), g)
        assert not m, C.cast(m, C.c_char_p).value

    prog = cref.lookup_count(sh.V, sh.B, sh.A)
    compiled = cref.compile_ref(prog)
    loaded = compiled.load(hal)
    mcol = data.slice(3 * sh.V * n, n)

    def count():
        loaded.run(po2, code, widths[0], data, widths[1])

    same = {}
    for lds in (1, 0):
        hal.set_tunable("lookup_hist_lds", lds)
        builtin()
        want = mcol.view().copy()
        mcol.copy_from(np.full(sh.A, cref.POISON, np.uint32))
        count()
        same[lds] = bool(np.array_equal(mcol.view(), want))
    in_range = int(cref.decode_words(want[:sh.A]).sum())

    samples = {1: [], 0: []}
    opsum = {lds: {} for lds in (1, 0)}

    def add_ops(lds, names):
        rep = hal.profile_report()
        for name in names:
            agg = opsum[lds].setdefault(name, {"ms": 0.0, "calls": 0})
            agg["ms"] += rep[name]["ms"]
            agg["calls"] += rep[name]["calls"]

    for _ in range(2):  # interleaved, so that a drifting clock does not favour whichever ran first
        for lds in (1, 0):
            hal.set_tunable("lookup_hist_lds", lds)
            for _ in range(a.warmup):
                builtin()
            hal.sync()
            hal.profile_reset()
            hal.profile_enable(True)
            for _ in range(a.calls // 2):
                builtin()
            hal.sync()
            hal.profile_enable(False)
            add_ops(lds, ("lookup_hist", "lookup_mult"))
            for _ in range(a.warmup):
                count()
            hal.sync()
            for _ in range(a.calls // 2):
                hal.timer_start()
                count()
                samples[lds].append(hal.timer_stop())
            hal.profile_reset()
            hal.profile_enable(True)
            for _ in range(a.calls // 2):
                count()
            hal.sync()
            hal.profile_enable(False)
            add_ops(lds, ("wit_program_count", "wit_program_count_store"))
    hal.set_tunable("lookup_hist_lds", 1)

    def mean(lds, name):
        agg = opsum[lds][name]
        assert agg["calls"] == a.calls, (name, agg)
        return agg["ms"] / agg["calls"]

    timing = {}
    for lds, form in ((1, "lds"), (0, "global")):
        s = samples[lds]
        new = mean(lds, "wit_program_count") + mean(lds, "wit_program_count_store")
        old = mean(lds, "lookup_hist") + mean(lds, "lookup_mult")
        timing[form] = {"run_call_ms_median": round(statistics.median(s), 4), "run_call_ms_min": round(min(s), 4), "run_call_ms_max": round(max(s), 4), "calls": len(s),
                        "wit_program_count_ms": round(mean(lds, "wit_program_count"), 4), "wit_program_count_store_ms": round(mean(lds, "wit_program_count_store"), 4),
                        "lookup_hist_ms": round(mean(lds, "lookup_hist"), 4), "lookup_mult_ms": round(mean(lds, "lookup_mult"), 4),
                        "count_over_builtin": round(new / old, 3), "histogram_over_builtin_histogram": round(mean(lds, "wit_program_count") / mean(lds, "lookup_hist"), 3)}
    doc = {"device_code_sha": b.device_code_hash(), "device": hal.device_name(), "po2": po2, "widths": list(widths), "V": sh.V, "sources": 2 * sh.V, "bins": sh.B,
           "rows": sh.A, "in_range_cells": in_range,
           "note": "tools/witcount_bench.py: per setting of lookup_hist_lds (lds = 1, global = 0), two interleaved rounds after warm-up; run_call = median ms of "
                   "bx_wit_program_run for a counts-only program (HIP events on the ctx's stream: empty per-row launch, clear, histogram, store); the *_ms "
                   "fields are op means of bx_profile_report over the timed calls; count_over_builtin = (wit_program_count + wit_program_count_store) / "
                   "(lookup_hist + lookup_mult); the built-in histogram reads a gathered copy of the limbs whose gather (in lookup_fill) is not counted",
           "same_words": same[1] and same[0], "timing": timing,
           "new_lds_over_new_global": round(timing["lds"]["wit_program_count_ms"] / timing["global"]["wit_program_count_ms"], 3),
           "builtin_lds_over_builtin_global": round(timing["lds"]["lookup_hist_ms"] / timing["global"]["lookup_hist_ms"], 3)}
    doc["winning_form"] = "lds" if doc["new_lds_over_new_global"] < 1 else "global"
    print(json.dumps({k: doc[k] for k in ("same_words", "timing", "new_lds_over_new_global", "builtin_lds_over_builtin_global", "winning_form")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    loaded.unload()
    hal.sync()
    ops.destroy(None, state)
    hal.close()
    assert doc["same_words"], "the count's column differs from the built-in circuit's"


if __name__ == "__main__":
    main()
