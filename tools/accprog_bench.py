"""What interpreting a circuit's accumulate terms costs against a hand-written kernel for the same terms.

    python tools/accprog_bench.py [--po2 20] [--widths 16 256 64] [--calls 26] [--warmup 5] [--out profiles/r23_acc_program.json]

One process, the lookup circuit at the given shape (V = 7 value columns at the default widths: S = 15 running sums):
  yardstick    the built-in stage, bx_lookup_circuit()->accumulate: lookup_build_kernel + bx_logup_accumulate + the store
  subject      the same stage written as an accumulate program (tests/acc_program_ref.py: lookup_program): bx_acc_program_keep, then
               bx_acc_program_run = acc_program_kernel + bx_logup_accumulate + the store
Before any timing the program's accum columns [0, 4 S) are compared word for word with the built-in stage's.  Then, per side, the
median ms of `calls` calls after `warmup`, each bracketed by HIP events on the ctx's stream, in two rounds interleaved with the other
side's.  A last pass with bx_profile_enable gives the per-op means of both sides in the same run (the two sides share the op name
logup_accumulate: the report is read between them), so that the term kernel stands against lookup_build_kernel alone — the scans and the
store are the same calls on both sides.  Recorded with the times: min and max, the ratios, the program's info, the kernel's registers /
scratch / occupancy (hipcc -Rpass-analysis=kernel-resource-usage, when hipcc is there) and its dynamic LDS for this program.  Stamped
with the library's device-code hash like the other summaries under profiles/.  There is no pass mark: the figure sizes a generated kernel.

The stage as a program, and the helper that hands it to the library's builder, are the test suite's (tests/acc_program_ref.py,
tests/acc_program_cases.py): this tool imports them from tests/ and does not run without that directory.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import acc_program_ref as ref  # noqa: E402
from acc_program_cases import compile_ref  # noqa: E402

from boundless_amd import build as b  # noqa: E402
from boundless_amd.circuit import lookup_circuit  # noqa: E402
from boundless_amd.hal import BxBuf, HipHal  # noqa: E402
from boundless_amd.prover import Segment, SegmentParams  # noqa: E402


def resource_usage(kernel="acc_program_kernel"):
    """VGPRs, SGPRs, scratch, occupancy of `kernel` as the compiler reports them for the library's flags ({} without hipcc)"""
    if shutil.which("hipcc") is None:
        return {}
    cmd = ["hipcc", "-x", "hip"] + b.FLAGS + [b.cuid_flag("acc_program.hip"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                             os.path.join(b.CSRC, "acc_program.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, on = {}, False
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            on = kernel in val and "keep" not in val
        elif on:
            out[key] = int(val) if val.isdigit() else val
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs=3, default=[16, 256, 64])
    ap.add_argument("--calls", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_acc_program.json"))
    a = ap.parse_args()
    assert a.calls >= 20 and a.calls % 2 == 0, "report a median of at least 20 calls, in two rounds"
    po2, widths = a.po2, tuple(a.widths)
    n = 1 << po2
    V = min((widths[1] - 1) // 3, (widths[2] // 4 - 1) // 2)
    S = 2 * V + 1
    hal = HipHal(0)
    ops = lookup_circuit().contents
    shape = SegmentParams(po2, *widths, 0, 0)

    def ok(msg):
        assert not msg, C.cast(msg, C.c_char_p).value

    ok(ops.normalize(None, C.byref(shape)))
    state = C.c_void_p()
    ok(ops.create(None, hal.ctx, C.byref(shape), C.byref(state)))
    code, data = hal.alloc(n * widths[0]), hal.alloc(n * widths[1])
    accum = [hal.alloc(n * widths[2]), hal.alloc(n * widths[2])]
    ok(ops.code_group(None, state, hal.ctx, code.raw))
    blob = Segment(index=0, po2=po2, seed=23).to_bytes()
    seg = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    g = (C.c_uint32 * 2)()
    ok(ops.witgen(None, state, hal.ctx, code.raw, data.raw, seg, len(blob), BxBuf(None, 0), g))
    mix = (C.c_uint32 * 4)(*[int(v) for v in np.random.default_rng(23).integers(0, ref.P, 4)])

    compiled = compile_ref(ref.lookup_program(V))
    info = compiled.info()
    assert info["sequences"] == S and info["sums"] == S
    loaded = compiled.load(hal)
    kept, run_ext, mults = hal.alloc(n * info["kept"]), hal.alloc(4 * n * S), hal.alloc(n * S)

    def builtin():
        ok(ops.accumulate(None, state, hal.ctx, accum[0].raw, mix))

    def keep():
        loaded.keep(po2, code, widths[0], data, widths[1], kept)

    def run():
        loaded.run(po2, kept, list(g), list(mix), run_ext, mults, accum[1], widths[2])

    builtin()
    keep()
    run()
    same = all(bool(np.array_equal(accum[0].slice(c * n, n).view(), accum[1].slice(c * n, n).view())) for c in range(4 * S))  # a column at a time

    samples = {"builtin": [], "keep": [], "run": []}
    for _ in range(2):  # interleaved, so that a drifting clock does not favour whichever ran first
        for name, fn in (("builtin", builtin), ("keep", keep), ("run", run)):
            for _ in range(a.warmup):
                fn()
            hal.sync()
            for _ in range(a.calls // 2):
                hal.timer_start()
                fn()
                samples[name].append(hal.timer_stop())

    # per-op means, both sides in one run; logup_accumulate is on both sides, so the report is read in between
    hal.profile_reset()
    hal.profile_enable(True)
    for _ in range(a.calls // 2):
        builtin()
    hal.sync()
    first = hal.profile_report()
    for _ in range(a.calls // 2):
        keep()
        run()
    hal.sync()
    hal.profile_enable(False)
    both = hal.profile_report()

    def mean(rep, op, minus=None):
        ms, calls = rep[op]["ms"], rep[op]["calls"]
        if minus is not None and op in minus:
            ms, calls = ms - minus[op]["ms"], calls - minus[op]["calls"]
        assert calls == a.calls // 2, (op, calls)
        return round(ms / calls, 4)

    ops_ms = {"builtin": {op: mean(first, op) for op in ("lookup_build", "logup_accumulate", "lookup_store")},
              "program": {op: mean(both, op, first) for op in ("acc_program_keep", "acc_program_run", "logup_accumulate", "acc_program_store")}}

    def row(name):
        s = samples[name]
        return {"ms": round(statistics.median(s), 4), "ms_min": round(min(s), 4), "ms_max": round(max(s), 4), "calls": len(s)}

    res = {name: row(name) for name in samples}
    subject_ms = res["keep"]["ms"] + res["run"]["ms"]
    doc = {"device_code_sha": b.device_code_hash(), "device": hal.device_name(), "po2": po2, "widths": list(widths), "V": V, "sequences": S,
           "note": "tools/accprog_bench.py: builtin = bx_lookup_circuit()->accumulate (lookup_build_kernel + bx_logup_accumulate + store); keep, run = "
                   "bx_acc_program_keep, bx_acc_program_run (acc_program_kernel + bx_logup_accumulate + store) on the same stage as an accumulate program; "
                   "median ms per call (HIP events on the ctx's stream, warm-up first, two rounds interleaved); op_ms = per-op means of bx_profile_report "
                   "over calls/2 calls per side in the same run",
           "same_words": same, "timing": res, "op_ms": ops_ms,
           "stage_over_builtin": round(subject_ms / res["builtin"]["ms"], 3),
           "run_over_builtin": round(res["run"]["ms"] / res["builtin"]["ms"], 3),
           "term_kernel_over_lookup_build": round(ops_ms["program"]["acc_program_run"] / ops_ms["builtin"]["lookup_build"], 3),
           "ns_per_row_and_instruction": round(ops_ms["program"]["acc_program_run"] * 1e6 / n / info["instructions"], 6),
           "program_info": info, "lds_bytes_per_workgroup": (info["narrow"] + 4 * info["wide"]) * 1024, "kernel_resources": resource_usage()}
    print(json.dumps({k: doc[k] for k in ("same_words", "timing", "op_ms", "stage_over_builtin", "run_over_builtin", "term_kernel_over_lookup_build",
                                          "program_info", "kernel_resources")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    loaded.unload()
    hal.sync()
    ops.destroy(None, state)
    hal.close()
    assert same, "the accumulate program disagrees with the built-in stage"


if __name__ == "__main__":
    main()
