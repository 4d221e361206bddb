"""What interpreting a circuit's constraints costs against a hand-written kernel for the same constraints, and what a kernel
generated from the same program costs.

    python tools/consprog_bench.py [--po2 20] [--widths 16 256 64] [--calls 26] [--warmup 5] [--out profiles/r13_cons_program.json]

One process, the lookup circuit at the given shape, random evaluation matrices (neither kernel branches on data):
  yardstick    lookup_eval_check_kernel through the built-in table's eval_check (bx_lookup_circuit): what generated code for these
               constraints costs
  interpreter  cons_program_kernel (bx_cons_program_eval_check) on the lookup circuit written as a constraint program
               (tests/cons_program_ref.py: lookup_program) over the same evaluations
  generated    the kernel generated from that program (boundless_amd.consgen), attached to a second load of it — a row only when the
               shape has a description under tests/golden/consgen/ (po2 20, widths 16 256 64 has); the description and the code object
               are read from tests/consgen_cases.py's directories, nothing is generated or compiled here
Median ms of `calls` calls after `warmup`, each bracketed by HIP events on the ctx's stream, two interleaved rounds; the outputs
are compared word for word first.  Recorded with the times: their ratio, the program's info, the kernel's registers / scratch /
occupancy (hipcc -Rpass-analysis=kernel-resource-usage), its dynamic LDS for this program, and the static instruction mix of its text
(tools/isa_mix.py; the text holds CP_FETCH = 4 copies of the dispatcher, one per instruction of a fetch).  Stamped with the library's
device-code hash like the other summaries under profiles/.  There is no pass mark: the figure says what a generated kernel would buy.

The lookup circuit as a program, and the helper that hands it to the library's builder, are the test suite's (tests/cons_program_ref.py,
tests/cons_program_cases.py): this tool imports them from tests/ and does not run without that directory.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cons_program_ref as ref  # noqa: E402
from cons_program_cases import compile_ref  # noqa: E402

from boundless_amd import build as b  # noqa: E402
from boundless_amd.circuit import lookup_circuit  # noqa: E402
from boundless_amd.hal import HipHal  # noqa: E402
from boundless_amd.prover import SegmentParams  # noqa: E402

P = 2013265921
SRC = os.path.join(b.CSRC, "cons_program.hip")


def resource_usage(kernel="cons_program_kernel"):
    """VGPRs, SGPRs, scratch, occupancy of `kernel` as the compiler reports them for the library's flags"""
    cmd = ["hipcc", "-x", "hip"] + b.FLAGS + [b.cuid_flag("cons_program.hip"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", SRC,
                                             "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, on = {}, False
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            on = kernel in val
        elif on:
            out[key] = int(val) if val.isdigit() else val
    return out


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
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs=3, default=[16, 256, 64])
    ap.add_argument("--calls", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_cons_program.json"))
    a = ap.parse_args()
    assert a.calls >= 20, "report a median of at least 20 calls"
    po2, widths = a.po2, tuple(a.widths)
    dom = 4 << po2
    hal = HipHal(0)
    rng = np.random.default_rng(13)
    evals = []
    for w in widths:  # filled a column at a time: the whole matrix would be several GB of host memory
        buf = hal.alloc(dom * w)
        for c in range(w):
            buf.slice(c * dom, dom).copy_from(rng.integers(0, P, dom, dtype=np.uint32))
        evals.append(buf)
    checks = [hal.alloc(4 * dom), hal.alloc(4 * dom), hal.alloc(4 * dom)]
    pm = (C.c_uint32 * 4)(*[int(v) for v in rng.integers(0, P, 4)])
    mix = (C.c_uint32 * 4)(*[int(v) for v in rng.integers(0, P, 4)])
    g = (C.c_uint32 * 2)(*[int(v) for v in rng.integers(0, P, 2)])

    ops = lookup_circuit().contents
    shape = SegmentParams(po2, *widths, 0, 0)
    state = C.c_void_p()
    msg = ops.create(None, hal.ctx, C.byref(shape), C.byref(state))
    assert not msg, C.cast(msg, C.c_char_p).value

    def builtin():
        m = ops.eval_check(None, state, hal.ctx, checks[0].raw, evals[0].raw, evals[1].raw, evals[2].raw, pm, mix, g)
        assert not m, C.cast(m, C.c_char_p).value

    compiled = compile_ref(ref.lookup_program(po2, widths))
    loaded = compiled.load(hal)

    def interpreter():
        hal.cons_program_eval_check(loaded, po2, checks[1], evals[0], evals[1], evals[2], widths, list(pm), list(mix), list(g))

    import consgen_cases

    gen_name = "lookup_%d_%d_%d_%d" % ((po2,) + widths)
    gen_loaded = gen_compiled = gen_meta = None
    if gen_name in consgen_cases.NAMES:
        gen_compiled = consgen_cases.compiled(gen_name)
        assert gen_compiled.digest() == compiled.digest(), "the committed description is not the program this tool builds"
        gen_loaded = gen_compiled.load(hal)
        gen_loaded.attach_kernel(consgen_cases.kernel_path(gen_name))
        gen_meta = consgen_cases.meta(gen_name)

    def generated():
        hal.cons_program_eval_check(gen_loaded, po2, checks[2], evals[0], evals[1], evals[2], widths, list(pm), list(mix), list(g))

    rows = [("builtin", builtin), ("interpreter", interpreter)] + ([("generated", generated)] if gen_loaded else [])
    for _, fn in rows:
        fn()
    same = all(bool(np.array_equal(checks[0].view(), checks[k].view())) for k in range(1, len(rows)))
    samples = {k: [] for k, _ in rows}
    for _ in range(2):  # interleaved, so that a drifting clock does not favour whichever ran first
        for k, fn in rows:
            samples[k] += timed(hal, fn, a.calls // 2, a.warmup)
    res = {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "calls": len(v)} for k, v in samples.items()}
    info = compiled.info
    import isa_mix

    doc = {"device_code_sha": b.device_code_hash(), "device": hal.device_name(), "po2": po2, "widths": list(widths),
           "note": "tools/consprog_bench.py: median ms per call (HIP events on the ctx's stream, warm-up first, two interleaved rounds); builtin = "
                   "lookup_eval_check_kernel through bx_lookup_circuit()->eval_check, interpreter = cons_program_kernel on the lookup circuit as a "
                   "constraint program, same evaluations; isa_mix = static counts of the kernel's text, which holds 4 copies of the dispatcher",
           "same_words": same, "timing": res, "interpreter_over_builtin": round(res["interpreter"]["ms"] / res["builtin"]["ms"], 3),
           "ns_per_point_and_instruction": round(res["interpreter"]["ms"] * 1e6 / dom / info["instructions"], 5),
           "program_info": info, "lds_bytes_per_workgroup": (info["narrow"] + 4 * info["wide"]) * 1024,
           "kernel_resources": resource_usage(), "isa_mix": isa_mix.analyse(SRC, ["cons_program_kernel"])}
    keys = ("same_words", "timing", "interpreter_over_builtin", "program_info", "kernel_resources")
    if gen_loaded:
        doc["generated_over_builtin"] = round(res["generated"]["ms"] / res["builtin"]["ms"], 3)
        doc["interpreter_over_generated"] = round(res["interpreter"]["ms"] / res["generated"]["ms"], 3)
        doc["generated_below_interpreter"] = res["generated"]["ms_max"] < res["interpreter"]["ms_min"]  # the whole range, in this run
        doc["generated_kernel"] = gen_meta
        doc["note"] += "; generated = bx_cp_eval built off line from the same program (boundless_amd.consgen) and attached to a second load of it"
        keys += ("generated_over_builtin", "interpreter_over_generated", "generated_below_interpreter", "generated_kernel")
    print(json.dumps({k: doc[k] for k in keys}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    loaded.unload()
    if gen_loaded:
        gen_loaded.unload()
    hal.sync()
    ops.destroy(None, state)
    hal.close()
    assert same, "the executors disagree with the built-in kernel"


if __name__ == "__main__":
    main()
