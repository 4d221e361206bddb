"""What interpreting a circuit's derived columns costs against a hand-written kernel for the same columns, and what a kernel
generated from the same program costs.

    python tools/witprog_bench.py [--po2 20] [--widths 16 256 64] [--calls 26] [--warmup 5] [--out profiles/r22_witgen.json]
    python tools/witprog_bench.py --build-kernel [--widths 16 256 64]

One process, the synthetic circuit at the given shape and its default knobs (T, G) = (64, 4):
  yardstick    witness_derive_kernel<64,4> through the built-in table's witgen (bx_synthetic_circuit): the `witgen_derive` op of
               bx_profile_report over as many witgen calls as the interpreter is timed for, in the same run
  interpreter  wit_program_kernel (bx_wit_program_run) on the derive stage written as a witness program
               (tests/wit_program_ref.py: synthetic_derive_program) over the same code group and the same free cells
  generated    bx_wp_run, the kernel generated from that program (boundless_amd.consgen --witness), attached to a second load of it
               — a row only when its code object exists under tests/_build/witgen/ and carries the program's digest.  The benchmark
               compiles nothing: --build-kernel, run once where hipcc is, writes the description and the code object there (the
               program at widths 16 256 64 is 34 segments; __graft_entry__.build() does not build it)
The interpreter's figure is the median ms of `calls` calls after `warmup`, each bracketed by HIP events on the ctx's stream, in two
rounds interleaved with the yardstick's, and so is the generated kernel's; before any timing the data groups are compared word for
word (the derived columns of the interpreter's and the generated kernel's copies are poisoned first).  Recorded with the times: min and
max per row, their ratios, the generated kernel's meta (registers, scratch, occupancy, hipcc seconds), the program's info, the kernel's registers / scratch /
occupancy (hipcc -Rpass-analysis=kernel-resource-usage) and its dynamic LDS for this program.  Stamped with the library's device-code
hash like the other summaries under profiles/.  There is no pass mark: the figure says how much a generated witness kernel would buy.

The derive stage as a program, and the helper that hands it to the library's builder, are the test suite's (tests/wit_program_ref.py,
tests/wit_program_cases.py): this tool imports them from tests/ and does not run without that directory.
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
import wit_program_ref as ref  # noqa: E402
from wit_program_cases import compile_ref  # noqa: E402

import witgen_cases  # noqa: E402

from boundless_amd import build as b  # noqa: E402
from boundless_amd import consgen  # noqa: E402
from boundless_amd.circuit import synthetic_circuit  # noqa: E402
from boundless_amd.hal import BxBuf, HipHal  # noqa: E402
from boundless_amd.prover import Segment, SegmentParams  # noqa: E402

P = 2013265921
SRC = os.path.join(b.CSRC, "wit_program.hip")


def resource_usage(kernel="wit_program_kernel"):
    """VGPRs, SGPRs, scratch, occupancy of `kernel` as the compiler reports them for the library's flags"""
    cmd = ["hipcc", "-x", "hip"] + b.FLAGS + [b.cuid_flag("wit_program.hip"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", SRC,
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


def kernel_paths(widths, T, G):
    """(description, code object) of the derive stage at these widths under tests/_build/witgen/"""
    stem = os.path.join(witgen_cases.OUT, "derive_%d_%d_%d_%d" % (T, G, widths[0], widths[1]))
    return stem + ".json", stem + ".hsaco"


def build_kernel(widths, T, G):
    """the derive stage as a description and its code object, written once: hipcc runs here and nowhere else in this tool"""
    prog = ref.synthetic_derive_program(widths[0], widths[1], T, G)
    desc = {"taps": [list(map(int, t)) for t in prog.taps], "steps": [[int(op), int(x), int(y), 0, 0] for op, x, y in prog.steps], "cells": []}
    desc_path, out = kernel_paths(widths, T, G)
    os.makedirs(witgen_cases.OUT, exist_ok=True)
    with open(desc_path, "w") as f:
        json.dump(desc, f, separators=(",", ":"))
        f.write("\n")
    meta = consgen.compile_witness_program(desc, out)
    print(json.dumps(meta))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs=3, default=[16, 256, 64])
    ap.add_argument("--calls", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_witgen.json"))
    ap.add_argument("--build-kernel", action="store_true", help="write the derive stage's description and code object (needs hipcc, no GPU) and exit")
    ap.add_argument("--cons-terms", type=int, default=64, help="with --build-kernel: the synthetic circuit's T")
    ap.add_argument("--cons-degree", type=int, default=4, help="with --build-kernel: the synthetic circuit's G")
    a = ap.parse_args()
    if a.build_kernel:
        return build_kernel(tuple(a.widths), a.cons_terms, a.cons_degree)
    assert a.calls >= 20 and a.calls % 2 == 0, "report a median of at least 20 calls, in two rounds"
    po2, widths = a.po2, tuple(a.widths)
    n = 1 << po2
    hal = HipHal(0)
    ops = synthetic_circuit().contents
    shape = SegmentParams(po2, *widths, 0, 0)
    msg = ops.normalize(None, C.byref(shape))
    assert not msg, C.cast(msg, C.c_char_p).value
    T, G = shape.cons_terms, shape.cons_degree
    state = C.c_void_p()
    msg = ops.create(None, hal.ctx, C.byref(shape), C.byref(state))
    assert not msg, C.cast(msg, C.c_char_p).value
    code, data = hal.alloc(n * widths[0]), [hal.alloc(n * widths[1]), hal.alloc(n * widths[1])]
    gen_path = kernel_paths(widths, T, G)[1]
    gen_meta = None
    if os.path.exists(gen_path) and os.path.exists(consgen.meta_path(gen_path)):
        with open(consgen.meta_path(gen_path)) as f:
            gen_meta = json.load(f)
    msg = ops.code_group(None, state, hal.ctx, code.raw)
    assert not msg, C.cast(msg, C.c_char_p).value
    blob = Segment(index=0, po2=po2, seed=21).to_bytes()
    seg = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    g = (C.c_uint32 * 2)()

    def builtin(into=0):
        m = ops.witgen(None, state, hal.ctx, code.raw, data[into].raw, seg, len(blob), BxBuf(None, 0), g)
        assert not m, C.cast(m, C.c_char_p).value

    prog = ref.synthetic_derive_program(widths[0], widths[1], T, G)
    compiled = compile_ref(prog)
    loaded = compiled.load(hal)

    def interpreter():
        loaded.run(po2, code, widths[0], data[1], widths[1])

    loaded_gen = None
    if gen_meta is not None and gen_meta["digest"] == compiled.digest():  # a code object of another program is no row
        data.append(hal.alloc(n * widths[1]))
        loaded_gen = compiled.load(hal)
        loaded_gen.attach_kernel(gen_path)

    def generated():
        loaded_gen.run(po2, code, widths[0], data[2], widths[1])

    # the same free cells in both copies; the interpreter's derived columns hold poison until it has run
    builtin(0)
    builtin(1)
    poison = np.full(n, P - 1, np.uint32)
    for col in prog.derived():
        data[1].slice(col * n, n).copy_from(poison)
    interpreter()
    if loaded_gen:
        builtin(2)
        for col in prog.derived():
            data[2].slice(col * n, n).copy_from(poison)
        generated()
    same_gen = loaded_gen is None or all(bool(np.array_equal(data[0].slice(col * n, n).view(), data[2].slice(col * n, n).view())) for col in range(widths[1]))
    same = same_gen and all(bool(np.array_equal(data[0].slice(col * n, n).view(), data[1].slice(col * n, n).view())) for col in range(widths[1]))  # a column at a time

    hal.profile_reset()
    samples, samples_gen = [], []
    for _ in range(2):  # interleaved, so that a drifting clock does not favour whichever ran first
        for _ in range(a.warmup):
            builtin()
        hal.sync()
        hal.profile_enable(True)  # the timed witgen calls only
        for _ in range(a.calls // 2):
            builtin()
        hal.sync()
        hal.profile_enable(False)
        for _ in range(a.warmup):
            interpreter()
        hal.sync()
        for _ in range(a.calls // 2):
            hal.timer_start()
            interpreter()
            samples.append(hal.timer_stop())
        if loaded_gen:
            for _ in range(a.warmup):
                generated()
            hal.sync()
            for _ in range(a.calls // 2):
                hal.timer_start()
                generated()
                samples_gen.append(hal.timer_stop())
    derive = hal.profile_report()["witgen_derive"]
    assert derive["calls"] == a.calls, derive
    builtin_ms = derive["ms"] / derive["calls"]
    res = {"interpreter": {"ms": round(statistics.median(samples), 4), "ms_min": round(min(samples), 4), "ms_max": round(max(samples), 4), "calls": len(samples)},
           "builtin": {"ms": round(builtin_ms, 4), "calls": derive["calls"], "op": "witgen_derive (bx_profile_report: mean over its calls)"}}
    if loaded_gen:
        res["generated"] = {"ms": round(statistics.median(samples_gen), 4), "ms_min": round(min(samples_gen), 4), "ms_max": round(max(samples_gen), 4),
                            "calls": len(samples_gen)}
    info = compiled.info()
    doc = {"device_code_sha": b.device_code_hash(), "device": hal.device_name(), "po2": po2, "widths": list(widths), "cons_terms": T, "cons_degree": G,
           "note": "tools/witprog_bench.py: interpreter = median ms per bx_wit_program_run call (HIP events on the ctx's stream, warm-up first, two rounds "
                   "interleaved with the yardstick's) of wit_program_kernel on the synthetic derive stage as a witness program; builtin = "
                   "witness_derive_kernel through bx_synthetic_circuit()->witgen, its witgen_derive op of bx_profile_report, same code group and free cells",
           "same_words": same, "timing": res, "interpreter_over_builtin": round(res["interpreter"]["ms"] / builtin_ms, 3),
           "ns_per_row_and_instruction": round(res["interpreter"]["ms"] * 1e6 / n / info["instructions"], 6),
           "program_info": info, "lds_bytes_per_workgroup": info["narrow"] * 1024, "kernel_resources": resource_usage()}
    if loaded_gen:
        doc["note"] += "; generated = bx_wp_run (boundless_amd.consgen --witness) attached to a second load of the same program, timed like the interpreter"
        doc["interpreter_over_generated"] = round(res["interpreter"]["ms"] / res["generated"]["ms"], 3)
        doc["generated_over_builtin"] = round(res["generated"]["ms"] / builtin_ms, 3)
        doc["generated_range_below_interpreter_range"] = res["generated"]["ms_max"] < res["interpreter"]["ms_min"]
        doc["generated_kernel_meta"] = gen_meta
    print(json.dumps({k: doc[k] for k in doc if k in ("same_words", "timing", "interpreter_over_builtin", "interpreter_over_generated", "generated_over_builtin",
                                                       "program_info", "kernel_resources", "generated_kernel_meta")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    loaded.unload()
    if loaded_gen:
        loaded_gen.unload()
    hal.sync()
    ops.destroy(None, state)
    hal.close()
    assert same, "the interpreter or the generated kernel disagrees with the built-in kernel"


if __name__ == "__main__":
    main()
