"""Off-line compile step of generated constraint-program kernels (include/bx_program.h, "Generated kernels").

    python -m boundless_amd.consgen DESC.json -o OUT.hsaco [--emit-only]
    python -m boundless_amd.consgen --witness DESC.json -o OUT.hsaco [--emit-only]

A description is JSON: {"n_globals": g, "ret": r, "taps": [[group, col, back], ...], "steps": [[op, a, b, c, d], ...]} with the op
numbers of enum bx_cons_op.  It is compiled by bx_cons_program_create, written as text by bx_cons_program_emit_hip and built with
hipcc, device code only, with the flags the library's own kernels are built with (build.FLAGS: gfx950, -fno-gpu-rdc,
-ffp-contract=off, -I csrc).  Beside OUT.hsaco goes OUT.meta.json: the program's digest, the compiler's resource report for
bx_cp_eval (-Rpass-analysis=kernel-resource-usage: VGPRs, SGPRs, scratch, occupancy), the program's steps and instructions, and the
seconds hipcc took.  --emit-only writes the text to OUT instead and runs no compiler.

--witness takes a WITNESS program ("Generated witness kernels"): {"taps": [[group, col, back], ...], "steps": [[op, a, b, c, d], ...],
"cells": [[global, col, row], ...], "counts": [{"col": c, "sources": [...], "bins": b, "rows": r}, ...],
"sorts": [{"keys": [[col, bits], ...], "payload": [...], "dests": [...], "rows": r}, ...]} (cells, counts and sorts optional;
counts and sorts are passed to the compiler and play no part in the kernel), compiled by bx_wit_program_create_sorted, written by bx_wit_program_emit_hip and built with the same
flags; its meta holds the digest, the resource report for bx_wp_run, steps, sets, instructions, narrow slots, text bytes and seconds.

This runs where hipcc is, before the code object is needed: the library loads what was built (bx_cons_program_attach_kernel) and
compiles nothing at run time.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

from . import build as b
from .circuit import ConsProgram, WitnessProgram


def program_of(desc):
    """-> CompiledConsProgram of a description (a dict as in the JSON above)"""
    p = ConsProgram(int(desc["n_globals"]))
    p.steps = [tuple(int(v) for v in s) for s in desc["steps"]]
    p.tap_list = [tuple(int(v) for v in t) for t in desc["taps"]]
    p.n_fp = sum(1 for s in p.steps if s[0] < 7)
    p.n_mix = len(p.steps) - p.n_fp
    return p.compile(ret=int(desc["ret"]))


def witness_program_of(desc):
    """-> CompiledWitnessProgram of a witness description (a dict as in the JSON above)"""
    w = WitnessProgram()
    w.steps = [tuple(int(v) for v in s) for s in desc["steps"]]
    w.tap_list = [tuple(int(v) for v in t) for t in desc["taps"]]
    w.cells = [tuple(int(v) for v in g) for g in desc.get("cells", [])]
    for ct in desc.get("counts", []):  # multiplicity columns: passed through, no part of the emitted kernel or its digest
        w.count(ct["col"], ct["sources"], ct["bins"], ct.get("rows", 0))
    for st in desc.get("sorts", []):  # sorted columns: likewise
        w.sort(st["keys"], st.get("payload", []), st["dests"], st.get("rows", 0))
    w.n_fp = sum(1 for s in w.steps if s[0] != 10)  # every step but BX_CONS_SET appends an fp var
    return w.compile()


_LAYOUT_KINDS = ("const", "first", "last", "active", "row", "periodic", "word")  # enum bx_layout_code_kind, in order


def layout_of(desc):
    """-> CompiledTraceLayout of a description's "layout" key (include/bx_layout.h):
    {"layout": {"stride": s, "noise_rows": z, "n_globals": g, "table": [...],
                "code": [["first"], ["last", a], ["const", a], ["active", a], ["row", a], ["periodic", a, b], ["word", a, b]],
                "fields": [{"col": c, "word": w, "shift": 0, "bits": 30, "pad": 0}, ...]}}
    A code column is its kind (a name or its number) and its operands a, b (0 when left out); PERIODIC windows index "table"."""
    from .circuit import TraceLayout

    d = desc["layout"]
    t = TraceLayout(stride=int(d.get("stride", 1)), noise_rows=int(d.get("noise_rows", 1994)), n_globals=int(d.get("n_globals", 0)))
    t.table = [int(v) for v in d.get("table", [])]
    for col in d["code"]:
        kind, ops = col[0], [int(v) for v in col[1:]] + [0, 0]
        t.code.append((_LAYOUT_KINDS.index(kind) if isinstance(kind, str) else int(kind), ops[0], ops[1]))
    for f in d.get("fields", []):
        t.field(f["col"], f["word"], f.get("shift", 0), f.get("bits", 30), f.get("pad", 0))
    return t.compile()


def _resource_usage(stderr, kernel="bx_cp_eval"):
    out, on = {}, False
    for line in stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            on = kernel in val
        elif on:
            out[key] = int(val) if val.isdigit() else val
    return out


def compile_text(text, out_path, extra_flags=(), kernel="bx_cp_eval"):
    """hipcc over one generated translation unit -> (resource report of `kernel`, seconds)"""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "bx_cp_generated.hip")
        with open(src, "w") as f:
            f.write(text)
        cmd = ["hipcc", "-x", "hip", "--cuda-device-only"] + b.FLAGS + ["-cuid=bxcpgenerated", "-Rpass-analysis=kernel-resource-usage"] + list(extra_flags) + [
            "-c", src, "-o", out_path]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        secs = time.time() - t0
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for the generated kernel:\n" + r.stdout + r.stderr[-4000:])
    return _resource_usage(r.stderr, kernel), secs


def compile_program(desc, out_path, emit_only=False):
    """Compiles the description `desc` (a dict, or the path of a JSON file) into the code object `out_path` and writes
    `<out_path minus .hsaco>.meta.json` beside it; -> the meta dict.  emit_only: writes the generated text to out_path, nothing else."""
    if not isinstance(desc, dict):
        with open(desc) as f:
            desc = json.load(f)
    prog = program_of(desc)
    try:
        text = prog.emit_hip()
        if emit_only:
            with open(out_path, "w") as f:
                f.write(text)
            return {"digest": prog.digest()}
        usage, secs = compile_text(text, out_path)
        info = prog.info
        meta = {"digest": prog.digest(), "vgprs": usage.get("VGPRs"), "agprs": usage.get("AGPRs"), "sgprs": usage.get("TotalSGPRs"),
                "scratch_bytes": usage.get("ScratchSize [bytes/lane]"), "occupancy_waves_per_simd": usage.get("Occupancy [waves/SIMD]"),
                "lds_bytes": usage.get("LDS Size [bytes/block]"), "steps": info["steps"], "instructions": info["instructions"],
                "narrow": info["narrow"], "wide": info["wide"], "text_bytes": len(text), "hipcc_seconds": round(secs, 2)}
        with open(meta_path(out_path), "w") as f:
            json.dump(meta, f, indent=1)
            f.write("\n")
        return meta
    finally:
        prog.close()


def compile_witness_program(desc, out_path, emit_only=False):
    """compile_program for a WITNESS description: the code object of bx_wp_run and its meta; -> the meta dict"""
    if not isinstance(desc, dict):
        with open(desc) as f:
            desc = json.load(f)
    prog = witness_program_of(desc)
    try:
        text = prog.emit_hip()
        if emit_only:
            with open(out_path, "w") as f:
                f.write(text)
            return {"digest": prog.digest()}
        usage, secs = compile_text(text, out_path, kernel="bx_wp_run")
        info = prog.info()
        meta = {"digest": prog.digest(), "vgprs": usage.get("VGPRs"), "agprs": usage.get("AGPRs"), "sgprs": usage.get("TotalSGPRs"),
                "scratch_bytes": usage.get("ScratchSize [bytes/lane]"), "occupancy_waves_per_simd": usage.get("Occupancy [waves/SIMD]"),
                "lds_bytes": usage.get("LDS Size [bytes/block]"), "steps": info["steps"], "sets": info["sets"], "instructions": info["instructions"],
                "narrow": info["narrow"], "text_bytes": len(text), "hipcc_seconds": round(secs, 2)}
        with open(meta_path(out_path), "w") as f:
            json.dump(meta, f, indent=1)
            f.write("\n")
        return meta
    finally:
        prog.close()


def meta_path(out_path):
    return (out_path[:-6] if out_path.endswith(".hsaco") else out_path) + ".meta.json"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("desc")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--emit-only", action="store_true")
    ap.add_argument("--witness", action="store_true", help="DESC is a witness program: build bx_wp_run")
    a = ap.parse_args(argv)
    print(json.dumps((compile_witness_program if a.witness else compile_program)(a.desc, a.out, a.emit_only)))


if __name__ == "__main__":
    sys.exit(main())
