"""CPU: a witness program's multiplicity columns (include/bx_program.h, "multiplicity columns") — create's refusals by name, what a
count list leaves alone (info, digest, generated text), the host executor against the definition-level reference of
tests/wit_count_ref.py, the compiler and host executor as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/wit_count_check.cpp; nothing is loaded into Python under a sanitizer), and the compiler's resource
report of the new kernels and of wit_program_kernel.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wit_count_ref as cref  # noqa: E402
import wit_program_ref as ref  # noqa: E402
from wit_program_cases import compile_ref as compile_plain  # noqa: E402

from boundless_amd import circuit  # noqa: E402
from boundless_amd.circuit import WitnessProgram  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_the_header_is_pedantic_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){bx_wit_count c; c.bins = BX_WIT_MAX_COUNT_BINS; c.rows = BX_WIT_MAX_COUNTS + BX_WIT_MAX_COUNT_SOURCES; '
                             '(void)c; return bx_wit_program_counts(0) != 0;}\n', capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wit_count_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "wit_count_check.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wit_count_check ok" in r.stdout


# ---- refusals ----
def test_create_refuses_every_rule_by_name():
    def refused(match, build):
        w = WitnessProgram()
        build(w)
        with pytest.raises(HalError, match=match):
            w.compile()

    refused(r"count 0: data column 4 is also SET \(step 1\)", lambda w: (w.const(1), w.set(4, 0), w.count(4, [0], 2)))
    refused("count 0: data column 4 is read by the GET of step 1: a multiplicity does not exist while the program runs",
            lambda w: (w.const(1), w.get(1, 4, 0), w.count(4, [0], 2)))
    refused("count 0: data column 4 is read by the GET of step 0", lambda w: (w.get(1, 4, 3), w.count(4, [0], 2)))  # any back
    refused("count 1: data column 5 is a source of count 0", lambda w: (w.count(4, [0, 5], 2), w.count(5, [1], 2)))
    refused("count 0: data column 4 is a source of count 0", lambda w: w.count(4, [0, 4], 2))
    refused("count 0: data column 4 is a source of count 1", lambda w: (w.count(4, [0], 2), w.count(5, [4], 2)))
    refused("count 0: data column 9 is a source of count 1", lambda w: (w.count(9, [1], 2), w.count(8, [9], 2), w.count(7, [8], 2)))  # list order, not column order
    refused("step 0: constant 2013265921 is not below P", lambda w: (w.const(P), w.count(4, [0], 0)))  # the step list is judged first
    refused("count 1: data column 4 is already the column of count 0", lambda w: (w.count(4, [0], 2), w.count(4, [1], 2)))
    refused(r"count 0: data column 65536 out of range \(at most 65535\)", lambda w: w.count(65536, [0], 2))
    refused("count 0: source 1: data column 65536 out of range", lambda w: w.count(4, [0, 65536], 2))
    refused("count 0: no sources", lambda w: w.count(4, [], 2))
    refused("count 0: 65 sources, more than BX_WIT_MAX_COUNT_SOURCES = 64", lambda w: w.count(100, range(65), 2))
    refused("count 0: source column 3 is named twice", lambda w: w.count(4, [3, 1, 3], 2))
    refused("count 0: bins is 0", lambda w: w.count(4, [0], 0))
    refused("count 0: bins 16777217 is above BX_WIT_MAX_COUNT_BINS = 16777216", lambda w: w.count(4, [0], (1 << 24) + 1))
    refused("count 0: bins 9 is above rows 8", lambda w: w.count(4, [0], 9, rows=8))
    refused("count 0: rows 16777217 is above 2\\^24", lambda w: w.count(4, [0], 9, rows=(1 << 24) + 1))
    refused("17 counts, more than BX_WIT_MAX_COUNTS = 16", lambda w: [w.count(100 + k, [0], 2) for k in range(17)])
    for bad in (dict(col=(1 << 32) + 4), dict(col=-1), dict(bins=(1 << 32) + 2), dict(rows=-8), dict(sources=[0, (1 << 32) + 1])):  # nothing wraps into a valid value
        with pytest.raises(ValueError, match="is not a 32-bit unsigned value"):
            WitnessProgram().count(**{**dict(col=4, sources=[0], bins=2, rows=0), **bad})
    # the limits themselves are fine, and so are a source that is SET, a cell that names a count column and a program of counts alone
    w = WitnessProgram()
    w.set(3, w.get(1, 0, 0))
    for k in range(16):
        w.count(100 + k, range(64) if k == 0 else [3], 1 << 24 if k == 1 else 8, rows=1 << 24 if k == 1 else 8)
    w.global_cell(0, 100, 5)
    prog = w.compile()
    assert len(prog.counts()) == 16 and prog.counts()[0]["sources"] == list(range(64)) and prog.counts()[1] == {"col": 101, "bins": 1 << 24, "rows": 1 << 24, "sources": [3]}
    w = WitnessProgram()
    w.count(1, [0], 3)
    prog = w.compile()
    assert prog.info() == {"steps": 0, "sets": 0, "narrow": 0, "instructions": 0, "taps": 0, "cells": 0}
    assert prog.counts() == [{"col": 1, "bins": 3, "rows": 0, "sources": [0]}]
    # an unused entry of the tap list is no GET
    w = WitnessProgram()
    w.tap(1, 4, 0)
    w.count(4, [0], 2)
    w.compile()


def test_a_count_list_changes_neither_info_nor_digest_nor_the_generated_text():
    for name, make in ref.PROGRAMS.items():
        plain = compile_plain(make())
        b = cref.to_builder(make())
        free = [c for c in range(ref.WIDTHS[1]) if c not in make().derived()]
        b.count(40, free + make().derived()[:1], 5, rows=7)
        b.count(41, free[:1], 1)
        counted = b.compile()
        assert counted.info() == plain.info(), name
        assert counted.digest() == plain.digest(), name
        assert counted.emit_hip() == plain.emit_hip(), name
        assert plain.counts() == [] and len(counted.counts()) == 2
        assert counted.derives(40) and counted.derives(41) and not plain.derives(40)
        assert all(counted.derives(c) for c in make().derived()) and not any(counted.derives(c) for c in free)


def test_create_counted_with_no_counts_is_create():
    lib = circuit._wit_lib()
    b = cref.to_builder(ref.every_form_program())
    plain = b.compile()
    steps = (circuit.ConsStep * len(b.steps))(*[circuit.ConsStep(*s) for s in b.steps])
    taps = (circuit.ConsTap * len(b.tap_list))(*[circuit.ConsTap(*t) for t in b.tap_list])
    cells = (circuit.WitGlobalCell * len(b.cells))(*[circuit.WitGlobalCell(*g) for g in b.cells])
    desc = circuit.WitProgramDesc(steps, len(b.steps), taps, len(b.tap_list), cells, len(b.cells))
    handle = C.c_void_p()
    assert not lib.bx_wit_program_create_counted(C.byref(desc), None, 0, C.byref(handle))
    other = circuit.CompiledWitnessProgram(lib, handle)
    assert other.info() == plain.info() and other.digest() == plain.digest() and other.emit_hip() == plain.emit_hip() and other.counts() == []
    assert b"null count list" in lib.bx_wit_program_create_counted(C.byref(desc), None, 1, C.byref(handle))


def test_consgen_passes_a_count_list_through():
    from boundless_amd import consgen

    desc = {"taps": [[1, 0, 0]], "steps": [[2, 0, 0, 0, 0], [10, 1, 0, 0, 0]], "counts": [{"col": 2, "sources": [0, 1], "bins": 4, "rows": 6}, {"col": 3, "sources": [1], "bins": 1}]}
    prog = consgen.witness_program_of(desc)
    assert prog.counts() == [{"col": 2, "bins": 4, "rows": 6, "sources": [0, 1]}, {"col": 3, "bins": 1, "rows": 0, "sources": [1]}]
    plain = consgen.witness_program_of({k: v for k, v in desc.items() if k != "counts"})
    assert plain.digest() == prog.digest() and plain.emit_hip() == prog.emit_hip() and plain.counts() == []
    with pytest.raises(HalError, match="count 0: bins 7 is above rows 6"):
        consgen.witness_program_of(dict(desc, counts=[{"col": 2, "sources": [0], "bins": 7, "rows": 6}]))


# ---- the host executor against the reference ----
def _columns(prog, po2, widths, kind, bins, seed=0):
    n = 1 << po2
    code = cref.source_columns("random", (widths[0], n), P, seed=seed + 1)
    data = cref.source_columns(kind, (widths[1], n), bins, seed=seed)
    data[prog.written()] = cref.POISON
    return code, data


HOST_CASES = {
    "counts_only": lambda n: cref.counts_only_program(min(3, n)),
    "counts_only_rows": lambda n: cref.counts_only_program(min(2, n - 1), rows=n - 1),
    "bins_is_rows": lambda n: cref.counts_only_program(n, rows=n, sources=(0, 1, 2, 4)),
    "one_row": lambda n: cref.counts_only_program(1, rows=1),
    "set_source": lambda n: cref.set_source_program(min(5, n)),
    "two_counts": lambda n: cref.two_counts_program(2, min(7, n - 1), rows_a=0, rows_b=n - 1),
    "wide_64": lambda n: cref.wide_program(64, min(9, n)),
}


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_run_host_is_the_reference_on_every_row(name):
    for po2 in (1, 3, 6):
        prog = HOST_CASES[name](1 << po2)
        compiled = cref.compile_ref(prog)
        widths = (ref.WIDTHS[0], 65 if name == "wide_64" else ref.WIDTHS[1])
        for kind in ("same", "mod", "random", "above"):
            bins = max(c[2] for c in prog.counts)
            code, data = _columns(prog, po2, widths, kind, bins, seed=po2)
            want = cref.evaluate(prog, po2, code, data)
            got = data.copy()
            compiled.run_host(po2, code, widths[0], got, widths[1])
            assert np.array_equal(got, want), f"po2 {po2}, {kind}: first differing (column, row) {tuple(np.argwhere(got != want)[0])}"
            free = [c for c in range(widths[1]) if c not in prog.written()]
            assert np.array_equal(got[free], data[free])
            for k, (col, sources, b, rows) in enumerate(prog.counts):
                rows = rows or (1 << po2)
                assert int(cref.decode_words(got[col, :rows]).sum()) == cref.in_range_cells(prog, k, po2, got)
                assert np.all(got[col, rows:] == cref.POISON), "a row at or above `rows` was written"
                if kind == "above" and not prog.derived():
                    assert not got[col, :rows].any()
                if kind == "same" and name == "counts_only":
                    assert int(cref.decode_words(got[col])[b - 1]) == len(sources) * rows


def test_run_host_refuses_what_does_not_fit_the_shape_by_message():
    code, data = np.zeros((3, 8), np.uint32), np.full((8, 8), 5, np.uint32)
    before = data.copy()
    for prog, match in ((cref.counts_only_program(2, rows=9), "bx_wit_program_run_host: count 0: rows 9 is above the trace's 8 rows"),
                        (cref.counts_only_program(9), r"bx_wit_program_run_host: count 0: bins 9 is above the trace's 8 rows \(rows == 0 counts all of them\)"),
                        (cref.counts_only_program(2, col=8), "bx_wit_program_run_host: count 0 fills data column 8, the data group has 8 columns"),
                        (cref.counts_only_program(2, sources=(1, 8)), "bx_wit_program_run_host: count 0: source 1 is data column 8, the data group has 8 columns"),
                        (cref.two_counts_program(2, 2, rows_b=16), "bx_wit_program_run_host: count 1: rows 16 is above the trace's 8 rows")):
        with pytest.raises(HalError, match=match):
            cref.compile_ref(prog).run_host(3, code, 3, data, 8)
        assert np.array_equal(data, before), "written before the refusal"
    cref.compile_ref(cref.counts_only_program(8, rows=8)).run_host(3, code, 3, data, 8)  # exactly N is fine


# ---- the compiler's resource report ----
def _report(src, tmp_path):
    from boundless_amd import build

    r = subprocess.run(["hipcc", "-x", "hip"] + build.FLAGS + [build.cuid_flag(src), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                               "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".co"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip().split(": ")[-1], m.group(2).strip()
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name:
            out[name][key] = int(val) if val.isdigit() else val
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_count_kernels_use_no_scratch_and_wit_program_kernel_is_unchanged(tmp_path):
    report = _report("wit_count.hip", tmp_path)
    kernels = {k: v for k, v in report.items() if "wit_count" in k}
    assert len(kernels) == 3 and {n for k in kernels for n in ("lds_kernel", "global_kernel", "store_kernel") if n in k} == {"lds_kernel", "global_kernel", "store_kernel"}
    for name, rep in kernels.items():
        assert rep["ScratchSize [bytes/lane]"] == 0 and rep["SGPRs Spill"] == 0 and rep["VGPRs Spill"] == 0, (name, rep)
        assert rep["Occupancy [waves/SIMD]"] == 8, (name, rep)
        assert rep["LDS Size [bytes/block]"] == 0, (name, rep)  # the bins are dynamic LDS: sized per count at launch
    (rep,) = [v for k, v in _report("wit_program.hip", tmp_path).items() if "wit_program_kernel" in k]
    assert (rep["VGPRs"], rep["TotalSGPRs"], rep["ScratchSize [bytes/lane]"]) == (10, 37, 0), rep
