"""CPU: witness programs (include/bx_program.h, "Witness programs") — the compiler's refusals and its bookkeeping, the host executor
against the definition-level reference of tests/wit_program_ref.py, the synthetic circuit's derive stage written as a program against
tests/synth_ref.py, the compiler and host executor as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/wit_program_check.cpp; nothing is loaded into Python under a sanitizer), and the device kernel's resource report.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref  # noqa: E402
import wit_program_ref as ref  # noqa: E402
from wit_program_cases import columns, compile_ref  # noqa: E402

from boundless_amd.circuit import ConsProgram, WitnessProgram  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_the_header_is_pedantic_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){bx_wit_program_desc d; bx_wit_program_info i; bx_wit_global_cell g; (void)d; (void)i; (void)g; return 0;}\n',
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wit_program_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "wit_program_check.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the host half compiles without a warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wit_program_check ok" in r.stdout


# ---- refusals ----
def test_create_refuses_every_rule_by_name():
    def refused(match, build):
        w = WitnessProgram()
        build(w)
        with pytest.raises(HalError, match=match):
            w.compile()

    for op, name in ((1, "CONST_EXT"), (3, "GET_GLOBAL"), (7, "TRUE"), (8, "AND_EQZ"), (9, "AND_COND")):
        refused(f"step 1: {name} does not belong in a witness program", lambda w, op=op: (w.const(1), w._fp(op, 0, 0)))
    refused("unknown op 11", lambda w: w._fp(11))
    refused(r"tap 0: tap group 2 \(accum\) does not exist when the witness is generated", lambda w: w.get(2, 0, 0))
    refused("tap group 3 out of range", lambda w: w.get(3, 0, 0))
    refused("tap column 65536 out of range", lambda w: w.get(0, 65536, 0))
    refused("tap back 65536 out of range", lambda w: w.get(1, 0, 65536))
    refused("tap index 1 out of range", lambda w: (w.get(0, 0, 0), w._fp(2, 1)))
    refused(f"constant {P} is not below P", lambda w: w.const(P))
    refused("operand b = 1 refers to a later or missing fp var", lambda w: w.add(w.const(1), 1))
    refused("operand b = 5 refers to a later or missing fp var", lambda w: (w.const(1), w.set(1, 5)))
    refused("SET column 65536 out of range", lambda w: w.set(65536, w.const(1)))
    refused(r"step 2: data column 4 is SET a second time \(first at step 1\)", lambda w: (w.const(1), w.set(4, 0), w.set(4, 0)))
    refused("step 2: GET of derived data column 4 with back 1: another row's value may not have been written yet",
            lambda w: (w.const(1), w.set(4, 0), w.get(1, 4, 1)))
    refused("step 0: GET of derived data column 4 with back 1", lambda w: (w.get(1, 4, 1), w.set(4, 0)))  # wherever it stands
    refused("step 0: GET of derived data column 4 before its SET at step 1", lambda w: (w.get(1, 4, 0), w.set(4, 0)))
    refused("global index 1 is named twice", lambda w: (w.global_cell(1, 0, 0), w.global_cell(0, 0, 0), w.global_cell(1, 2, 5)))
    refused("global index 64 is not below BX_MAX_GLOBALS", lambda w: w.global_cell(64, 0, 0))
    with pytest.raises(HalError, match=r"the program needs 33 live values, the limit is 32 \(BX_CONS_MAX_NARROW\)"):
        compile_ref(ref.narrow_limit_program(extra=1))
    assert compile_ref(ref.narrow_limit_program()).info()["narrow"] == 32


def test_a_constraint_program_refuses_set_and_a_get_of_a_free_column_one_row_back_is_fine():
    p = ConsProgram()
    p.const(1)
    p.steps.append((10, 0, 0, 0, 0))  # BX_CONS_SET
    with pytest.raises(HalError, match="cons_program: step 1: unknown op 10"):
        p.compile(ret=0)
    w = WitnessProgram()
    w.set(4, w.get(1, 3, 1))  # column 3 is free: any row of it may be read
    assert w.compile().info()["sets"] == 1


def test_a_forwarded_get_emits_no_instruction():
    w = WitnessProgram()
    x = w.get(1, 0, 0)
    w.set(1, x)
    y = w.get(1, 1, 0)  # the var that was stored, not a load
    prog = w.compile()
    assert (x, y) == (0, 1)
    assert prog.info() == {"steps": 3, "sets": 1, "narrow": 1, "instructions": 2, "taps": 2, "cells": 0}  # a tap and a store
    assert prog.derives(1) and not prog.derives(0)
    # ... and the forwarded var is good as an operand: column 2 = column 1's new value squared
    w.set(2, w.mul(y, y))
    prog = w.compile()
    assert prog.info()["instructions"] == 4 and prog.info()["narrow"] == 1  # the product takes the slot its dying operand gives back
    code, data = np.zeros((1, 4), np.uint32), np.zeros((3, 4), np.uint32)
    data[0] = [5, 6, 7, 8]
    prog.run_host(2, code, 1, data, 3)
    assert data[1].tolist() == [5, 6, 7, 8]
    assert data[2].tolist() == [v * v * ref.R_INV % P for v in (5, 6, 7, 8)]


# ---- the host executor against the reference ----
@pytest.mark.parametrize("name", list(ref.PROGRAMS))
def test_run_host_is_the_reference_on_every_row(name):
    prog = ref.PROGRAMS[name]()
    compiled = compile_ref(prog)
    assert compiled.info()["sets"] == len(prog.derived()) and all(compiled.derives(c) for c in prog.derived())
    for po2 in (1, 3, 6):
        for pattern in ("random", "zero", "all_pm1", "alt_half"):
            code, data = columns(prog, po2, ref.WIDTHS, pattern)
            want = ref.evaluate(prog, po2, code, data)
            got = data.copy()
            compiled.run_host(po2, code, ref.WIDTHS[0], got, ref.WIDTHS[1])
            assert np.array_equal(got, want), f"po2 {po2}, {pattern}: first differing (column, row) {tuple(np.argwhere(got != want)[0])}"
            free = [c for c in range(ref.WIDTHS[1]) if c not in prog.derived()]
            assert np.array_equal(got[free], data[free])
            if pattern == "random":
                assert not np.any(got[prog.derived()] == P - 1), "degenerate reference: the poison survives"


def test_run_host_refuses_what_does_not_fit_by_message():
    prog = ref.every_form_program()  # taps code column 2 and data column 5, sets data column 7
    compiled = compile_ref(prog)
    code, data = columns(prog, 3, ref.WIDTHS)
    before = data.copy()
    with pytest.raises(HalError, match="bx_wit_program_run_host: the program taps column 2 of group 0, which has 2 columns"):
        compiled.run_host(3, code[:2].copy(), 2, data, 8)
    with pytest.raises(HalError, match="bx_wit_program_run_host: the program sets data column 7, the data group has 7 columns"):
        compiled.run_host(3, code, 3, data[:7].copy(), 7)
    with pytest.raises(HalError, match=r"po2 must be in \[1, 24\]"):
        compiled.run_host(0, code[:, :1].copy(), 3, data[:, :1].copy(), 8)
    assert np.array_equal(data, before)


@pytest.mark.parametrize("T,G", [(8, 2), (64, 4)])
def test_the_synthetic_derive_stage_as_a_program_gives_synth_refs_columns(T, G):
    """the one program whose words an independent, already trusted restatement defines"""
    sh = synth_ref.Shape(7, 16, 16, 16, T, G)
    prog = ref.synthetic_derive_program(16, 16, T, G)
    assert sorted(prog.derived()) == list(range(sh.F, 16))
    want, _ = synth_ref.data_columns(sh, seed=1234)
    code = synth_ref.code_columns(sh)
    data = want.copy()
    data[sh.F:] = P - 1
    compile_ref(prog).run_host(7, code, 16, data, 16)
    assert np.array_equal(data, want)
    assert np.array_equal(ref.evaluate(prog, 7, code, np.where(np.arange(16)[:, None] >= sh.F, np.uint32(P - 1), want)), want)


# ---- the device kernel's resource report ----
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_kernel_compiles_for_gfx950_without_scratch_or_spills(tmp_path):
    from boundless_amd import build

    src = os.path.join(CSRC, "wit_program.hip")
    r = subprocess.run(["hipcc", "-x", "hip"] + build.FLAGS + [build.cuid_flag("wit_program.hip"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                               "-c", src, "-o", str(tmp_path / "wit_program.co")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    report = r.stderr[r.stderr.index("wit_program_kernel"):]

    def field(name):
        return int(re.search(re.escape(name) + r": (\d+)", report).group(1))

    assert field("ScratchSize [bytes/lane]") == 0
    assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
    assert field("Occupancy [waves/SIMD]") == 8  # as cons_program_kernel has
    assert field("LDS Size [bytes/block]") == 0  # the slot file is dynamic: sized per program at launch
