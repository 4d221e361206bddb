"""CPU: the RATIO step of accumulate programs (include/bx_program.h, "Accumulate programs") — the compiler's new refusals and its
bookkeeping (ratios(), info()), the op numbers that must stay unknown, the host executor against the definition-level reference of
tests/acc_ratio_ref.py, the zero rule, the compiler and the host executor as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/acc_ratio_check.cpp; nothing is loaded into Python under a sanitizer), and the promise that a
program without RATIO compiles and runs to what it did: tests/golden/accprog/parent_run_host_pins.json holds info() and the SHA-256
of run_host's words (po2 1, 3 and 6 of acc_program_cases.inputs) for the seven named programs of tests/acc_program_ref.py, written
with the library of the commit before RATIO.  No GPU."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_ref as ref  # noqa: E402
import acc_ratio_ref as rref  # noqa: E402
from acc_ratio_cases import POISON, SPARE, compile_ref, inputs, w_accum  # noqa: E402

from boundless_amd.circuit import AccumulateProgram, ConsProgram, WitnessProgram  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_the_header_is_pedantic_c99_and_ratio_is_op_16():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){const char* (*f)(const bx_acc_program*, uint32_t*) = bx_acc_program_ratios; (void)f; '
                             "return BX_CONS_RATIO - 16;}\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "acc_ratio_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "acc_ratio_check.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "acc_ratio_check ok" in r.stdout


# ---- refusals ----
def _refused(match, build, n_globals=0):
    p = AccumulateProgram(n_globals=n_globals)
    build(p)
    with pytest.raises(HalError, match="acc_program: .*" + match):
        p.compile()


def test_create_refuses_the_new_rules_by_name():
    _refused(r"step 2: SUM sequence 1 is numbered above a RATIO sequence \(step 1: RATIO sequence 0 is numbered below a SUM sequence\)",
             lambda p: (p.const(1), p.ratio(0, 0, 0), p.sum_(1, 0, 0)))
    _refused(r"step 1: PROD sequence 1 is numbered above a RATIO sequence \(step 2: RATIO sequence 0 is numbered below a PROD sequence\): "
             "all sums come first, then all products, then all ratios", lambda p: (p.const(1), p.prod(1, 0), p.ratio(0, 0, 0)))
    _refused(r"PROD sequence 2 is numbered above a RATIO sequence \(step 3: RATIO sequence 1 is numbered below",
             lambda p: (p.const(1), p.prod(0, 0), p.prod(2, 0), p.ratio(1, 0, 0)))
    # the existing text, with a RATIO in the program too
    _refused("SUM sequence 1 is numbered above a PROD sequence: all sums come first, then all products", lambda p: (p.const(1), p.prod(0, 0), p.sum_(1, 0, 0), p.ratio(2, 0, 0)))
    # the rules that cover all three kinds, in their existing words
    _refused(r"step 2: sequence 0 is defined a second time \(first at step 1\)", lambda p: (p.const(1), p.ratio(0, 0, 0), p.ratio(0, 0, 0)))
    _refused(r"step 2: sequence 0 is defined a second time \(first at step 1\)", lambda p: (p.const(1), p.prod(0, 0), p.ratio(0, 0, 0)))
    _refused("sequence 1 is not defined: the sequences must be exactly 0 .. S-1", lambda p: (p.const(1), p.prod(0, 0), p.ratio(2, 0, 0)))
    _refused("sequence 1024 is not below BX_ACC_MAX_SEQS = 1024", lambda p: p.ratio(1024, p.const(1), 0))
    _refused("step 1: operand a = 5 refers to a later or missing fp var", lambda p: (p.const(1), p.ratio(0, 5, 0)))
    _refused("step 1: operand b = 7 refers to a later or missing fp var", lambda p: (p.const(1), p.ratio(0, 0, 7)))


def test_the_numbers_between_prod_and_ratio_stay_unknown_ops():
    for op in (13, 14, 15, 99):
        _refused(f"step 1: unknown op {op}", lambda p, op=op: (p.const(1), p.steps.append((op, 0, 0, 0, 0))))
    for op in (13, 14, 15, 16, 99):
        p = ConsProgram()
        p.const(1)
        p.steps.append((op, 0, 0, 0, 0))
        with pytest.raises(HalError, match=f"cons_program: step 1: unknown op {op}"):
            p.compile(ret=0)
        w = WitnessProgram()
        w.steps.append((op, 0, 0, 0, 0))
        with pytest.raises(HalError, match=f"wit_program: step 0: unknown op {op}"):
            w.compile()


# ---- bookkeeping ----
def test_ratios_and_info_of_the_named_programs():
    """fails on a library without RATIO: the builder has no `ratio`, the compiler no op 16"""
    p = AccumulateProgram(n_globals=1)
    a, b = p.get(1, 4, 0), p.get(0, 2, 1)
    p.sum_(0, a, p.add(b, p.global_(0)))
    p.ratio(1, a, p.mul(b, p.const_ext(1, 1, 0, 0)))
    prog = p.compile()
    assert prog.ratios() == 1
    # steps: 2 GETs, global, add, SUM, const_ext, mul, RATIO; instructions: 6 values + TSUM + TPROD + TDEN
    assert prog.info() == {"steps": 8, "sequences": 2, "sums": 1, "instructions": 9, "narrow": 3, "wide": 1, "taps": 2, "kept": 2, "n_globals": 1}
    for name, make in rref.PROGRAMS.items():
        r = make()
        c = compile_ref(r)
        info = c.info()
        assert (info["sequences"], info["sums"], c.ratios()) == rref.COUNTS[name], name
        assert (info["taps"], info["steps"], c.kept()) == (len(r.taps), len(r.steps), r.kept()), name
        assert r.ratios() == c.ratios() and len(r.sequences()) == info["sequences"]
    for make in ref.PROGRAMS.values():
        assert compile_ref(make()).ratios() == 0


def test_a_program_without_ratio_is_what_it_was():
    with open(os.path.join(ROOT, "tests", "golden", "accprog", "parent_run_host_pins.json")) as f:
        pins = json.load(f)
    assert set(pins) == set(ref.PROGRAMS) and len(pins) == 7
    for name, make in ref.PROGRAMS.items():
        prog = make()
        c = compile_ref(prog)
        assert c.info() == pins[name]["info"], name
        h = hashlib.sha256()
        for po2 in (1, 3, 6):
            code, data, g, mix = inputs(prog, po2)
            wa = w_accum(prog)
            got = np.full((wa, 1 << po2), POISON, np.uint32)
            c.run_host(po2, code, ref.WIDTHS[0], data, ref.WIDTHS[1], g, mix, got, wa)
            h.update(got.tobytes())
        assert h.hexdigest() == pins[name]["run_host_sha256"], f"{name}: run_host's words moved"


# ---- the host executor against the reference ----
def _run_host(prog, compiled, po2, pattern, seed=0):
    code, data, g, mix = inputs(prog, po2, pattern=pattern, seed=seed)
    wa, S = w_accum(prog), len(prog.sequences())
    want = rref.evaluate(prog, po2, code, data, g, mix)
    got = np.full((wa, 1 << po2), POISON, np.uint32)
    compiled.run_host(po2, code, ref.WIDTHS[0], data, ref.WIDTHS[1], g, mix, got, wa)
    bad = np.argwhere(got[:4 * S] != want)
    assert bad.size == 0, f"po2 {po2}, {pattern}: first differing (column, row) {tuple(bad[0])}"
    assert np.all(got[4 * S:] == POISON) and SPARE > 0, "a column at or above 4 S was written"
    return want


@pytest.mark.parametrize("name", list(rref.PROGRAMS))
def test_run_host_is_the_reference_on_every_row(name):
    prog = rref.PROGRAMS[name]()
    compiled = compile_ref(prog)
    for po2 in (1, 3, 6):
        for pattern in ("random", "zero", "all_pm1", "alt_half", "alt_half_rows", "edge_mix"):
            want = _run_host(prog, compiled, po2, pattern)
            if pattern == "random" and po2 == 6 and name != "ratio_zero_denominator":
                assert len(np.unique(want[0])) > (1 << po2) // 2, "degenerate reference"


@pytest.mark.parametrize("seed", range(6))
def test_run_host_is_the_reference_on_random_programs(seed):
    prog = rref.random_program(seed, 40 + 30 * seed, sums=seed % 3, prods=(seed + 1) % 3, ratios=1 + seed % 4)
    compiled = compile_ref(prog)
    info = compiled.info()
    assert (info["sequences"], info["sums"], compiled.ratios()) == (seed % 3 + (seed + 1) % 3 + 1 + seed % 4, seed % 3, 1 + seed % 4)
    for po2 in (1, 3, 6):
        for pattern in ("random", "zero", "all_pm1", "alt_half"):
            _run_host(prog, compiled, po2, pattern, seed)


def test_a_zero_denominator_zeroes_its_sequence_from_the_planted_row_on():
    prog = rref.ratio_zero_denominator_program()
    compiled = compile_ref(prog)
    po2 = 6
    n = 1 << po2
    code, data, g, mix = inputs(prog, po2, seed=3)
    rows = rref.planted_zero_rows(n)
    zero = ref.encode(rref.ZERO_VALUE)
    for col, row in zip(prog.zero_cols, rows):
        assert list(np.nonzero(data[col] == zero)[0]) == [row]
    want = rref.evaluate(prog, po2, code, data, g, mix)
    got = np.full((w_accum(prog), n), POISON, np.uint32)
    compiled.run_host(po2, code, ref.WIDTHS[0], data, ref.WIDTHS[1], g, mix, got, w_accum(prog))
    for words in (want, got):  # on the reference too
        for s, row in enumerate(rows):
            seq = words[4 * s:4 * s + 4]
            assert not seq[:, row:].any(), f"sequence {s}: a word at or after row {row} is not zero"
            assert np.all(seq[:, :row].any(axis=0)), f"sequence {s}: a row before {row} is zero"
    assert np.array_equal(got[:8], want)


def test_run_host_refuses_too_few_accum_columns_by_message():
    prog = rref.all_three_kinds_program()
    compiled = compile_ref(prog)
    code, data, g, mix = inputs(prog, 3)
    acc = np.full((23, 8), POISON, np.uint32)
    with pytest.raises(HalError, match="bx_acc_program_run_host: the program writes 24 accum columns, the accum group has 23"):
        compiled.run_host(3, code, 3, data, 8, g, mix, acc, 23)
    assert np.all(acc == POISON)
