"""CPU: accumulate programs (include/bx_program.h, "Accumulate programs") — the compiler's refusals and its bookkeeping, the host executor
against the definition-level reference of tests/acc_program_ref.py, the lookup circuit's accumulate stage written as a program against
tests/lookup_ref.py, the compiler and host executor as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/acc_program_check.cpp; nothing is loaded into Python under a sanitizer), the device kernels' resource reports, and the promise
that no existing stream, digest or generated text moved.  No GPU."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_ref as ref  # noqa: E402
import lookup_ref  # noqa: E402
from acc_program_cases import POISON, SPARE, compile_ref, inputs, w_accum  # noqa: E402

from boundless_amd.circuit import AccumulateProgram, ConsProgram, WitnessProgram  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_the_header_is_pedantic_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){bx_acc_program_desc d; bx_acc_program_info i; (void)d; (void)i; return BX_CONS_PROD - 12;}\n',
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "acc_program_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "acc_program_check.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the host half compiles without a warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "acc_program_check ok" in r.stdout


# ---- refusals ----
def test_create_refuses_every_rule_by_name():
    def refused(match, build, n_globals=0):
        p = AccumulateProgram(n_globals=n_globals)
        build(p)
        with pytest.raises(HalError, match="acc_program: .*" + match):
            p.compile()

    for op, name in ((7, "TRUE"), (8, "AND_EQZ"), (9, "AND_COND"), (10, "SET")):
        refused(f"step 1: {name} does not belong in an accumulate program", lambda p, op=op: (p.const(1), p._fp(op, 0, 0)))
    refused("unknown op 13", lambda p: p._fp(13))
    refused(r"tap 0: tap group 2 \(accum\): the program produces the accum group, it does not read it", lambda p: p.prod(0, p.get(2, 0, 0)))
    refused("tap group 3 out of range", lambda p: p.get(3, 0, 0))
    refused("tap column 65536 out of range", lambda p: p.get(0, 65536, 0))
    refused("tap back 65536 out of range", lambda p: p.get(1, 0, 65536))
    refused("SUM's m = 0 is ext-typed; a multiplicity must be a base value", lambda p: p.sum_(0, p.const_ext(1, 0, 0, 0), p.const(1)))
    refused(r"step 2: sequence 0 is defined a second time \(first at step 1\)", lambda p: (p.const(1), p.prod(0, 0), p.prod(0, 0)))
    refused("sequence 1 is not defined: the sequences must be exactly 0 .. S-1", lambda p: (p.const(1), p.prod(0, 0), p.prod(2, 0)))
    refused(r"the program defines no sequence \(S = 0\)", lambda p: p.const(1))
    refused("sequence 1024 is not below BX_ACC_MAX_SEQS = 1024", lambda p: p.prod(1024, p.const(1)))
    refused("SUM sequence 1 is numbered above a PROD sequence: all sums come first", lambda p: (p.const(1), p.prod(0, 0), p.sum_(1, 0, 0)))
    refused(f"constant {P} is not below P", lambda p: p.const(P))
    refused("operand d = 3 refers to a later or missing fp var", lambda p: p.sum_(0, p.const(1), 3))
    refused("global index 2 out of range", lambda p: p.global_(2), n_globals=2)
    refused("mix component 4 out of range", lambda p: p.mix(4))
    with pytest.raises(HalError, match=r"the program needs 33 live narrow \(base\) values, the limit is 32 \(BX_CONS_MAX_NARROW\)"):
        compile_ref(ref.narrow_limit_program(extra=1))
    with pytest.raises(HalError, match=r"the program needs 25 live wide \(ext\) values, the limit is 24 \(BX_CONS_MAX_WIDE\)"):
        compile_ref(ref.wide_limit_program(extra=1))
    assert compile_ref(ref.narrow_limit_program()).info()["narrow"] == 32
    assert compile_ref(ref.wide_limit_program()).info()["wide"] == 24


def test_the_other_two_compilers_do_not_know_the_new_ops():
    """existing behaviour: 10, 11 and 12 stay unknown ops to a constraint program, 11 and 12 to a witness program"""
    for op in (10, 11, 12):
        p = ConsProgram()
        p.const(1)
        p.steps.append((op, 0, 0, 0, 0))
        with pytest.raises(HalError, match=f"cons_program: step 1: unknown op {op}"):
            p.compile(ret=0)
    for op in (11, 12):
        w = WitnessProgram()
        with pytest.raises(HalError, match=f"wit_program: step 0: unknown op {op}"):
            w._fp(op)
            w.compile()


def test_info_and_kept_columns():
    p = AccumulateProgram(n_globals=1)
    a, b, a1 = p.get(1, 4, 0), p.get(0, 2, 1), p.get(1, 4, 3)  # (1, 4) twice: one kept column
    p.tap(1, 0, 0)  # in the tap list, never read: kept all the same
    p.sum_(0, a, p.add(b, p.global_(0)))
    p.prod(1, p.mul(a1, p.const_ext(1, 1, 0, 0)))
    prog = p.compile()
    assert prog.kept() == [(1, 4), (0, 2), (1, 0)]
    assert prog.info() == {"steps": 9, "sequences": 2, "sums": 1, "instructions": 9, "narrow": 4, "wide": 1, "taps": 4, "kept": 3, "n_globals": 1}
    for name, make in ref.PROGRAMS.items():
        r = make()
        info = compile_ref(r).info()
        seqs = r.sequences()
        assert compile_ref(r).kept() == r.kept(), name
        assert (info["sequences"], info["sums"], info["taps"], info["steps"]) == (len(seqs), sum(seqs.values()), len(r.taps), len(r.steps)), name


# ---- the host executor against the reference ----
@pytest.mark.parametrize("name", list(ref.PROGRAMS))
def test_run_host_is_the_reference_on_every_row(name):
    prog = ref.PROGRAMS[name]()
    compiled = compile_ref(prog)
    wa, S = w_accum(prog), len(prog.sequences())
    for po2 in (1, 3, 6):
        for pattern in ("random", "zero", "all_pm1", "alt_half", "edge_mix"):
            code, data, g, mix = inputs(prog, po2, pattern=pattern)
            want = ref.evaluate(prog, po2, code, data, g, mix)
            got = np.full((wa, 1 << po2), POISON, np.uint32)
            compiled.run_host(po2, code, ref.WIDTHS[0], data, ref.WIDTHS[1], g, mix, got, wa)
            bad = np.argwhere(got[:4 * S] != want)
            assert bad.size == 0, f"po2 {po2}, {pattern}: first differing (column, row) {tuple(bad[0])}"
            assert np.all(got[4 * S:] == POISON) and SPARE > 0, "a column at or above 4 S was written"
            if pattern == "random" and po2 == 6:
                assert len(np.unique(want[0])) > (1 << po2) // 2, "degenerate reference"


def test_zero_denominators_contribute_zero_on_the_planted_rows():
    prog = ref.zero_denominator_program()
    po2 = 6
    code, data, g, mix = inputs(prog, po2, seed=3)
    want = ref.evaluate(prog, po2, code, data, g, mix)
    rows = ref.planted_rows(1 << po2)
    assert len(rows) > 10 and np.all(data[4][rows] == ref.encode(ref.ZERO_VALUE))
    for s in (0, 1):  # the running sum does not move on a planted row (row 0: it starts at zero)
        col = want[4 * s:4 * s + 4]
        assert np.all(col[:, 0] == 0)
        for r in rows[1:]:
            assert np.array_equal(col[:, r], col[:, r - 1])
        assert len({tuple(col[:, r]) for r in range(1 << po2)}) > (1 << po2) - len(rows) - 2  # ... and moves on the others


def test_run_host_refuses_what_does_not_fit_by_message():
    prog = ref.every_form_program()  # taps code column 2 and data column 5
    compiled = compile_ref(prog)
    code, data, g, mix = inputs(prog, 3)
    wa = w_accum(prog)
    acc = np.full((wa, 8), POISON, np.uint32)
    with pytest.raises(HalError, match=r"bx_acc_program_run_host: the program taps column 2 of group 0 \(kept column \d+\), which has 2 columns"):
        compiled.run_host(3, code[:2].copy(), 2, data, 8, g, mix, acc, wa)
    with pytest.raises(HalError, match=r"bx_acc_program_run_host: the program taps column 5 of group 1 \(kept column \d+\), which has 5 columns"):
        compiled.run_host(3, code, 3, data[:5].copy(), 5, g, mix, acc, wa)
    with pytest.raises(HalError, match="bx_acc_program_run_host: the program writes 28 accum columns, the accum group has 27"):
        compiled.run_host(3, code, 3, data, 8, g, mix, acc[:27].copy(), 27)
    with pytest.raises(HalError, match=r"po2 must be in \[1, 24\]"):
        compiled.run_host(0, code[:, :1].copy(), 3, data[:, :1].copy(), 8, g, mix, acc[:, :1].copy(), wa)
    assert np.all(acc == POISON)


def test_the_lookup_accumulate_as_a_program_gives_lookup_refs_columns():
    """the one program whose words an independent, already trusted restatement defines"""
    sh = lookup_ref.Shape(9, 3, 10, 20)
    assert sh.V == 2
    code = lookup_ref.code_columns(sh)
    data, g = lookup_ref.data_columns(sh, seed=1234)
    alpha = np.random.default_rng(5).integers(0, P, 4, dtype=np.uint32).tolist()
    want = lookup_ref.accum_columns(sh, 1234, code, data, alpha)
    prog = ref.lookup_program(sh.V)
    got = np.full((sh.wa, sh.N), POISON, np.uint32)
    compile_ref(prog).run_host(9, code, sh.wc, data, sh.wd, g, alpha, got, sh.wa)
    assert np.array_equal(got[:4 * sh.S], want[:4 * sh.S])
    assert np.array_equal(ref.evaluate(prog, 9, code, data, g, alpha), want[:4 * sh.S])


# ---- the device kernels' resource reports ----
def _report(tmp_path, unit):
    from boundless_amd import build

    r = subprocess.run(["hipcc", "-x", "hip"] + build.FLAGS + [build.cuid_flag(unit), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(CSRC, unit), "-o", str(tmp_path / (unit + ".co"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stderr


def _fields(report, kernel):
    part = report[report.index(kernel):]
    names = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
    return {n: int(re.search(r"\s" + re.escape(n) + r": (\d+)", part).group(1)) for n in names}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_kernels_compile_for_gfx950_without_scratch_or_spills(tmp_path):
    report = _report(tmp_path, "acc_program.hip")
    for kernel in ("acc_program_kernel", "acc_program_keep_kernel"):
        f = _fields(report, kernel)
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (kernel, f)
        assert f["LDS Size [bytes/block]"] == 0  # the slot files are dynamic: sized per program at launch


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_other_two_interpreters_keep_the_resource_reports_they_had(tmp_path):
    """figures of the commit before accumulate programs; cp_exec moved into a header both interpreters now share"""
    before = {"cons_program_kernel": {"TotalSGPRs": 54, "VGPRs": 26, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 8, "SGPRs Spill": 0,
                                      "VGPRs Spill": 0, "LDS Size [bytes/block]": 0},
              "wit_program_kernel": {"TotalSGPRs": 37, "VGPRs": 10, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 8, "SGPRs Spill": 0,
                                     "VGPRs Spill": 0, "LDS Size [bytes/block]": 0}}
    assert _fields(_report(tmp_path, "cons_program.hip"), "cons_program_kernel") == before["cons_program_kernel"]
    assert _fields(_report(tmp_path, "wit_program.hip"), "wit_program_kernel") == before["wit_program_kernel"]


# ---- nothing that existed moved ----
def test_digests_and_generated_text_of_every_fixture_are_what_they_were():
    """the new opcodes are appended after CP_ST: tests/golden/accprog/generated_pins.json was written (tools/accprog_pins.py) with the
    library of the commit before them"""
    import consgen_cases
    import witgen_cases

    with open(os.path.join(ROOT, "tests", "golden", "accprog", "generated_pins.json")) as f:
        pins = json.load(f)
    assert set(pins) == {f"consgen/{n}" for n in consgen_cases.NAMES} | {f"witgen/{n}" for n in witgen_cases.NAMES}
    for kind, cases in (("consgen", consgen_cases), ("witgen", witgen_cases)):
        for name in cases.NAMES:
            prog = cases.compiled(name)
            try:
                assert prog.digest() == pins[f"{kind}/{name}"]["digest"], f"{kind}/{name}: the digest moved"
                assert hashlib.sha256(prog.emit_hip().encode()).hexdigest() == pins[f"{kind}/{name}"]["text_sha256"], f"{kind}/{name}: the generated text moved"
            finally:
                prog.close()
