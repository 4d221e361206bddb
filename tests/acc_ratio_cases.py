"""What tests/test_acc_ratio_cpu.py and tests/test_acc_ratio_gpu.py share, on top of tests/acc_program_cases.py: the inputs of a case
with ratio_zero_denominator's rows planted, and the accum width of a program with columns to spare."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_cases as cases  # noqa: E402
import acc_ratio_ref as rref  # noqa: E402

POISON, SPARE, compile_ref, w_accum = cases.POISON, cases.SPARE, cases.compile_ref, cases.w_accum


def inputs(prog, po2, pattern="random", seed=0):
    code, data, g, mix = cases.inputs(prog, po2, pattern=pattern, seed=seed)
    if hasattr(prog, "zero_cols") and pattern == "random":
        rref.plant_zero_rows(prog, data, 1 << po2)
    return code, data, g, mix
