"""What tests/test_acc_program_cpu.py and tests/test_acc_program_gpu.py share: a reference Program (tests/acc_program_ref.py) handed to
the library's builder step by step, the columns, public words and mix a case runs on, and the accum width with columns to spare."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_ref as ref  # noqa: E402
import extreme_words  # noqa: E402

P = ref.P
POISON = 0xDEADBEEF  # not a field word: a cell nobody may write
SPARE = 3            # accum columns beyond 4 S


def to_builder(prog):
    """the library's AccumulateProgram holding the reference program's steps and taps (same op numbers: enum bx_cons_op)"""
    from boundless_amd.circuit import AccumulateProgram

    b = AccumulateProgram(n_globals=prog.n_globals)
    b.steps = list(prog.steps)
    b.tap_list = list(prog.taps)
    b.n_fp = prog.n_fp
    return b


def compile_ref(prog):
    return to_builder(prog).compile()


def w_accum(prog):
    return 4 * len(prog.sequences()) + SPARE


def inputs(prog, po2, widths=ref.WIDTHS, pattern="random", seed=0):
    """-> (code, data, globals, mix): uint32 matrices (width, N) of `pattern` (tests/extreme_words.py, or "zero"), the public words
    and the four mix words drawn from the same pattern.  A program's planted rows (zero_denominator) hold its value."""
    n = 1 << po2
    if pattern == "zero":
        code, data = (np.zeros((w, n), np.uint32) for w in widths)
        extra = np.zeros(prog.n_globals + 4, np.uint32)
    else:
        code, data = (extreme_words.pattern(pattern, (w, n), seed=1000 * seed + 10 * po2 + q) for q, w in enumerate(widths))
        extra = extreme_words.pattern(pattern, prog.n_globals + 4, seed=1000 * seed + 10 * po2 + 7)
    if prog.planted is not None:
        col, value = prog.planted
        data[col][ref.planted_rows(n)] = ref.encode(value)
    return code, data, extra[:prog.n_globals].tolist(), extra[prog.n_globals:].tolist()
