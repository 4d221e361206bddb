"""What tests/test_wit_program_cpu.py and tests/test_wit_program_gpu.py share: a reference Program (tests/wit_program_ref.py) handed to
the library's builder step by step, and random or extreme columns with the derived ones poisoned."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import wit_program_ref as ref  # noqa: E402

P = ref.P


def to_builder(prog):
    """the library's WitnessProgram holding the reference program's steps, taps and cells (same op numbers: enum bx_cons_op)"""
    from boundless_amd.circuit import WitnessProgram

    b = WitnessProgram()
    b.steps = [(op, a, bb, 0, 0) for op, a, bb in prog.steps]
    b.tap_list = list(prog.taps)
    b.cells = list(prog.cells)
    b.n_fp = prog.n_fp
    return b


def compile_ref(prog):
    return to_builder(prog).compile()


def columns(prog, po2, widths, pattern="random", seed=0):
    """-> (code, data) uint32 matrices (width, N): `pattern` of tests/extreme_words.py, or "zero"; the columns the program derives
    hold P - 1, so that a cell the executor does not write shows"""
    n = 1 << po2
    if pattern == "zero":
        code, data = (np.zeros((w, n), np.uint32) for w in widths)
    else:
        code, data = (extreme_words.pattern(pattern, (w, n), seed=1000 * seed + 10 * po2 + q) for q, w in enumerate(widths))
    data[prog.derived()] = P - 1
    return code, data
