"""What tests/test_cons_program_cpu.py and tests/test_cons_program_gpu.py share: a reference Program (tests/cons_program_ref.py) handed
to the library's builder step by step, and the named programs both files run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_program_ref as ref  # noqa: E402

WIDTHS = (3, 5, 8)


def to_builder(prog):
    """the library's ConsProgram holding the reference program's steps and taps (same op numbers: enum bx_cons_op)"""
    from boundless_amd.circuit import ConsProgram

    b = ConsProgram(prog.n_globals)
    b.steps = [tuple(int(v) for v in s) for s in prog.steps]
    b.tap_list = [tuple(int(v) for v in t) for t in prog.taps]
    b.n_fp, b.n_mix = prog.n_fp, prog.n_mix
    return b


def compile_ref(prog):
    return to_builder(prog).compile(ret=prog.ret)


# name -> reference program; the sizes are what the kernel can get wrong: one constraint; about 40 steps with AND_COND three deep;
# about 700 steps (many instruction fetches, slots reused); every opcode form; the two slot files at their limits (the wide one
# takes 24 * 4 + narrow KiB of LDS: above the 64 KiB a kernel may use by default), and both at their limits in one program
PROGRAMS = {
    "one_constraint": ref.one_constraint_program,
    "steps_40": lambda: ref.random_program(40, 40, WIDTHS, nesting=3, pressure=8),
    "steps_700": lambda: ref.random_program(700, 700, WIDTHS, nesting=2, ext_share=0.25, pressure=14, n_taps=30),
    "every_form": ref.every_form_program,
    "narrow_limit": ref.narrow_limit_program,
    "wide_limit": ref.wide_limit_program,
    "both_limits": ref.both_limits_program,  # 32 + 4 * 24 KiB: the whole 128 KiB the kernel may be given
}
