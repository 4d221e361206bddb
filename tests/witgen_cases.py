"""What the generated-witness-kernel tests and tools/witprog_bench.py share: the witness-program descriptions committed under
tests/golden/witgen/ (written by tools/witgen_fixtures.py) and the code objects built from them into tests/_build/witgen/.

build() runs where hipcc is (__graft_entry__.build()); the GPU tests only READ a description and its code object from here, so a
program and its kernel always come from the same committed file.  Beside the programs' objects it builds two refusal fixtures:
`other_abi` (one_set's generated text built with another BX_WP_ABI) and `wrong_digest` (one_set with one constant tap moved one row
back: a kernel of another program).  A code object without bx_wp_run is any constraint kernel of tests/_build/consgen/."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import wit_program_ref as ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "witgen")
OUT = os.path.join(HERE, "_build", "witgen")
FIVE = list(ref.PROGRAMS)  # one_set, steps_40, steps_700, every_form, narrow_limit: widths (3, 8)
DERIVES = ["derive_8_2_16_16", "derive_64_4_16_16"]  # widths (16, 16)
SEVEN = FIVE + DERIVES
CIRCUITS = ["square", "cube"]
NAMES = SEVEN + CIRCUITS
SEGMENTED = {"derive_64_4_16_16": 3}  # more statements than one function of the generated text holds: name -> segments
ONE_FUNCTION = [n for n in NAMES if n not in SEGMENTED]
REFUSALS = ["other_abi", "wrong_digest"]


def widths(name):
    return (16, 16) if name in DERIVES else ref.WIDTHS


def description(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def ref_program(desc):
    """the reference Program (tests/wit_program_ref.py) holding a description's steps, taps and cells"""
    p = ref.Program()
    p.steps = [tuple(s[:3]) for s in desc["steps"]]
    p.taps = [tuple(t) for t in desc["taps"]]
    p.cells = [tuple(g) for g in desc["cells"]]
    p.n_fp = sum(1 for s in p.steps if s[0] != ref.OP_SET)
    return p


def compiled(name):
    """the library's CompiledWitnessProgram of a description"""
    from boundless_amd.consgen import witness_program_of

    return witness_program_of(description(name))


def wrong_digest_description():
    """one_set with its code tap one row further back: the same shape, another program"""
    desc = description("one_set")
    k = next(i for i, t in enumerate(desc["taps"]) if t[0] == 0)
    desc["taps"][k][2] += 1
    return desc


def kernel_path(name):
    path = os.path.join(OUT, name + ".hsaco")
    assert os.path.exists(path), f"{path} is missing: run build() (__graft_entry__.build() compiles the generated kernels)"
    return path


def meta(name):
    from boundless_amd.consgen import meta_path

    path = meta_path(kernel_path(name))
    assert os.path.exists(path), f"{path} is missing: run build()"
    with open(path) as f:
        return json.load(f)


def _newest_input():
    from boundless_amd import build as b

    deps = [os.path.join(b.CSRC, f) for f in ("wit_program_gen.hpp", "fp.hpp")] + [b.LIB]
    return max(os.path.getmtime(p) for p in deps)


def build(force=False):
    from boundless_amd import consgen

    os.makedirs(OUT, exist_ok=True)
    newest = _newest_input()

    def fresh(out, src):
        return not force and os.path.exists(out) and os.path.getmtime(out) >= max(newest, os.path.getmtime(src))

    def one(name):
        src, out = os.path.join(GOLDEN, name + ".json"), os.path.join(OUT, name + ".hsaco")
        if not (fresh(out, src) and os.path.exists(consgen.meta_path(out))):
            consgen.compile_witness_program(src, out)

    def other_abi():
        src, out = os.path.join(GOLDEN, "one_set.json"), os.path.join(OUT, "other_abi.hsaco")
        if not fresh(out, src):
            prog = compiled("one_set")
            try:
                consgen.compile_text(prog.emit_hip(), out, extra_flags=["-DBX_WP_ABI=2u"], kernel="bx_wp_run")
            finally:
                prog.close()

    def wrong_digest():
        src, out = os.path.join(GOLDEN, "one_set.json"), os.path.join(OUT, "wrong_digest.hsaco")
        if not (fresh(out, src) and os.path.exists(consgen.meta_path(out))):
            consgen.compile_witness_program(wrong_digest_description(), out)

    with ThreadPoolExecutor(max_workers=8) as ex:
        jobs = [ex.submit(one, name) for name in NAMES] + [ex.submit(other_abi), ex.submit(wrong_digest)]
        for j in jobs:
            j.result()
    return OUT
