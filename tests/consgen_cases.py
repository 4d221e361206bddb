"""What the generated-kernel tests and tools/consprog_bench.py share: the program descriptions committed under
tests/golden/consgen/ (written by tools/consgen_fixtures.py) and the code objects built from them into tests/_build/consgen/.

build() runs where hipcc is (__graft_entry__.build()); the GPU tests only READ a description and its code object from here, so a
program and its kernel always come from the same committed file.  Beside the programs' objects it builds the two refusal fixtures:
`no_symbols` (tests/golden/consgen/no_symbols.hip: a kernel with none of bx_cp_eval, bx_cp_abi, bx_cp_digest) and `other_abi`
(one_constraint's generated text built with another BX_CP_ABI)."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import cons_program_ref as ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "consgen")
OUT = os.path.join(HERE, "_build", "consgen")
SEVEN = ["one_constraint", "steps_40", "steps_700", "every_form", "narrow_limit", "wide_limit", "both_limits"]
LOOKUPS = ["lookup_9_3_10_20", "lookup_12_3_10_20", "lookup_9_16_256_64", "lookup_20_16_256_64"]
LONG = ["steps_1500"]  # more instructions than one function of the generated text holds: two segments, the slots through memory between them
NAMES = SEVEN + LONG + ["square"] + LOOKUPS
NO_SCRATCH = ["one_constraint", "steps_40", "steps_700", "every_form", "square"] + LOOKUPS  # the rest sit at the slot limits
REFUSALS = ["no_symbols", "other_abi"]


def description(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def ref_program(desc):
    """the reference Program (tests/cons_program_ref.py) holding a description's steps and taps"""
    p = ref.Program(desc["n_globals"])
    p.steps = [tuple(s) for s in desc["steps"]]
    p.taps = [tuple(t) for t in desc["taps"]]
    p.n_fp = sum(1 for s in p.steps if s[0] < ref.TRUE)
    p.n_mix = len(p.steps) - p.n_fp
    return p.done(desc["ret"])


def compiled(name):
    """the library's CompiledConsProgram of a description"""
    from boundless_amd.consgen import program_of

    return program_of(description(name))


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

    deps = [os.path.join(b.CSRC, f) for f in ("cons_program_gen.hpp", "fp.hpp", "lazy_ext.hpp", "poseidon2_arith.hpp")] + [b.LIB]
    return max(os.path.getmtime(p) for p in deps)


def build(force=False):
    from boundless_amd import build as b
    from boundless_amd import consgen

    os.makedirs(OUT, exist_ok=True)
    newest = _newest_input()

    def fresh(out, src):
        return not force and os.path.exists(out) and os.path.getmtime(out) >= max(newest, os.path.getmtime(src))

    def one(name):
        src, out = os.path.join(GOLDEN, name + ".json"), os.path.join(OUT, name + ".hsaco")
        if not (fresh(out, src) and os.path.exists(consgen.meta_path(out))):
            consgen.compile_program(src, out)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, NAMES))
    # refusal fixtures
    src, out = os.path.join(GOLDEN, "no_symbols.hip"), os.path.join(OUT, "no_symbols.hsaco")
    if not fresh(out, src):
        cmd = ["hipcc", "-x", "hip", "--cuda-device-only"] + b.FLAGS + ["-cuid=bxcpnosymbols", "-c", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for no_symbols.hip:\n" + r.stdout + r.stderr)
    src, out = os.path.join(GOLDEN, "one_constraint.json"), os.path.join(OUT, "other_abi.hsaco")
    if not fresh(out, src):
        prog = compiled("one_constraint")
        try:
            consgen.compile_text(prog.emit_hip(), out, extra_flags=["-DBX_CP_ABI=2u"])
        finally:
            prog.close()
    return OUT
