"""Writes the program descriptions under tests/golden/consgen/ (the input of boundless_amd.consgen) from the generators of
tests/cons_program_ref.py.

    python tools/consgen_fixtures.py [--check]

One JSON file per program: the seven of tests/cons_program_cases.py, one of 1 500 steps (longer than one function of the
generated text), the square circuit, and the lookup circuit at the shapes the
tests and tools/consprog_bench.py run.  They are committed as DATA: the GPU tests and the bench tool read a description and the
code object built from it (tests/consgen_cases.py), and never generate a program again where they run, so a numpy that draws other
numbers cannot pair a program with another program's kernel.  --check writes nothing and fails if a committed file differs from
what the generators give now.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cons_program_ref as ref  # noqa: E402
from cons_program_cases import PROGRAMS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "consgen")
LOOKUPS = [(9, (3, 10, 20)), (12, (3, 10, 20)), (9, (16, 256, 64)), (20, (16, 256, 64))]


def lookup_name(po2, widths):
    return "lookup_%d_%d_%d_%d" % ((po2,) + tuple(widths))


def description(prog):
    return {"n_globals": int(prog.n_globals), "ret": int(prog.ret), "taps": [[int(v) for v in t] for t in prog.taps],
            "steps": [[int(v) for v in s] for s in prog.steps]}


def fixtures():
    out = {name: description(make()) for name, make in PROGRAMS.items()}
    # longer than one function of the generated text (csrc/cons_program_emit.cpp: CP_SEGMENT = 1024 instructions): two segments
    out["steps_1500"] = description(ref.random_program(1500, 1500, (3, 5, 8), nesting=2, ext_share=0.25, pressure=14, n_taps=30))
    out["square"] = description(ref.square_program())
    for po2, widths in LOOKUPS:
        out[lookup_name(po2, widths)] = description(ref.lookup_program(po2, widths))
    return out


def text_of(desc):
    return json.dumps(desc, separators=(",", ":")) + "\n"


def main():
    check = "--check" in sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    stale = []
    for name, desc in fixtures().items():
        path = os.path.join(OUT, name + ".json")
        if check:
            if not os.path.exists(path) or open(path).read() != text_of(desc):
                stale.append(name)
        else:
            with open(path, "w") as f:
                f.write(text_of(desc))
    if stale:
        sys.exit("stale fixtures: " + ", ".join(stale))


if __name__ == "__main__":
    main()
