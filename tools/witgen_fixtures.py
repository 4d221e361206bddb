"""Writes the witness-program descriptions under tests/golden/witgen/ (the input of boundless_amd.consgen --witness) from the
generators of tests/wit_program_ref.py.

    python tools/witgen_fixtures.py [--check]

One JSON file per program: the five of tests/wit_program_ref.py (PROGRAMS), the synthetic circuit's derive stage at widths 16 / 16
with (T, G) = (8, 2) (one function of the generated text) and (64, 4) (about 2 200 instructions: three segments, a SET in every one
of them, forwarded p_s values crossing from one to the next), and the square and cube witness programs of
tests/test_wit_program_gpu.py (restated here as reference Programs: that file needs the library).  They are committed as DATA: the
GPU tests and tools/witprog_bench.py read a description and the code object built from it (tests/witgen_cases.py), and never generate
a program again where they run, so a numpy that draws other numbers cannot pair a program with another program's kernel.  --check
writes nothing and fails if a committed file differs from what the generators give now.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wit_program_ref as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "witgen")
DERIVES = [(8, 2), (64, 4)]  # (T, G) at widths 16 / 16


def derive_name(T, G, w_code=16, w_data=16):
    return "derive_%d_%d_%d_%d" % (T, G, w_code, w_data)


def square_witness():
    """data[1] = data[0]^2 + code[0] * data[0](r-1) + 1 * data[0](r-3): _square_witness() of tests/test_wit_program_gpu.py"""
    w = ref.Program()
    x, xb, xb3, c0 = w.get(1, 0, 0), w.get(1, 0, 1), w.get(1, 0, 3), w.get(0, 0, 0)
    w.set(1, w.add(w.add(w.mul(x, x), w.mul(c0, xb)), w.mul(w.const(1), xb3)))
    return w


def cube_witness():
    """data[1] = data[0]^3 + code[0], public word 0 = data[1][0]: the witness half of _cube_programs() of tests/test_wit_program_gpu.py"""
    w = ref.Program()
    x = w.get(1, 0, 0)
    w.set(1, w.add(w.mul(w.mul(x, x), x), w.get(0, 0, 0)))
    w.global_cell(0, 1, 0)
    return w


def description(prog):
    return {"taps": [[int(v) for v in t] for t in prog.taps], "steps": [[int(op), int(a), int(b), 0, 0] for op, a, b in prog.steps],
            "cells": [[int(v) for v in g] for g in prog.cells]}


def fixtures():
    out = {name: description(make()) for name, make in ref.PROGRAMS.items()}
    for T, G in DERIVES:
        out[derive_name(T, G)] = description(ref.synthetic_derive_program(16, 16, T, G))
    out["square"] = description(square_witness())
    out["cube"] = description(cube_witness())
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
