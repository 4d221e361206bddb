"""Writes tests/golden/accprog/generated_pins.json: for every description under tests/golden/consgen/ and tests/golden/witgen/ the
program's digest and the SHA-256 of its generated text, as the library this is run with gives them.

    python tools/accprog_pins.py

The file was written with the library of the commit BEFORE accumulate programs; tests/test_acc_program_cpu.py holds every later library
to it.  That is the promise of csrc/cons_program.hpp: opcodes are only ever appended, so no existing stream, digest or generated text
changes.  Run it again only when a change is MEANT to move them.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def pins():
    import consgen_cases
    import witgen_cases

    out = {}
    for kind, cases in (("consgen", consgen_cases), ("witgen", witgen_cases)):
        for name in cases.NAMES:
            prog = cases.compiled(name)
            out[f"{kind}/{name}"] = {"digest": prog.digest(), "text_sha256": hashlib.sha256(prog.emit_hip().encode()).hexdigest()}
            prog.close()
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "accprog", "generated_pins.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
