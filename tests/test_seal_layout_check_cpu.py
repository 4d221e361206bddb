"""CPU: the seal's layout (csrc/seal_layout.hpp, host-only) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/seal_layout_check.cpp): the length it lays out is the length of the seal the C oracle — which shares
no code with it — proves for the same shape, its invariants hold for every size and the extreme widths, and every bad circuit table is
refused by name.  Nothing is loaded into Python.  And prover and verifier take the tap sets and the FRI round rule from that one place."""
import os
import re
import subprocess

from oracle import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")

# (po2, w_code, w_data, w_accum) of the synthetic circuit; po2 9 .. 12 fold once, po2 13 twice.  (1, 1, 1): no column has more than two
# tap rows (data column 0 is also opened one row back); (2, 5, 8): data column 4 has three, the accumulators two; (3, 9, 4) and
# (40, 6, 16): odd and wide groups; (4, 8, 8): one accumulator pair (two ext accumulators over four free data columns and a `last`
# selector).
SHAPES = [(9, 1, 1, 1), (9, 2, 5, 8), (9, 3, 9, 4), (9, 40, 6, 16), (10, 4, 8, 8), (10, 2, 5, 8), (11, 3, 9, 4), (11, 1, 1, 1),
          (12, 40, 6, 16), (12, 4, 8, 8), (13, 1, 1, 1), (13, 2, 5, 8), (13, 4, 8, 8)]


def test_layout_equals_the_oracles_seals_and_holds_its_invariants_under_sanitizers(tmp_path):
    lines = []
    for po2, wc, wd, wa in SHAPES:
        seal, _ = ol.prove_segment(po2, wc, wd, wa, 3)
        rounds = 1 if po2 <= 12 else 2
        lines.append(" ".join(str(int(v)) for v in [po2, wc, wd, wa, rounds, seal.size] + seal[:6].tolist()))
    cases_txt = tmp_path / "cases.txt"
    cases_txt.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "seal_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", os.path.join(ROOT, "tests", "seal_layout_check.cpp"), os.path.join(CSRC, "circuit_host.cpp"),
                        os.path.join(CSRC, "lookup_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the layout compiles without a warning under -Wall -Wextra, and without a HIP header
    r = subprocess.run([exe, str(cases_txt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seal_layout_check ok" in r.stdout
    assert f"{len(SHAPES)} oracle seals compared" in r.stdout


def test_the_layout_is_derived_in_one_place():
    layout = open(os.path.join(CSRC, "seal_layout.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", layout), "seal_layout.hpp is host-only"
    sources = {f: open(os.path.join(CSRC, f), errors="replace").read() for f in sorted(os.listdir(CSRC))}
    # a circuit's tap sets are asked for, and the FRI rounds are counted, by the layout's builder alone
    for what, pattern in (("a circuit table's taps", r"->\s*taps\s*\("), ("BX_FRI_MIN_DEGREE", r"\bBX_FRI_MIN_DEGREE\b")):
        places = [(f, m.start()) for f, text in sources.items() for m in re.finditer(pattern, text)]
        assert [f for f, _ in places] == ["seal_layout.hpp"], (what, places)
