"""CPU: the step-list compiler of the three program kinds (csrc/program_compile.cpp) against the pins of tests/golden/progstream: 1200
seeded descriptions, well-formed and broken on purpose, each either compiled — its info, stream, constants, taps and the kind's own
tables hashed field by field — or refused with its full text.  The golden file was written by the three separate compilers this one
replaced (tests/golden/progstream/README.md gives the command), so one differing line is a stream, a table, a refusal or an ORDER of
refusals that moved.  tests/program_stream_pins.cpp is a program of its own, built with AddressSanitizer and
UndefinedBehaviorSanitizer; nothing is loaded into Python under a sanitizer.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "progstream", "pins.txt")


def test_every_stream_table_and_refusal_is_the_pinned_one(tmp_path):
    exe = str(tmp_path / "program_stream_pins")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "program_stream_pins.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert not r.stderr.strip(), r.stderr
    want = open(GOLDEN, "rb").read()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.split(b"\n"), want.split(b"\n")
        first = next((k for k, (g, w) in enumerate(zip(got_lines, want_lines)) if g != w), min(len(got_lines), len(want_lines)))
        raise AssertionError(f"line {first + 1} differs:\n  got  {got_lines[first:first + 1]}\n  want {want_lines[first:first + 1]}")

    # the pins mean something only if the descriptions cover what the compiler can do; the program's last line says what they covered
    summary = want.decode().strip().split("\n")[-1]
    assert summary.startswith("summary ")
    kinds = {}
    for part in summary[len("summary "):].split(" | "):
        name, *fields = part.split()
        kinds[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    assert set(kinds) == {"cons", "wit", "acc"}
    lines = want.decode().strip().split("\n")[:-1]
    for name, k in kinds.items():
        total = k["ok"] + k["refused"]
        assert total == 400 and sum(1 for line in lines if line.startswith(name + " ")) == total
        assert 4 * k["ok"] >= total and 4 * k["refused"] >= total, (name, k)  # at least a quarter compile, at least a quarter are refused
        assert k["reuse"] >= 50, (name, k)  # more instructions than slots: slots are reused
        assert k["two_faults_refused"] >= 20, (name, k)  # descriptions that break two rules at once: the order of refusals
    assert kinds["cons"]["mixed"] >= 20 and kinds["acc"]["mixed"] >= 20  # base and ext operands in every mixed opcode of one program
    assert kinds["wit"]["forwarded"] >= 50 and kinds["wit"]["dead_forward"] >= 50  # forwarded GETs, and ones that nothing reads afterwards
    assert kinds["acc"]["all_terms"] >= 10  # base and ext SUM and PROD terms in one program
    assert all(re.fullmatch(r"(cons|wit|acc) \d+ (ok [0-9a-f]{64}|refused \S.*)", line) for line in lines)
    assert len({line.split(" ", 3)[3] for line in lines if " ok " in line}) > 600  # distinct programs, not one hashed 600 times
