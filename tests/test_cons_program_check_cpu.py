"""CPU: the constraint-program compiler and host executor (csrc/program_compile.cpp, csrc/cons_program_host.cpp) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: seeded malformed and well-formed descriptors are refused or compiled, and every compiled stream agrees
with a direct evaluation of its step list (tests/cons_program_check.cpp).  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cons_program_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cons_program_check.cpp"),
                        os.path.join(csrc, "cons_program_host.cpp"), os.path.join(csrc, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the host half compiles without a warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cons_program_check ok" in r.stdout
