"""CPU: the operand table and the one stream check of the three program kinds (csrc/cons_program.hpp: op_rules, program_fits) as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: for a program of each kind that holds every opcode of the
kind, the smallest bad value in every used field of every instruction is refused, a foreign opcode is refused, unused fields carry
anything, and the host executors, constraints_at and both emitters answer a corrupt stream with "corrupt instruction stream"
(tests/program_fits_check.cpp).  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_operand_table_and_stream_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "program_fits_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        "-Wno-unknown-pragmas",  # "#pragma unroll" of the shared arithmetic headers is hipcc's
                        f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "program_fits_check.cpp"),
                        os.path.join(csrc, "cons_program_host.cpp"), os.path.join(csrc, "program_compile.cpp"), os.path.join(csrc, "cons_program_emit.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # no warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "program_fits_check ok" in r.stdout
