"""CPU: the factored constraint sum of csrc/circuit_dev.hpp (the core of witness_derive and eval_check), compiled for the host with
every sredc operand asserted against its bound, against the plain canonical loop — for every dispatched (T, G) and for uneven ones."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_factored_constraint_sum_equals_the_plain_loop_within_its_bounds(tmp_path):
    exe = str(tmp_path / "cons_factored_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-DBX_CHECK_BOUNDS", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}",
                        os.path.join(ROOT, "tests", "cons_factored_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cons_factored_check ok" in r.stdout
