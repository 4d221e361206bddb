"""CPU: the pair form of the degree-4 constraint sum of csrc/circuit_dev.hpp (cons_sum<TT, 4>, the core of witness_derive and
eval_check at the flagship knobs) — its compile-time plan, and its values against the plain canonical loop with every bound asserted —
built once plainly and once with the undefined-behaviour and address sanitizers, each a stand-alone program run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "ubsan-asan"])
def test_pair_plan_is_sound_and_the_pair_form_equals_the_plain_loop_within_its_bounds(tmp_path, flags):
    exe = str(tmp_path / "cons_pairs_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-DBX_CHECK_BOUNDS", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}",
                        os.path.join(ROOT, "tests", "cons_pairs_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cons_pairs_check ok" in r.stdout
