"""CPU: the weighted ext accumulator of csrc/lazy_ext.hpp (WeightedExtAcc: the 16 raw products of W * V into seven 64-bit chains that
are folded hi * R + lo and reduced once) and the tail of the synthetic circuit's eval_check built on it (accumulator_value, pair_value,
the boundary constraints through LazyExtAcc), against the canonical composition of fp.hpp.

tests/ext_mix_check.cpp is a stand-alone program: every term count from 0 to 40 and 1000, all weights +-P/2 in every sign pattern,
values all +P/2, all -P/2, alternating and at the value bound +-P, the selectors in {0, 1, P - 1, R, +-P/2}, the data word in
{0, P - 1, P/2, P/2 + 1}, every extreme fill of the columns, the challenges and the mix powers, and a million random constraints.  Built
plainly, with every bound asserted (-DBX_CHECK_BOUNDS) and with the bounds under the address and undefined-behaviour sanitizers, where a
chain that left 64 bits is a signed overflow.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-DBX_CHECK_BOUNDS"], ["-DBX_CHECK_BOUNDS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "bounds", "bounds-asan-ubsan"])
def test_weighted_sum_and_tail_equal_the_canonical_composition(tmp_path, flags):
    exe = str(tmp_path / "ext_mix_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O2", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}",
                        os.path.join(ROOT, "tests", "ext_mix_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ext_mix_check ok" in r.stdout
    # the bound the fold schedule rests on is live: a weight one step outside [-P/2, P/2] is refused where bounds are asserted
    r = subprocess.run([exe, "overweight"], capture_output=True, text=True, timeout=60)
    if "-DBX_CHECK_BOUNDS" in flags:
        assert r.returncode != 0 and "a weight that is not centred" in r.stderr, (r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 0, r.stderr
