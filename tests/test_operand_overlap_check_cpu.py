"""CPU: the interval test behind the HAL's operand rule (csrc/operands.hpp: bufs_overlap, bufs_same) as a stand-alone program
(tests/operand_overlap_check.cpp), built plain and under AddressSanitizer + UndefinedBehaviorSanitizer: empty buffers, touching
intervals, one shared word, containment, and buffers at the top of the address space, where forming an end address would wrap.
Nothing is loaded into Python.  And the thresholds tests/test_hal_operands_gpu.py sizes its large cases by, read from the sources."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hal_operand_sizes as sizes  # noqa: E402


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_interval_helper_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "operand_overlap_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *flags, f"-I{CSRC}", os.path.join(ROOT, "tests", "operand_overlap_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # no warning, and no HIP header: the helper is host-only
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "operand_overlap_check ok" in r.stdout


def test_the_helper_is_host_only_and_the_entry_points_use_it():
    helper = open(os.path.join(CSRC, "operands.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", helper)
    assert '#include "operands.hpp"' in open(os.path.join(CSRC, "ctx.hpp")).read()
    # every refusal has the form "<entry point>: <operand> and <operand> overlap"
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("poly.hip", "hal.hip", "scan.hip", "ntt.hip", "poseidon2.hip", "prover.hip"))
    names = {m.group(1) for m in re.finditer(r'bufs_overlap\([^;]*"(\w+): \w+ and \w+ overlap"\);', text)}
    assert names >= set(sizes.ENTRY_POINTS_WITH_A_RULE), sorted(set(sizes.ENTRY_POINTS_WITH_A_RULE) - names)


def _constant(text, name):
    m = re.search(r"constexpr\s+(?:int|size_t)\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, f"{name} is no longer a plain constant of scan.hip"
    return int(m.group(1))


def test_large_array_cases_sit_just_past_the_thresholds_in_the_sources():
    """The GPU test's three large sizes are one element (five words) past the points where divide_rec and three_phase_rec take a third
    level and where the element-wise kernels take a second grid-stride trip.  A constant that moves fails here, not silently there."""
    scan = open(os.path.join(CSRC, "scan.hip")).read()
    div_l, div_direct = _constant(scan, "DIV_L"), _constant(scan, "DIV_DIRECT")
    pp_l, pp_direct = _constant(scan, "PP_L"), _constant(scan, "PP_DIRECT")
    # the recursions still have the shape the thresholds are derived from: direct at or below *_DIRECT, one level per factor of *_L
    assert re.search(r"if \(n <= DIV_DIRECT\)", scan) and re.search(r"chunks = \(n \+ DIV_L - 1\) / DIV_L", scan)
    assert re.search(r"if \(EXCL && n <= PP_DIRECT\)", scan) and re.search(r"chunks = \(n \+ PP_L - 1\) / PP_L", scan)
    poly = open(os.path.join(CSRC, "poly.hip")).read()
    m = re.search(r"grid1d\(size_t n, unsigned bs = (\d+), size_t cap = (\d+)\)", poly)
    assert m, "grid1d's defaults are no longer in its signature"
    bs, cap = int(m.group(1)), int(m.group(2))
    for kernel in ("eltwise_add_kernel", "eltwise_mul_factor_kernel", "eltwise_zeroize_kernel"):
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(grid1d\(\w+\.len\)\), dim3\(%d\)" % (kernel, bs), poly), kernel
    assert sizes.DIVIDE_THIRD_LEVEL == div_direct * div_l * div_l == 1 << 21
    assert sizes.SCAN_THIRD_LEVEL == pp_direct * pp_l * pp_l == 1 << 23
    assert sizes.ELTWISE_ONE_TRIP == cap * bs == 65536 * 256
    assert sizes.DIVIDE_N == sizes.DIVIDE_THIRD_LEVEL + 1 and sizes.SCAN_N == sizes.SCAN_THIRD_LEVEL + 1
    assert sizes.ELTWISE_WORDS == sizes.ELTWISE_ONE_TRIP + 5
