"""CPU: the live range of the Poseidon2 permutation (poseidon2_arith.hpp: poseidon2_mix_bounded<DIAG, LO, HI>, the host mirror of the
kernels' poseidon2_mix<LO, HI>), compiled for the host with every bound asserted: the ranged permutations <16, 24> and <0, 8> against
the full one on their live cells, and hash_rows_kernel's chained sponge (<16, 24> ... <0, 8>) against the plain one for 0, 1, 15, 16,
17, 31, 32, 33, 48 and 256 columns, over random and extreme words and the extreme diagonals (tests/p2_live_check.cpp).  The program is
stand-alone and runs under the address and undefined-behaviour sanitizers: a column read past the row or a 64-bit accumulator that
wraps is a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "p2_live_check.cpp")
SANITIZE = ["-fsanitize=address,undefined,signed-integer-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build_and_run(exe, extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-DBX_CHECK_BOUNDS", *extra, f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "p2_live_check ok" in r.stdout
    return r


def test_live_range_bounds_and_exactness(tmp_path):
    _build_and_run(str(tmp_path / "p2_live_check"), [])


def test_live_range_sanitized(tmp_path):
    """-fsanitize=address,undefined,signed-integer-overflow on the stand-alone program"""
    r = _build_and_run(str(tmp_path / "p2_live_check_san"), SANITIZE)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
