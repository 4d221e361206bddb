"""CPU: the paired internal rounds of the Poseidon2 kernels (poseidon2_arith.hpp: internal_round_pair), compiled for the host with
every bound asserted: one paired step against two plain rounds, the whole permutation against the canonical implementation, over
extreme cells and diagonals (tests/p2_paired_check.cpp) — and the same stand-alone program under the undefined-behaviour
sanitizer, which turns a 64-bit accumulator that wraps into a failure."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "p2_paired_check.cpp")


def _build_and_run(exe, extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-DBX_CHECK_BOUNDS", *extra, f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "p2_paired_check ok" in r.stdout
    return r


def test_paired_rounds_bounds_and_exactness(tmp_path):
    _build_and_run(str(tmp_path / "p2_paired_check"), [])


def test_paired_rounds_no_signed_overflow(tmp_path):
    """-fsanitize=signed-integer-overflow,undefined on the stand-alone program: no accumulator of the paired step wraps"""
    r = _build_and_run(str(tmp_path / "p2_paired_check_ubsan"), ["-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in r.stderr, r.stderr
