"""CPU: the folded external round constants of the Poseidon2 permutation and the sponge's signed carried capacity
(poseidon2_arith.hpp: p2_fold_consts, p2_build_table, poseidon2_mix_bounded<DIAG, LO, HI, SIGNED_OUT>, the host mirror of the kernels'
poseidon2_mix), compiled for the host with every bound asserted (tests/p2_rcfold_check.cpp): words [0, 288) of the table as they were,
zero blocks zero, M c == rc' for every folded round, the bounded permutation against the plain canonical one over the full range,
<16, 24> (canonical and signed) and <0, 8>, and hash_rows_kernel's chained sponge against the plain one for 0 - 256 columns, over
extreme and random words and parameter sets.  The program is stand-alone and runs under the address and undefined-behaviour
sanitizers: a table word read past its end or a 64-bit accumulator that wraps is a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "p2_rcfold_check.cpp")
SANITIZE = ["-fsanitize=address,undefined,signed-integer-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build_and_run(exe, extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-DBX_CHECK_BOUNDS", *extra, f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "p2_rcfold_check ok" in r.stdout
    return r


def test_rcfold_bounds_and_exactness(tmp_path):
    _build_and_run(str(tmp_path / "p2_rcfold_check"), [])


def test_rcfold_sanitized(tmp_path):
    """-fsanitize=address,undefined,signed-integer-overflow on the stand-alone program"""
    r = _build_and_run(str(tmp_path / "p2_rcfold_check_san"), SANITIZE)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
