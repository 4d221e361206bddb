"""CPU: the reference of the LogUp helpers (tests/logup_ref.py) stands on its own feet, and the five entry points are part of the
declared, exported C ABI."""
import ctypes
import fnmatch
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logup_ref as R  # noqa: E402

NAMES = ["bx_batch_invert_ext", "bx_batch_invert_elem", "bx_prefix_sums", "bx_batch_prefix_sums", "bx_logup_accumulate"]


def test_reference_constants():
    assert R.P == 15 * 2**27 + 1
    assert R.encode(1) == 2**32 % R.P == 268435454
    assert R.decode(R.encode(123456789)) == 123456789
    x3 = [0, 0, 0, 1]
    assert R.f4_mul(x3, [0, 1, 0, 0]) == [R.P - 11, 0, 0, 0]  # X^3 * X = X^4 = -11


def test_reference_base_field_inverse_times_input_is_one():
    rng = np.random.default_rng(2024)
    x = rng.integers(1, R.P, 1000, dtype=np.uint32)
    inv = R.batch_invert_elem(x)
    assert np.all(inv < R.P)
    assert np.all(R.elem_mul(x, inv) == R.encode(1))
    assert np.array_equal(R.batch_invert_elem_big(x), inv)
    assert R.batch_invert_elem(np.zeros(3, np.uint32)).tolist() == [0, 0, 0]


def test_reference_ext_inverse_times_input_is_one():
    rng = np.random.default_rng(2025)
    x = rng.integers(0, R.P, 4000, dtype=np.uint32)
    x[4 * 7:4 * 8] = 0  # one zero element: maps to zero
    x[4 * 9 + 1:4 * 10] = 0  # an element of the base field
    inv = R.batch_invert_ext(x)
    assert np.all(inv < R.P)
    prod = R.ext_mul(x, inv).reshape(-1, 4)
    want = np.tile(np.array([R.encode(1), 0, 0, 0], dtype=np.uint32), (1000, 1))
    want[7] = 0
    assert np.array_equal(prod, want)
    assert not inv[4 * 7:4 * 8].any()
    assert np.array_equal(R.batch_invert_ext_big(x), inv)
    # inverting twice returns the input, zeros staying zero
    assert np.array_equal(R.batch_invert_ext(inv), x)


def test_reference_fused_definition_is_the_three_steps():
    rng = np.random.default_rng(7)
    n, count = 37, 3
    d = rng.integers(0, R.P, 4 * n * count, dtype=np.uint32)
    d[4 * 5:4 * 6] = 0
    m = rng.integers(0, R.P, n * count, dtype=np.uint32)
    want = R.logup_accumulate(d, m, count)
    assert np.array_equal(R.batch_prefix_sums(R.scale_ext(R.batch_invert_ext(d), m), count), want)
    assert np.array_equal(R.logup_accumulate_big(d, m, count), want)
    # the running sum written out by hand for the first sequence
    acc = [0, 0, 0, 0]
    for i in range(n):
        term = R.f4_scale(R.f4_inv([R.decode(int(w)) for w in d[4 * i:4 * i + 4]]), R.decode(int(m[i])))
        acc = R.f4_add(acc, term)
        assert [R.decode(int(w)) for w in want[4 * i:4 * i + 4]] == acc


def test_reference_product_agrees_with_the_c_oracle(oracle):
    """The C oracle's binding has no bare Fp4 product, but its prefix_products over two elements is one: io[1] = io[0] * io[1]."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, R.P, 4 * 200, dtype=np.uint32)
    b = rng.integers(0, R.P, 4 * 200, dtype=np.uint32)
    want = R.ext_mul(a, b).reshape(-1, 4)
    for i in range(200):
        io = np.concatenate([a[4 * i:4 * i + 4], b[4 * i:4 * i + 4]]).astype(np.uint32)
        oracle.bxo_prefix_products(io, 2)
        assert np.array_equal(io[4:], want[i]), i
    # and a whole running product
    seq = a.copy()
    oracle.bxo_prefix_products(seq, 200)
    assert np.array_equal(seq, R.batch_prefix_products(a))


def _header_text():
    text = open(os.path.join(ROOT, "include", "bx_hal.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_in_the_header():
    decl = set(re.findall(r"\bconst char\*\s+(bx_[a-z0-9_]+)\s*\(", _header_text()))
    missing = [n for n in NAMES if n not in decl]
    assert not missing, f"not declared in include/bx_hal.h: {missing}"


def test_entry_points_are_covered_by_the_export_map():
    text = open(os.path.join(ROOT, "boundless_amd", "csrc", "exports.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"global:(.*?)local:", text, flags=re.S)
    assert m, "exports.map has no global: section"
    patterns = [p.strip() for p in m.group(1).split(";") if p.strip()]
    for n in NAMES:
        assert any(fnmatch.fnmatchcase(n, p) for p in patterns), f"{n} matches no global pattern of exports.map ({patterns})"


def test_library_exports_the_entry_points():
    """Fails on a library built without the feature: the symbols do not exist."""
    from boundless_amd import build

    lib = ctypes.CDLL(build.build(verbose=False))
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, f"declared but not exported: {missing}"


def test_python_binding_has_the_methods():
    from boundless_amd import hal

    for n in NAMES:
        assert callable(getattr(hal.HipHal, n[len("bx_"):])), n


def test_null_ctx_is_refused_with_a_message():
    """No GPU needed: every entry point answers a null ctx with its own error string."""
    from boundless_amd import hal

    lib = hal.load_library()
    buf = hal.BxBuf(None, 0)
    assert b"bx_batch_invert_ext" in lib.bx_batch_invert_ext(None, buf)
    assert b"bx_batch_invert_elem" in lib.bx_batch_invert_elem(None, buf)
    assert b"bx_prefix_sums" in lib.bx_prefix_sums(None, buf)
    assert b"bx_batch_prefix_sums" in lib.bx_batch_prefix_sums(None, buf, 1)
    assert b"bx_logup_accumulate" in lib.bx_logup_accumulate(None, buf, buf, buf, 1)


def test_headers_still_compile_as_pedantic_c99():
    src = '#include "bx_hal.h"\n#include "bx_prover.h"\nint main(void) { const char* (*f)(bx_ctx*, bx_buf, bx_buf, bx_buf, size_t) = bx_logup_accumulate; (void)f; return 0; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
