"""CPU: bx_batch_ratio_products (include/bx_hal.h) — the symbol, its answer to a NULL ctx, the header as C99, the big-integer
reference of tests/ratio_ref.py against itself (definition = invert, multiply, prefix products = the vectorised restatement), and the
compiler's resource report for the scan kernels: no scratch and no spills in the new instantiations, and the figures the existing
ones had before the tile pre-step became an enum.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logup_ref as L  # noqa: E402
import ratio_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = L.P


def test_the_library_exports_the_entry_point_and_python_binds_it():
    """fails on a library built without the feature"""
    from boundless_amd import build, hal

    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "bx_batch_ratio_products")
    assert callable(hal.HipHal.batch_ratio_products)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bx_hal.h")).read(), flags=re.S)
    assert re.search(r"const char\*\s+bx_batch_ratio_products\s*\(bx_ctx\* ctx, bx_buf out_ext, bx_buf nums_ext, bx_buf denoms_ext, size_t count\);", text)


def test_a_null_ctx_is_answered_by_name():
    from boundless_amd import hal

    buf = hal.BxBuf(None, 0)
    assert hal.load_library().bx_batch_ratio_products(None, buf, buf, buf, 1) == b"bx_batch_ratio_products: null ctx"


def test_the_header_still_compiles_as_pedantic_c99():
    src = ('#include "bx_hal.h"\n#include "bx_prover.h"\n'
           "int main(void) { const char* (*f)(bx_ctx*, bx_buf, bx_buf, bx_buf, size_t) = bx_batch_ratio_products; (void)f; return 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_overlap_paragraph_lists_the_entry_point():
    text = open(os.path.join(ROOT, "include", "bx_hal.h")).read()
    para = text[text.index("Operand overlap."):text.index("#ifndef BX_HAL_H")]
    assert "bx_batch_ratio_products" in para and "bx_logup_accumulate" in para


def _rand(seed, n, zeros=()):
    x = np.random.default_rng(seed).integers(0, P, (n, 4), dtype=np.uint32)
    for z in zeros:
        x[z] = 0
    return x.ravel()


@pytest.mark.parametrize("n,count", [(1, 1), (2, 1), (7, 3), (8, 1), (9, 2), (40, 3)])
def test_the_reference_is_invert_multiply_prefix_products(n, count):
    nums = _rand(10 * n + count, n * count, zeros=[n * count // 3] if n > 8 else ())  # a zero numerator too
    dens = _rand(20 * n + count, n * count)
    want = R.ratio_products(nums, dens, count)
    assert np.array_equal(R.by_parts(nums, dens, count), want)
    assert np.array_equal(R.ratio_products_big(nums, dens, count), want)
    # the first sequence by hand
    acc = [1, 0, 0, 0]
    for i in range(n):
        a, d = ([L.decode(int(w)) for w in v[4 * i:4 * i + 4]] for v in (nums, dens))
        acc = L.f4_mul(acc, L.f4_mul(a, L.f4_inv(d)))
        assert [L.decode(int(w)) for w in want[4 * i:4 * i + 4]] == acc
        assert L.f4_mul(L.f4_inv(d), d) == [1, 0, 0, 0]


def test_a_zero_denominator_is_the_factor_zero_in_the_reference():
    n, count = 24, 2
    nums, dens = _rand(1, n * count), _rand(2, n * count, zeros=[5, n + 23])
    for fn in (R.ratio_products, R.by_parts, R.ratio_products_big):
        got = fn(nums, dens, count).reshape(count, n, 4)
        assert np.all(got[0][:5].any(axis=1)) and not got[0][5:].any()
        assert np.all(got[1][:23].any(axis=1)) and not got[1][23:].any()
    x = _rand(3, 16)
    x[x.reshape(-1, 4).any(axis=1).repeat(4) == 0] = 1
    assert np.array_equal(R.ratio_products(x, x, 2).reshape(-1, 4), np.tile(np.array([L.encode(1), 0, 0, 0], np.uint32), (16, 1)))


# ---- the compiler's report ----
FIELDS = ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
# the figures of the commit before this entry point (template arguments then: <Op, bool LOGUP> and <bool SCALE>)
BEFORE = {
    r"scan_lookback_kernelINS_7ScanMulELNS_7ScanPreE0E": (74, 86, 0, 4, 0, 0, 36964),
    r"scan_lookback_kernelINS_7ScanSumELNS_7ScanPreE0E": (63, 80, 0, 4, 0, 0, 36964),
    r"scan_lookback_kernelINS_7ScanSumELNS_7ScanPreE1E": (63, 126, 0, 3, 0, 0, 45412),
    r"binv_ext_kernelILNS_8BinvModeE0E": (50, 124, 0, 4, 0, 0, 36864),
    r"binv_ext_kernelILNS_8BinvModeE1E": (52, 126, 0, 4, 0, 0, 36864),
}
NEW = (r"scan_lookback_kernelINS_7ScanMulELNS_7ScanPreE2E", r"binv_ext_kernelILNS_8BinvModeE2E")


def _fields(report, kernel):
    m = re.search(r"Function Name: \S*" + kernel, report)
    assert m, f"no kernel {kernel} in the report"
    part = report[m.end():]
    return tuple(int(re.search(r"\s" + re.escape(n) + r": (\d+)", part).group(1)) for n in FIELDS)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_scan_kernels_resource_reports(tmp_path):
    from boundless_amd import build

    r = subprocess.run(["hipcc", "-x", "hip"] + build.FLAGS + [build.cuid_flag("scan.hip"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(CSRC, "scan.hip"), "-o", str(tmp_path / "scan.co")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for kernel, want in BEFORE.items():
        assert _fields(r.stderr, kernel) == want, (kernel, dict(zip(FIELDS, _fields(r.stderr, kernel))))
    for kernel in NEW:
        f = dict(zip(FIELDS, _fields(r.stderr, kernel)))
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (kernel, f)
        assert f["LDS Size [bytes/block]"] <= 36964, (kernel, f)  # ONE tile for both loads
