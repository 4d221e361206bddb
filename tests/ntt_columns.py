"""Test helper (not collected): the extreme NTT columns shared by tests/test_hal_gpu.py and tests/test_selectable_paths_gpu.py."""
import numpy as np

P = 2013265921
N_ADV = 5


def adversarial_columns(n):
    """Extreme columns of n rows for the NTT kernels (the default kernels carry values in [0, 2P) across their LDS regroupings, so
    the words that sit at the ends of every intermediate range must go through the COMPILED kernels, not only through the host
    check of the arithmetic source): all 0, all P - 1, an impulse at row 0, an impulse at row n - 1, alternating 0 / P - 1."""
    z = np.zeros(n, np.uint32)
    top = np.full(n, P - 1, np.uint32)
    first, last, alt = z.copy(), z.copy(), z.copy()
    first[0] = P - 1
    last[n - 1] = P - 1
    alt[1::2] = P - 1
    return np.concatenate([z, top, first, last, alt])
