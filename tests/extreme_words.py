"""Worst-case operands for the kernels that run on signed, centred Montgomery arithmetic (csrc/poseidon2_arith.hpp,
circuit_dev.hpp, lazy_ext.hpp): a canonical word v is centred to v - P when v > P/2, so the words of largest magnitude are
P//2 (-> +P/2) and P//2 + 1 (-> -P/2), not 0, 1 and P - 1 (-> 0, 1, -1).  No GPU, no library: plain numpy.

`patterns(shape, seed)` yields (name, uint32 array) pairs; `random` is the control and must pass wherever the others do.
"""
import numpy as np

P = 2013265921
MONT_ONE = 268435454  # 2^32 mod P
HALF = P // 2  # 1006632960
EDGE = [0, 1, P - 1, P // 2, P // 2 + 1, P // 2 - 1, MONT_ONE, P - MONT_ONE]
NAMES = ("all_half", "all_half1", "alt_half", "alt_half_rows", "all_pm1", "edge_mix", "random")
EXTREME = NAMES[:-1]


def pattern(name, shape, seed=0):
    """the named pattern as a uint32 array of `shape` (an int or a tuple)"""
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    if name == "all_half":
        return np.full(shape, HALF, np.uint32)
    if name == "all_half1":
        return np.full(shape, HALF + 1, np.uint32)
    if name == "all_pm1":
        return np.full(shape, P - 1, np.uint32)
    if name in ("alt_half", "alt_half_rows"):
        axis = len(shape) - 1 if name == "alt_half" else 0
        idx = np.arange(shape[axis]).reshape([-1 if k == axis else 1 for k in range(len(shape))])
        return np.broadcast_to((HALF + (idx & 1)).astype(np.uint32), shape).copy()
    rng = np.random.default_rng([seed, NAMES.index(name)])
    if name == "edge_mix":
        return np.array(EDGE, np.uint32)[rng.integers(0, len(EDGE), shape)]
    if name == "random":
        return rng.integers(0, P, shape, dtype=np.uint32)
    raise ValueError(name)


def patterns(shape, seed=0):
    for name in NAMES:
        yield name, pattern(name, shape, seed)


def poseidon2_extreme_matrix(rows=256, cols=48):
    """A column-major (cols, rows) matrix for hash_rows (m[:, r] is row r): rows drawn from every extreme word, whole rows of P//2,
    of P//2 + 1 and of P - 1, and rows of their alternation (along the row and from row to row)."""
    m = pattern("edge_mix", (cols, rows), seed=7)
    m[:, 0], m[:, 1], m[:, 2] = HALF, HALF + 1, P - 1
    m[:, 3] = pattern("alt_half", cols)
    m[:, 4] = pattern("alt_half", cols + 1)[1:]
    m[:, 100:140] = pattern("alt_half", (cols, 40))  # whole rows of P//2 and of P//2 + 1 in turn
    assert set(EDGE) == set(m[:, 5:100].ravel().tolist())
    return m
