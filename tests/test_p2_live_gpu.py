"""GPU: the live range of the Poseidon2 permutation (poseidon2.hip: poseidon2_mix<LO, HI>) and the tables it reads through scalar loads,
bit for bit against the C oracle.  hash_rows_kernel runs <16, 24> for every block of 16 columns but the last and <0, 8> for the last,
which is peeled and loads under a guard: 16 / 32 / 48 columns make it a full block, 17 / 31 / 33 a padded one behind one or two loop
blocks, 1 / 15 a padded one alone, 0 the empty row; 63 / 65 / 257 rows are partial waves; the same at every hash_rows_block.  Every fold
kernel runs <0, 8>: the Merkle folds at the smallest sizes that select each of them, and hash_fold_indexed.  One run after
bx_poseidon2_set_params with an extreme diagonal, so that the tables the kernels load are the derived ones."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle_lib as ol

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extreme_words import poseidon2_extreme_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
P = ol.P
ROWS = (1, 63, 64, 65, 257)
COLS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 256)
FOLD_DEFAULTS = {"fold_quad": 1, "fold_deep": 2, "fold_deep_min_lanes": 1 << 17, "fold_fuse_below": 1 << 17}


@pytest.fixture(scope="module")
def hal():
    from boundless_amd.hal import HipHal

    h = HipHal(0)
    yield h
    h.close()


def rnd(seed, n):
    return ol.random_elems(np.random.default_rng(seed), n)


def c(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def oracle_hash_rows(oracle, x, rows, cols):
    ref = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(ref, x if cols else np.zeros(1, np.uint32), rows, cols)
    return ref


def device_hash_rows(hal, x, rows, cols):
    out = hal.alloc_digest(rows)
    out.copy_from(np.zeros(8 * rows, np.uint32))
    src = hal.copy_from(x) if cols else hal.alloc(1).slice(0, 0)  # no columns: an empty matrix, the digest of the empty row
    hal.hash_rows(out, src)
    return out.view().copy()


@pytest.fixture(scope="module")
def row_cases(oracle):
    """{(rows, cols): (matrix, the oracle's digests)}: computed once, shared by the three block sizes, not modified"""
    cases = {}
    for rows in ROWS:
        for cols in COLS:
            x = rnd(rows * 31 + cols, rows * cols)
            ref = oracle_hash_rows(oracle, x, rows, cols)
            x.setflags(write=False)
            ref.setflags(write=False)
            cases[rows, cols] = (x, ref)
    return cases


@pytest.mark.parametrize("block", [256, 64, 128])
@pytest.mark.parametrize("rows", ROWS)
def test_hash_rows_shapes(hal, row_cases, rows, block):
    try:
        hal.set_tunable("hash_rows_block", block)
        for cols in COLS:
            x, ref = row_cases[rows, cols]
            assert np.array_equal(device_hash_rows(hal, x, rows, cols), ref), (rows, cols, block)
    finally:
        hal.set_tunable("hash_rows_block", 256)


def test_extreme_words_through_hash_rows(hal, oracle):
    rows, cols = 256, 48
    x = c(poseidon2_extreme_matrix(rows, cols).reshape(-1))
    assert np.array_equal(device_hash_rows(hal, x, rows, cols), oracle_hash_rows(oracle, x, rows, cols))


def test_extreme_words_padded_last_block(hal, oracle):
    """the same matrix cut to 33 columns: two loop blocks of extreme words and a padded peeled block of one column"""
    rows, cols = 256, 33
    x = c(poseidon2_extreme_matrix(rows, 48)[:cols].reshape(-1))
    assert np.array_equal(device_hash_rows(hal, x, rows, cols), oracle_hash_rows(oracle, x, rows, cols))


def merkle_reference(oracle, x, rows, cols):
    ref = np.zeros(16 * rows, np.uint32)
    ref[8 * rows:] = oracle_hash_rows(oracle, x, rows, cols)
    size = rows
    while size > 1:
        oracle.bxo_hash_fold(ref, size, size // 2)
        size //= 2
    return ref


@pytest.fixture(scope="module")
def tree_2048(oracle):
    """(matrix, the oracle's tree) of 2048 rows x 17 columns (a loop block and a padded peeled one): computed once, shared, not modified"""
    rows, cols = 2048, 17
    x = rnd(2049, rows * cols)
    ref = merkle_reference(oracle, x, rows, cols)
    ref.setflags(write=False)
    return x, ref


# the smallest schedules that reach each fold kernel on a 2048-leaf tree (hal.hip: merkle_fold_layers), as in test_p2_paired_gpu.py:
#   layer: one hash_fold_kernel launch per layer down to the root;  deep2 / deep3: hash_fold_deep_kernel<2> / <3> from 2048 inputs (512 /
#   256 lanes: two blocks / one) down to a single lane;  small_quad / small_lane: the fused small-layer launch, four lanes per node
#   (hash_fold_quad_kernel, which keeps the full permutation) and one (hash_fold_multi_kernel);  defaults: the schedule as shipped
FOLD_KERNELS = {
    "layer": {"fold_deep": 1, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "deep2": {"fold_deep": 2, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "deep3": {"fold_deep": 3, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "small_quad": {"fold_quad": 1},
    "small_lane": {"fold_quad": 0},
    "defaults": {},
}


@pytest.mark.parametrize("kernel", list(FOLD_KERNELS))
def test_fold_kernels(hal, tree_2048, kernel):
    x, ref = tree_2048
    rows = 2048
    try:
        for name, value in FOLD_KERNELS[kernel].items():
            hal.set_tunable(name, value)
        nodes = hal.alloc_digest(2 * rows)
        nodes.copy_from(np.zeros(16 * rows, np.uint32))
        hal.merkle_build(nodes, hal.copy_from(x), rows)
        assert np.array_equal(nodes.view()[8:], ref[8:])
    finally:
        for name, value in FOLD_DEFAULTS.items():
            hal.set_tunable(name, value)


def check_hash_fold(hal, oracle, outputs, seed):
    host = np.zeros(8 * 4 * outputs, np.uint32)
    host[8 * 2 * outputs:] = rnd(seed, 8 * 2 * outputs)
    io = hal.copy_from(host)
    hal.hash_fold(io, 2 * outputs, outputs)
    ref = host.copy()
    oracle.bxo_hash_fold(ref, 2 * outputs, outputs)
    assert np.array_equal(io.view()[8 * outputs:], ref[8 * outputs:])


@pytest.mark.parametrize("outputs", [1, 65, 300])
def test_hash_fold_single_layer(hal, oracle, outputs):
    """hash_fold_kernel through Hal::hash_fold: one lane, a partial wave behind a full one, two blocks"""
    check_hash_fold(hal, oracle, outputs, 100 + outputs)


def test_hash_fold_extreme_digests(hal, oracle):
    """digests of extreme words through hash_fold_kernel"""
    outputs = 96
    host = np.zeros(8 * 4 * outputs, np.uint32)
    host[8 * 2 * outputs:] = c(poseidon2_extreme_matrix(256, 48).reshape(-1)[:8 * 2 * outputs])
    io = hal.copy_from(host)
    hal.hash_fold(io, 2 * outputs, outputs)
    ref = host.copy()
    oracle.bxo_hash_fold(ref, 2 * outputs, outputs)
    assert np.array_equal(io.view()[8 * outputs:], ref[8 * outputs:])


@pytest.mark.parametrize("n,count", [(1, 1), (37, 300)])
def test_hash_fold_indexed(hal, oracle, n, count):
    from boundless_amd import image

    lib = image._lib()
    rng = np.random.default_rng(1000 + n)
    digs = ol.random_elems(rng, (n, 8))
    sel = rng.integers(0, n, (count, 2), dtype=np.uint32)
    d_in, d_sel, d_out = hal.copy_from(digs.reshape(-1)), hal.copy_from(sel.reshape(-1)), hal.alloc_digest(count)
    hal._check(lib.bx_hash_fold_indexed(hal.ctx, d_out.raw, d_in.raw, d_sel.raw, count))
    got = d_out.view().reshape(count, 8)
    for j in range(count):
        want = np.zeros(8, np.uint32)
        oracle.bxo_hash_pair(want, c(digs[sel[j, 0]]), c(digs[sel[j, 1]]))
        assert np.array_equal(got[j], want), j


def extreme_diagonal():
    """canonical diagonal whose derived constants sit at the ends of the centred range: A_i = d_i R^2 = +(P-1)/2 and -(P-1)/2 in
    turn, and cell 0's multiplier d_0 R = +(P-1)/2 (the "A = +-(P-1)/2" diagonal of tests/p2_live_check.cpp)"""
    rinv = pow(1 << 32, -1, P)
    pos, neg = (P - 1) // 2 * rinv * rinv % P, (P + 1) // 2 * rinv * rinv % P
    d = np.array([pos if i & 1 else neg for i in range(24)], np.uint32)
    d[0] = (P - 1) // 2 * rinv % P
    assert (int(d[1]) << 64) % P == (P - 1) // 2 and (int(d[2]) << 64) % P == (P + 1) // 2 and (int(d[0]) << 32) % P == (P - 1) // 2
    return d


def test_set_params_with_an_extreme_diagonal(hal, oracle):
    """the scalar-loaded tables (E, A and the diagonal) are the ones poseidon2_upload_params derives from the diagonal that was set:
    hash_rows with a loop block and a peeled one, a fold layer, and a deep fold (constants fetched per permutation of a subtree)"""
    rc0, d0 = hal.poseidon2_get_params()
    rc1 = np.random.default_rng(6).integers(0, P, 213, dtype=np.uint32)
    d1 = extreme_diagonal()
    try:
        hal.poseidon2_set_params(rc1, d1)
        oracle.bxo_poseidon2_set_params(c(rc1), c(d1))
        rows, cols = 65, 33
        x = rnd(19, rows * cols)
        assert np.array_equal(device_hash_rows(hal, x, rows, cols), oracle_hash_rows(oracle, x, rows, cols))
        check_hash_fold(hal, oracle, 65, 20)
        rows, cols = 256, 3
        x = rnd(21, rows * cols)
        ref = merkle_reference(oracle, x, rows, cols)
        for name, value in FOLD_KERNELS["deep2"].items():
            hal.set_tunable(name, value)
        nodes = hal.alloc_digest(2 * rows)
        nodes.copy_from(np.zeros(16 * rows, np.uint32))
        hal.merkle_build(nodes, hal.copy_from(x), rows)
        assert np.array_equal(nodes.view()[8:], ref[8:])
    finally:
        for name, value in FOLD_DEFAULTS.items():
            hal.set_tunable(name, value)
        hal.poseidon2_set_params(rc0, d0)
        oracle.bxo_poseidon2_set_params(c(rc0), c(d0))
