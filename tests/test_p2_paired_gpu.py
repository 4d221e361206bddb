"""GPU: every Poseidon2 kernel that runs the paired internal rounds (poseidon2.hip: poseidon2_mix), bit for bit against the C oracle:
hash_rows over the shapes that separate a single permutation, the chained sponge with a padded tail and a partial wave; the Merkle
folds at the smallest sizes that select each fold kernel; the matrix of extreme words; and a diagonal from the extreme set of
tests/p2_paired_check.cpp set through bx_poseidon2_set_params, whose derived tables the kernels then read."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle_lib as ol

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extreme_words import poseidon2_extreme_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
P = ol.P
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


def check_hash_rows(hal, oracle, x, rows, cols):
    out = hal.alloc_digest(rows)
    out.copy_from(np.zeros(8 * rows, np.uint32))
    src = hal.copy_from(x) if cols else hal.alloc(1).slice(0, 0)  # no columns: an empty matrix, the digest of the empty row
    hal.hash_rows(out, src)
    ref = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(ref, x if cols else np.zeros(1, np.uint32), rows, cols)
    assert np.array_equal(out.view(), ref)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_hash_rows_shapes(hal, oracle, rows):
    """cols 0 and 1..16: one permutation (0: of the zero state); 17..32: two, the second padded; 33, 256: chained; rows 63 / 65 / 257:
    a partial wave, alone and behind full ones"""
    for cols in (0, 1, 15, 16, 17, 32, 33, 256):
        check_hash_rows(hal, oracle, rnd(rows * 31 + cols, rows * cols), rows, cols)


def merkle_reference(oracle, x, rows, cols):
    ref = np.zeros(16 * rows, np.uint32)
    leaves = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(leaves, x, rows, cols)
    ref[8 * rows:] = leaves
    size = rows
    while size > 1:
        oracle.bxo_hash_fold(ref, size, size // 2)
        size //= 2
    return ref


@pytest.fixture(scope="module")
def tree_2048(oracle):
    """(matrix, the oracle's tree) of 2048 rows x 3 columns: computed once, shared, not modified"""
    rows, cols = 2048, 3
    x = rnd(2048, rows * cols)
    ref = merkle_reference(oracle, x, rows, cols)
    ref.setflags(write=False)
    return x, ref


# the smallest schedules that reach each fold kernel on a 2048-leaf tree (hal.hip: merkle_fold_layers):
#   layer: one hash_fold_kernel launch per layer down to the root;  deep2 / deep3: hash_fold_deep_kernel<2> / <3> from 2048 inputs (512 /
#   256 lanes: two blocks / one) down to a single lane;  small_quad / small_lane: the fused small-layer launch, four lanes per node and one
FOLD_KERNELS = {
    "layer": {"fold_deep": 1, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "deep2": {"fold_deep": 2, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "deep3": {"fold_deep": 3, "fold_deep_min_lanes": 1, "fold_fuse_below": 0},
    "small_quad": {"fold_quad": 1},
    "small_lane": {"fold_quad": 0},
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


@pytest.mark.parametrize("outputs", [1, 65, 300])
def test_hash_fold_single_layer(hal, oracle, outputs):
    """hash_fold_kernel through Hal::hash_fold: one lane, a partial wave behind a full one, two blocks"""
    host = np.zeros(8 * 4 * outputs, np.uint32)
    host[8 * 2 * outputs:] = rnd(outputs, 8 * 2 * outputs)
    io = hal.copy_from(host)
    hal.hash_fold(io, 2 * outputs, outputs)
    ref = host.copy()
    oracle.bxo_hash_fold(ref, 2 * outputs, outputs)
    assert np.array_equal(io.view()[8 * outputs:], ref[8 * outputs:])


@pytest.mark.parametrize("n,count", [(1, 1), (37, 300)])
def test_hash_fold_indexed(hal, oracle, n, count):
    from boundless_amd import image

    lib = image._lib()
    rng = np.random.default_rng(n)
    digs = ol.random_elems(rng, (n, 8))
    sel = rng.integers(0, n, (count, 2), dtype=np.uint32)
    d_in, d_sel, d_out = hal.copy_from(digs.reshape(-1)), hal.copy_from(sel.reshape(-1)), hal.alloc_digest(count)
    hal._check(lib.bx_hash_fold_indexed(hal.ctx, d_out.raw, d_in.raw, d_sel.raw, count))
    got = d_out.view().reshape(count, 8)
    for j in range(count):
        want = np.zeros(8, np.uint32)
        oracle.bxo_hash_pair(want, c(digs[sel[j, 0]]), c(digs[sel[j, 1]]))
        assert np.array_equal(got[j], want), j


def test_extreme_words_through_hash_rows(hal, oracle):
    rows, cols = 256, 48
    check_hash_rows(hal, oracle, c(poseidon2_extreme_matrix(rows, cols).reshape(-1)), rows, cols)


def extreme_diagonal():
    """canonical diagonal whose derived constants sit at the ends of the centred range: A_i = d_i R^2 = +(P-1)/2 and -(P-1)/2 in
    turn, and cell 0's multiplier d_0 R = +(P-1)/2 (the "A = +-(P-1)/2" diagonal of tests/p2_paired_check.cpp)"""
    rinv = pow(1 << 32, -1, P)
    pos, neg = (P - 1) // 2 * rinv * rinv % P, (P + 1) // 2 * rinv * rinv % P
    d = np.array([pos if i & 1 else neg for i in range(24)], np.uint32)
    d[0] = (P - 1) // 2 * rinv % P
    assert (int(d[1]) << 64) % P == (P - 1) // 2 and (int(d[2]) << 64) % P == (P + 1) // 2 and (int(d[0]) << 32) % P == (P - 1) // 2
    return d


def test_set_params_with_an_extreme_diagonal(hal, oracle):
    rc0, d0 = hal.poseidon2_get_params()
    rc1 = np.random.default_rng(5).integers(0, P, 213, dtype=np.uint32)
    d1 = extreme_diagonal()
    try:
        hal.poseidon2_set_params(rc1, d1)
        oracle.bxo_poseidon2_set_params(c(rc1), c(d1))
        check_hash_rows(hal, oracle, rnd(17, 64 * 17), 64, 17)
        host = np.zeros(8 * 4 * 65, np.uint32)
        host[8 * 2 * 65:] = rnd(18, 8 * 2 * 65)
        io = hal.copy_from(host)
        hal.hash_fold(io, 130, 65)
        ref = host.copy()
        oracle.bxo_hash_fold(ref, 130, 65)
        assert np.array_equal(io.view()[8 * 65:], ref[8 * 65:])
    finally:
        hal.poseidon2_set_params(rc0, d0)
        oracle.bxo_poseidon2_set_params(c(rc0), c(d0))
