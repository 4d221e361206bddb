"""GPU: the folded external round constants (poseidon2.hip: sbox_half_folded, the table region behind the paired rounds' constants) and the
sponge's signed carried capacity (poseidon2_mix<16, 24, true>), bit for bit against the C oracle.  hash_rows over 1 / 65 / 300 rows (one
lane, a partial wave behind a full one, a ragged second workgroup) and 0 .. 64 columns (the empty row, a padded, a full last block, one
to four chained permutations); a Merkle build over 2^12 leaves scheduled so that hash_fold_deep_kernel<2> (4096 -> 1024), hash_fold_kernel
(1024 -> 512) and the quad kernel (512 -> 1) all run.  Everything with the built-in parameters and with a random set installed through
bx_poseidon2_set_params (the folded region must follow a parameter change), on all-zero, all-(P-1) and random matrices."""
import numpy as np
import pytest

from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu
P = ol.P
ROWS = (1, 65, 300)
COLS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 64)
TREE_ROWS, TREE_COLS = 1 << 12, 17  # a loop block and a padded peeled one per leaf
FOLD_DEFAULTS = {"fold_quad": 1, "fold_deep": 2, "fold_deep_min_lanes": 1 << 17, "fold_fuse_below": 1 << 17}
FOLD_ALL_KERNELS = {"fold_quad": 1, "fold_deep": 2, "fold_deep_min_lanes": 1, "fold_fuse_below": 512}  # hal.hip: merkle_fold_layers
MATRICES = ("zeros", "minus_ones", "random")


def c(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


@pytest.fixture(scope="module")
def hal():
    from boundless_amd.hal import HipHal

    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(scope="module", params=["builtin", "random"])
def params(request, hal, oracle):
    """the parameter set under test, installed on the device and in the oracle; the built-in one is put back afterwards"""
    if request.param == "builtin":
        yield request.param
        return
    rc0, d0 = hal.poseidon2_get_params()
    rng = np.random.default_rng(29)
    rc1, d1 = rng.integers(0, P, 213, dtype=np.uint32), rng.integers(0, P, 24, dtype=np.uint32)
    try:
        hal.poseidon2_set_params(rc1, d1)
        oracle.bxo_poseidon2_set_params(c(rc1), c(d1))
        yield request.param
    finally:
        hal.poseidon2_set_params(rc0, d0)
        oracle.bxo_poseidon2_set_params(c(rc0), c(d0))


def matrix(kind, n, seed):
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "minus_ones":
        return np.full(n, P - 1, np.uint32)
    return ol.random_elems(np.random.default_rng(seed), n)


def oracle_hash_rows(oracle, x, rows, cols):
    ref = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(ref, x if cols else np.zeros(1, np.uint32), rows, cols)
    return ref


def device_hash_rows(hal, x, rows, cols):
    out = hal.alloc_digest(rows)
    out.copy_from(np.full(8 * rows, 0xFFFFFFFF, np.uint32))
    src = hal.copy_from(x) if cols else hal.alloc(1).slice(0, 0)  # no columns: an empty matrix, the digest of the empty row
    hal.hash_rows(out, src)
    return out.view().copy()


@pytest.mark.parametrize("kind", MATRICES)
def test_hash_rows(hal, oracle, params, kind):
    for rows in ROWS:
        for cols in COLS:
            x = matrix(kind, rows * cols, 1000 * rows + cols)
            got, want = device_hash_rows(hal, x, rows, cols), oracle_hash_rows(oracle, x, rows, cols)
            assert np.array_equal(got, want), (params, kind, rows, cols)
            assert int(got.max()) < P


@pytest.mark.parametrize("kind", MATRICES)
def test_merkle_build_every_fold_kernel(hal, oracle, params, kind):
    rows, cols = TREE_ROWS, TREE_COLS
    x = matrix(kind, rows * cols, 4096)
    ref = np.zeros(16 * rows, np.uint32)
    ref[8 * rows:] = oracle_hash_rows(oracle, x, rows, cols)
    size = rows
    while size > 1:
        oracle.bxo_hash_fold(ref, size, size // 2)
        size //= 2
    try:
        for name, value in FOLD_ALL_KERNELS.items():
            hal.set_tunable(name, value)
        nodes = hal.alloc_digest(2 * rows)
        nodes.copy_from(np.zeros(16 * rows, np.uint32))
        hal.merkle_build(nodes, hal.copy_from(x), rows)
        assert np.array_equal(nodes.view()[8:], ref[8:]), (params, kind)
    finally:
        for name, value in FOLD_DEFAULTS.items():
            hal.set_tunable(name, value)
