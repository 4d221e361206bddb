"""GPU parity of the kernel paths that only a tunable (bx_set_tunable / BX_TUNABLES), a pointer alignment or a size
selects — the paths the default settings and the power-of-two sizes of tests/test_hal_gpu.py never take.  Every comparison is
bit-exact: against the C oracle, and for the `sha-256` suite against tests/sha256_ref.py.  A test that sets a tunable puts the
default (csrc/ctx.hpp, csrc/ntt_plan.hpp) back in a `finally` block, so no test sees a setting left over from another."""
import contextlib
import os
import sys

import numpy as np
import pytest

from oracle import oracle_lib as ol

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sha256_ref  # noqa: E402
from extreme_words import HALF, MONT_ONE, pattern, poseidon2_extreme_matrix  # noqa: E402
from ntt_columns import adversarial_columns  # noqa: E402

pytestmark = pytest.mark.gpu
P = ol.P
SEG = 1 << 15  # coefficients per workgroup of the batch_evaluate_any kernels (poly.hip: EV_T * EV_K)

HALF_W, HALF1_W = np.full(4, HALF, np.uint32), np.full(4, HALF + 1, np.uint32)
ONE_W, ZERO_W = np.array([MONT_ONE, 0, 0, 0], np.uint32), np.zeros(4, np.uint32)
MINUS_ONE_W = np.array([P - MONT_ONE, 0, 0, 0], np.uint32)
COEFF_PATTERNS = ("random", "edge_mix", "alt_half")


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


@contextlib.contextmanager
def tuned(hal, settings, defaults):
    """set tunables for the body, put the given defaults (csrc/ctx.hpp) back afterwards, also when the body raises"""
    try:
        for name, value in settings.items():
            hal.set_tunable(name, value)
        yield
    finally:
        for name, value in defaults.items():
            hal.set_tunable(name, value)


def bitrev_perm(n):
    """perm[j] = bitrev_n(j), built by doubling: rev_{k+1} = [2 rev_k, 2 rev_k + 1]"""
    r = np.zeros(1, np.int64)
    for _ in range(n):
        r = np.concatenate([2 * r, 2 * r + 1])
    return r


# ------------------------------------------------------------------ a. batch_evaluate_any
EVAL_POINTS = [ZERO_W, ONE_W, MINUS_ONE_W, HALF_W, HALF1_W, rnd(11, 4)]  # the set of test_batch_evaluate_any_extreme_operands
EVAL_XS = c(np.concatenate(EVAL_POINTS + EVAL_POINTS))
EVAL_WHICH = np.array([0] * 6 + [1] * 6, np.uint32)  # every point on both polynomials
NPOLY = 2
_eval_cases = {}


def eval_case(oracle, name, size, xs=EVAL_XS, which=EVAL_WHICH, keep=True):
    """(natural-order coefficients of NPOLY polynomials, the oracle's Horner evaluations): computed once per (pattern, size)"""
    key = (name, size)
    if key in _eval_cases:
        return _eval_cases[key]
    coeffs = c(pattern(name, (NPOLY, size), seed=size).reshape(-1))
    ref = np.zeros(4 * which.size, np.uint32)
    oracle.bxo_batch_evaluate_any(coeffs, size, c(which), c(xs), ref, which.size)
    coeffs.setflags(write=False), ref.setflags(write=False)
    if keep:
        _eval_cases[key] = (coeffs, ref)
    return coeffs, ref


def stored_form(coeffs, size, bitrev):
    """what the device holds: the natural array, or position j holding the coefficient of x^bitrev(j)"""
    if not bitrev:
        return coeffs
    return c(coeffs.reshape(NPOLY, size)[:, bitrev_perm(size.bit_length() - 1)].reshape(-1))


def evaluate(hal, d_coeffs, bitrev, xs=EVAL_XS, which=EVAL_WHICH):
    out = hal.alloc(4 * which.size)
    call = hal.batch_evaluate_any_bitrev if bitrev else hal.batch_evaluate_any
    call(d_coeffs, NPOLY, hal.copy_from(which), hal.copy_from(xs), out)
    return out.view()


@pytest.mark.parametrize("name", COEFF_PATTERNS)
@pytest.mark.parametrize("bitrev", [False, True], ids=["natural", "bitrev"])
@pytest.mark.parametrize("n", [15, 16, 18])
def test_evaluate_any_dword_kernel_on_whole_segments(hal, oracle, n, bitrev, name):
    """eval_x4 = 0 sends whole 2^15-coefficient segments through eval_partial_kernel: its whole-segment loop, the per-segment factor
    x^(seg 2^15) for seg > 0 (2^16: one, 2^18: seven), and its bit-reversed branch — rev7 / rev8 table indices and the exponent
    rev(seg), which has no bits at 2^15, one at 2^16 and three at 2^18."""
    size = 1 << n
    coeffs, ref = eval_case(oracle, name, size)
    with tuned(hal, {"eval_x4": 0}, {"eval_x4": 1}):
        got = evaluate(hal, hal.copy_from(stored_form(coeffs, size, bitrev)), bitrev)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name", COEFF_PATTERNS)
@pytest.mark.parametrize("bitrev", [False, True], ids=["natural", "bitrev"])
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("n", [15, 17])
def test_evaluate_any_on_a_slice_that_is_only_word_aligned(hal, oracle, n, off, bitrev, name):
    """Default tunables: a coefficient buffer that does not start on a 16-byte boundary (a slice at an odd word offset) cannot take the
    16-byte loads of the x4 kernel and falls back to the dword kernel.  The words around the slice and around `out` stay."""
    size = 1 << n
    coeffs, ref = eval_case(oracle, name, size)
    pad = 8
    rng = np.random.default_rng(n * 10 + off)
    host = rng.integers(0, 1 << 32, off + NPOLY * size + pad, dtype=np.uint32)
    host[off:off + NPOLY * size] = stored_form(coeffs, size, bitrev)
    out_host = rng.integers(0, 1 << 32, 8 + ref.size + pad, dtype=np.uint32)  # `out` keeps its 16-byte alignment (ext elements)
    whole, out_whole = hal.copy_from(host), hal.copy_from(out_host)
    d_coeffs, out = whole.slice(off, NPOLY * size), out_whole.slice(8, ref.size)
    assert d_coeffs.raw.dptr % 16 != 0 and out.raw.dptr % 16 == 0
    call = hal.batch_evaluate_any_bitrev if bitrev else hal.batch_evaluate_any
    call(d_coeffs, NPOLY, hal.copy_from(EVAL_WHICH), hal.copy_from(EVAL_XS), out)
    got = out_whole.view()
    assert np.array_equal(got[8:8 + ref.size], ref)
    assert np.array_equal(got[:8], out_host[:8]) and np.array_equal(got[8 + ref.size:], out_host[8 + ref.size:]), "around out"
    assert np.array_equal(whole.view(), host), "the coefficients and the words around them"


@pytest.mark.parametrize("name", COEFF_PATTERNS)
@pytest.mark.parametrize("size", [100, 257, SEG - 1, SEG + 1, 40000, 3 * SEG + 77])
def test_evaluate_any_ragged_sizes(hal, oracle, size, name):
    """Default tunables, natural order: a poly_size that is no multiple of 2^15 takes the dword kernel with a ragged last segment —
    alone (100, 257, 2^15 - 1), one coefficient long behind a whole one (2^15 + 1), and behind one and three whole ones."""
    coeffs, ref = eval_case(oracle, name, size)
    assert np.array_equal(evaluate(hal, hal.copy_from(coeffs), False), ref)


@pytest.mark.parametrize("name", COEFF_PATTERNS)
@pytest.mark.parametrize("segs", [3, 5])
def test_evaluate_any_x4_kernel_with_a_segment_count_that_is_no_power_of_two(hal, oracle, segs, name):
    """Default tunables, aligned, whole segments: the x4 kernels.  eval_tables_kernel rounds the number of segment powers up to a
    power of two; three and five segments use a part of that table."""
    size = segs * SEG
    coeffs, ref = eval_case(oracle, name, size)
    d_coeffs = hal.copy_from(coeffs)
    assert d_coeffs.raw.dptr % 16 == 0
    assert np.array_equal(evaluate(hal, d_coeffs, False), ref)


@pytest.mark.parametrize("name", COEFF_PATTERNS)
def test_evaluate_any_beyond_the_x4_range(hal, oracle, name):
    """2^25 coefficients are 1024 segments, more than the 512 the x4 tables hold: default tunables take the dword kernel, natural and
    bit-reversed (ten segment bits).  Two evaluations: a random point on polynomial 0, all-(P//2 + 1) on polynomial 1."""
    n, size = 25, 1 << 25
    xs, which = c(np.concatenate([rnd(12, 4), HALF1_W])), np.array([0, 1], np.uint32)
    coeffs, ref = eval_case(oracle, name, size, xs, which, keep=False)
    d = hal.copy_from(coeffs)
    assert np.array_equal(evaluate(hal, d, False, xs, which), ref), "natural"
    d.copy_from(stored_form(coeffs, size, True))
    assert np.array_equal(evaluate(hal, d, True, xs, which), ref), "bit-reversed"
    d.free()


def test_evaluate_sizes_outside_an_entry_points_range_are_refused(hal):
    """Checked on the host before any launch: the pointer form takes [2^15, 2^24] only (its pointers are never read here), the
    bit-reversed form powers of two only."""
    from boundless_amd.hal import HalError

    ptrs = hal.copy_from(np.array([0x1000, 0], np.uint32))  # any 8-byte-aligned address: the call returns before reading it
    flags, xs, out = hal.copy_from(np.zeros(1, np.uint32)), hal.copy_from(rnd(1, 4)), hal.alloc_zeroed(4)
    with pytest.raises(HalError, match=r"\[2\^15, 2\^24\]"):
        hal.batch_evaluate_ptrs(ptrs, flags, 1 << 25, xs, out)
    with pytest.raises(HalError, match="power of two"):
        hal.batch_evaluate_any_bitrev(hal.copy_from(rnd(2, 3 * SEG)), 1, flags, xs, out)
    assert not out.view().any()


# ------------------------------------------------------------------ b. NTT column groups
NTT_DEFAULTS = {"ntt_fast": 1, "ntt_group_cols": 0, "ntt_cols_per_wg": 8, "ntt_tile_b_wide": 1, "ntt_tile_b_log": 13}


def ntt_columns(seed, n, count):
    """`count` columns of n rows: random ones, the last five extreme where there is room for them"""
    if count >= 7:
        return np.concatenate([rnd(seed, n * (count - 5)), adversarial_columns(n)])
    return rnd(seed, n * count)


@pytest.mark.parametrize("cpw", [8, 4])
@pytest.mark.parametrize("g,count", [(1, 3), (2, 5), (3, 7), (5, 7), (4, 4), (8, 3)])
@pytest.mark.parametrize("bits", [12, 14])
def test_ntt_column_groups(hal, oracle, bits, g, count, cpw):
    """ntt_group_cols = g runs pass A and pass B of a two-pass forward transform on g columns at a time: input and output offsets per
    group, a ragged last group (5 = 2 + 2 + 1, 7 = 3 + 3 + 1, 7 = 5 + 2), one column per group; g >= count takes the ungrouped path.
    With ntt_cols_per_wg = 4 a group of three is narrower than the multi-column pass A and one of five is no multiple of it.
    2^12 and 2^14 rows expand to 2^14 and 2^16: a contiguous pass of 2^12 and a strided pass of 4 and of 16 rows.  Which kernel each
    group launches (the ragged one included) is in tests/golden/ntt_launches.json, replayed by tests/test_ntt_plan_check_cpu.py."""
    n = 1 << bits
    x = ntt_columns(bits * 100 + count, n, count)
    y = ntt_columns(bits * 100 + count + 1, 4 * n, count)
    ref_out = np.zeros(4 * n * count, np.uint32)
    oracle.bxo_batch_expand_into_evaluate_ntt(ref_out, x, count, n, 2)
    with tuned(hal, {"ntt_fast": 1, "ntt_group_cols": g, "ntt_cols_per_wg": cpw}, NTT_DEFAULTS):
        d_in, out = hal.copy_from(x), hal.alloc(4 * n * count)
        hal.batch_expand_into_evaluate_ntt(out, d_in, count, 2)
        assert np.array_equal(out.view(), ref_out), "batch_expand_into_evaluate_ntt"
        assert np.array_equal(d_in.view(), x), "the input of the expanding call"
        for eb in (0, 2):  # in place, on columns of the expanded size (the same two-pass split)
            io = hal.copy_from(y)
            hal.batch_evaluate_ntt(io, count, eb)
            ref = y.copy()
            oracle.bxo_batch_evaluate_ntt(ref, count, 4 * n, eb)
            assert np.array_equal(io.view(), ref), ("batch_evaluate_ntt", eb)


# ------------------------------------------------------------------ c. ntt_tile_b_wide = 0
@pytest.mark.parametrize("m,tile_b_log", [(22, 13), (23, 13), (22, 12)])
def test_ntt_pass_b_without_the_widened_tile(hal, oracle, m, tile_b_log):
    """With ntt_tile_b_wide = 1 every strided pass of 2^10 or more rows is widened to the 2^14-element tile.  Switched off, a 2^22
    transform runs its 2^10-row pass B on the 2^13 tile — the compiled geometry ntt_r16_kernel<.., 10, 3> — or, with
    ntt_tile_b_log = 12, on the generic one, and a 2^23 transform its 2^11-row pass on the generic geometry.  That these settings
    plan these kernels is checked without a GPU: the three tuples are cases of tests/golden/ntt_launches.json, which
    tests/test_ntt_plan_check_cpu.py replays through the planner.  Both directions (pass B serves the inverse too), two columns:
    random, and alternating 0 / P - 1."""
    size, n = 1 << m, 1 << (m - 2)

    def two_columns(seed, rows):
        alt = np.zeros(rows, np.uint32)
        alt[1::2] = P - 1
        return np.concatenate([rnd(seed, rows), alt])

    x, small = two_columns(m, size), two_columns(m + 1, n)
    ref = x.copy()
    oracle.bxo_batch_interpolate_ntt(ref, 2, size)
    ref_out = np.zeros(2 * size, np.uint32)
    oracle.bxo_batch_expand_into_evaluate_ntt(ref_out, small, 2, n, 2)
    with tuned(hal, {"ntt_fast": 1, "ntt_tile_b_wide": 0, "ntt_tile_b_log": tile_b_log}, NTT_DEFAULTS):
        io = hal.copy_from(x)
        hal.batch_interpolate_ntt(io, 2)
        assert np.array_equal(io.view(), ref), "batch_interpolate_ntt"
        d_in = hal.copy_from(small)
        hal.batch_expand_into_evaluate_ntt(io, d_in, 2, 2)
        assert np.array_equal(io.view(), ref_out), "batch_expand_into_evaluate_ntt"
        assert np.array_equal(d_in.view(), small), "the input of the expanding call"
        io.free(), d_in.free()


# ------------------------------------------------------------------ c'. NTT on a slice that is only word-aligned
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("bits", [13, 14])
def test_ntt_on_a_slice_that_is_only_word_aligned(hal, oracle, bits, off):
    """Default tunables: a buffer that does not start on a 16-byte boundary cannot take the radix-16 pass A (16-byte accesses) and runs
    the v1 contiguous pass beside the radix-16 strided pass, in both directions — the plan tests/test_ntt_plan_check_cpu.py replays
    for the `offset` cases of tests/golden/ntt_launches.json.  2^13 and 2^14 are the smallest two-pass sizes.  Every entry point,
    bit-exact against the oracle, and the words around the slice stay."""
    n, count, pad = 1 << bits, 2, 8
    rng = np.random.default_rng(bits * 10 + off)
    x = rnd(bits * 10 + off, n * count)

    def on_slice(call, data):
        host = rng.integers(0, 1 << 32, off + data.size + pad, dtype=np.uint32)
        host[off:off + data.size] = data
        whole = hal.copy_from(host)
        d = whole.slice(off, data.size)
        assert d.raw.dptr % 16 != 0
        call(d)
        got = whole.view()
        assert np.array_equal(got[:off], host[:off]) and np.array_equal(got[off + data.size:], host[off + data.size:]), "around the slice"
        return got[off:off + data.size]

    ref = x.copy()
    oracle.bxo_batch_interpolate_ntt(ref, count, n)
    assert np.array_equal(on_slice(lambda d: hal.batch_interpolate_ntt(d, count), x), ref), "batch_interpolate_ntt"
    oracle.bxo_zk_shift(ref, count, n)
    assert np.array_equal(on_slice(lambda d: hal.batch_interpolate_zk(d, count), x), ref), "batch_interpolate_zk"
    for eb in (0, 2):
        ref = x.copy()
        oracle.bxo_batch_evaluate_ntt(ref, count, n, eb)
        assert np.array_equal(on_slice(lambda d: hal.batch_evaluate_ntt(d, count, eb), x), ref), ("batch_evaluate_ntt", eb)
    small = c(x[:n // 4 * count])  # n / 4 rows expand to the same two-pass size n
    ref_out = np.zeros(n * count, np.uint32)
    oracle.bxo_batch_expand_into_evaluate_ntt(ref_out, small, count, n // 4, 2)
    out = hal.alloc(n * count)
    assert out.raw.dptr % 16 == 0
    assert np.array_equal(on_slice(lambda d: hal.batch_expand_into_evaluate_ntt(out, d, count, 2), small), small), "the input of the expanding call"
    assert np.array_equal(out.view(), ref_out), "batch_expand_into_evaluate_ntt"


# ------------------------------------------------------------------ d. hash_rows_block
HASH_ROWS_SHAPES = [(1, 1), (63, 15), (64, 16), (65, 17), (100, 33), (1000, 40), (4097, 24)]
_hash_rows_cases = {}


def hash_rows_case(oracle, rows, cols):
    """(column-major matrix, the oracle's digests); (256, 48) is the extreme matrix of test_poseidon2_extreme_operands"""
    key = (rows, cols)
    if key not in _hash_rows_cases:
        x = c(poseidon2_extreme_matrix(rows, cols).reshape(-1)) if key == (256, 48) else rnd(rows * 31 + cols, rows * cols)
        ref = np.zeros(8 * rows, np.uint32)
        oracle.bxo_hash_rows(ref, x, rows, cols)
        x.setflags(write=False), ref.setflags(write=False)
        _hash_rows_cases[key] = (x, ref)
    return _hash_rows_cases[key]


@pytest.mark.parametrize("rows,cols", HASH_ROWS_SHAPES + [(256, 48)])
@pytest.mark.parametrize("block", [64, 128])
def test_hash_rows_with_smaller_workgroups(hal, oracle, block, rows, cols):
    """hash_rows_block changes the launch geometry of hash_rows_kernel: row counts below, at and just above a workgroup, a last
    workgroup that is partly idle, and the matrix of extreme words."""
    x, ref = hash_rows_case(oracle, rows, cols)
    with tuned(hal, {"hash_rows_block": block}, {"hash_rows_block": 256}):
        out = hal.alloc_digest(rows)
        hal.hash_rows(out, hal.copy_from(x))
        assert np.array_equal(out.view(), ref)


@pytest.mark.parametrize("block", [64, 128])
def test_merkle_build_leaves_with_smaller_workgroups(hal, oracle, block):
    """bx_merkle_build hashes its leaves through the same launcher"""
    rows, cols = 1024, 20
    x = rnd(rows, rows * cols)
    ref = np.zeros(16 * rows, np.uint32)
    leaves = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(leaves, x, rows, cols)
    ref[8 * rows:] = leaves
    size = rows
    while size > 1:
        oracle.bxo_hash_fold(ref, size, size // 2)
        size //= 2
    with tuned(hal, {"hash_rows_block": block}, {"hash_rows_block": 256}):
        nodes = hal.alloc_zeroed(16 * rows)
        hal.merkle_build(nodes, hal.copy_from(x), rows)
        assert np.array_equal(nodes.view()[8:], ref[8:])


# ------------------------------------------------------------------ e. fold_quad_wg
FOLD_ROWS = [2, 8, 16, 32, 128, 1024, 1 << 13, 1 << 17]  # below, at and above every cap; 2^17 is the largest fused layer
_fold_cases = {}


def fold_case(oracle, rows):
    """(leaf digests, the oracle's node array): random field words as leaves"""
    if rows not in _fold_cases:
        leaves = rnd(rows + 5, 8 * rows)
        ref = np.zeros(16 * rows, np.uint32)
        ref[8 * rows:] = leaves
        size = rows
        while size > 1:
            oracle.bxo_hash_fold(ref, size, size // 2)
            size //= 2
        ref.setflags(write=False)
        _fold_cases[rows] = (leaves, ref)
    return _fold_cases[rows]


def fold_both_ways(hal, host_nodes, rows):
    """the node array after bx_merkle_fold, and after the layer-by-layer bx_hash_fold chain"""
    nodes = hal.copy_from(host_nodes)
    hal._check(hal.lib.bx_merkle_fold(hal.ctx, nodes.raw, rows))
    chain = hal.copy_from(host_nodes)
    size = rows
    while size > 1:
        hal.hash_fold(chain, size, size // 2)
        size //= 2
    return nodes.view(), chain.view()


@pytest.mark.parametrize("rows", FOLD_ROWS)
@pytest.mark.parametrize("wg", [16, 64, 256])
def test_merkle_fold_with_smaller_quad_workgroups(hal, oracle, wg, rows):
    """fold_quad_wg caps the input digests per workgroup of hash_fold_quad_kernel, which runs 2 * per_wg lanes: 32 (half a wave), 128
    and 512, over layers smaller than, equal to and larger than the cap, several fused launches deep.  fold_quad and
    fold_fuse_below stay at their defaults.  Every node from index 1 on against the oracle's tree."""
    leaves, ref = fold_case(oracle, rows)
    host = np.concatenate([np.zeros(8 * rows, np.uint32), leaves])
    with tuned(hal, {"fold_quad_wg": wg}, {"fold_quad_wg": 512}):
        got, chain = fold_both_ways(hal, host, rows)
    assert np.array_equal(got[8:], ref[8:]), "bx_merkle_fold"
    assert np.array_equal(chain[8:], ref[8:]), "bx_hash_fold chain"


@pytest.fixture(scope="module")
def shal():
    from boundless_amd.hal import HipHal

    h = HipHal(0, hashfn="sha-256")
    yield h
    h.close()


@pytest.mark.parametrize("rows", [16, 1024, 1 << 13])
def test_sha256_merkle_fold_with_a_smaller_workgroup_cap(shal, rows):
    """The same cap drives sha256_fold_multi_kernel of the `sha-256` suite: against tests/sha256_ref.py."""
    leaves = np.random.default_rng(rows).integers(0, 2**32, (rows, 8), dtype=np.uint64).astype(np.uint32)  # digest words: any value
    want = sha256_ref.merkle_nodes(leaves)
    host = np.zeros((2 * rows, 8), np.uint32)
    host[rows:] = leaves
    with tuned(shal, {"fold_quad_wg": 64}, {"fold_quad_wg": 512}):
        got, chain = fold_both_ways(shal, host.reshape(-1), rows)
    assert np.array_equal(got.reshape(2 * rows, 8)[1:], want[1:]), "bx_merkle_fold"
    assert np.array_equal(chain.reshape(2 * rows, 8)[1:], want[1:]), "bx_hash_fold chain"
