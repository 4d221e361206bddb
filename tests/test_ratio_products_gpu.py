"""GPU: bx_batch_ratio_products against the big-integer reference of tests/ratio_ref.py, word for word, under both settings of the
tunable scan_lookback (1: one launch of the look-back kernel with the ratio pre-step; 0: the inverting launch and the three-phase
products).

Sizes: 1, 2 (below a chunk), 7, 8, 9 (the chunk of 8 a lane inverts at once), 2047, 2048, 2049 (the tile), 4097 (three tiles) and
2048 * 64 + 3 (the second look-back window).  Every operand lives inside a larger device buffer at a 16-byte aligned offset that is
not the allocation's start, with canary words on both sides that must come back untouched; `out` is poisoned first.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import extreme_words  # noqa: E402
import logup_ref as L  # noqa: E402
import ratio_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

P = L.P
ONE = L.encode(1)
POISON = 0xDEADBEEF
PAD = 48
SIZES = [1, 2, 7, 8, 9, 2047, 2048, 2049, 4097, 2048 * 64 + 3]
COUNTS = [1, 3]
SMALL = 9  # up to here the reference is the term-by-term definition on Python ints, above it its vectorised restatement


@pytest.fixture(scope="module")
def hal():
    from boundless_amd.hal import HipHal

    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(params=[1, 0], ids=["lookback", "three_phase"])
def lookback(hal, request):
    hal.set_tunable("scan_lookback", request.param)
    yield request.param
    hal.set_tunable("scan_lookback", 1)


class Placed:
    """`data` inside a larger device buffer at word offset PAD + 4 k, canaries around it"""

    def __init__(self, hal, rng, data):
        data = np.ascontiguousarray(data, dtype=np.uint32)
        self.n = data.size
        self.off = PAD + int(rng.integers(1, 8)) * 4
        self.host = rng.integers(0, 1 << 32, self.off + self.n + PAD + 8, dtype=np.uint32)
        self.host[self.off:self.off + self.n] = data
        self.whole = hal.copy_from(self.host)
        self.buf = self.whole.slice(self.off, self.n)

    def words(self):
        got = self.whole.view()
        assert np.array_equal(got[:self.off], self.host[:self.off]) and np.array_equal(got[self.off + self.n:], self.host[self.off + self.n:]), \
            "words outside the operand were written"
        return got[self.off:self.off + self.n]

    def check(self, want, what):
        got = self.words()
        bad = np.nonzero(got != np.asarray(want, dtype=np.uint32))[0]
        assert bad.size == 0, f"{what}: {bad.size} of {self.n} words differ from the reference, first at word {int(bad[0])}"

    def unchanged(self, what):
        self.check(self.host[self.off:self.off + self.n], what)

    def free(self):
        self.whole.free()


_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def reference(nums, dens, count):
    return R.ratio_products(nums, dens, count) if nums.size <= 4 * SMALL * count else R.ratio_products_big(nums, dens, count)


def nonzero_ext(seed, n):
    """n ext elements none of which is zero (a word is zero with probability 1 / P; an element that came out zero is made one)"""
    x = np.random.default_rng(seed).integers(0, P, (n, 4), dtype=np.uint32)
    x[~x.any(axis=1), 0] = ONE
    return x.ravel()


def inputs(kind, n, count):
    """-> (nums, denoms) of count * n ext elements"""
    total = n * count
    if kind == "random":
        return nonzero_ext(1000 + total, total), nonzero_ext(2000 + total, total)
    if kind == "equal":
        x = nonzero_ext(3000 + total, total)
        return x, x.copy()
    a, b = kind.split("/")
    return extreme_words.pattern(a, 4 * total, seed=total), extreme_words.pattern(b, 4 * total, seed=total + 1)


def run_case(hal, kind, n, count, alias, what):
    nums, dens = cached(("in", kind, n, count), lambda: inputs(kind, n, count))
    want = cached(("want", kind, n, count), lambda: reference(nums, dens, count))
    rng = np.random.default_rng(n + count)
    a, d = Placed(hal, rng, nums), Placed(hal, rng, dens)
    out = a if alias else Placed(hal, rng, np.full(nums.size, POISON, np.uint32))
    hal.batch_ratio_products(out.buf, a.buf, d.buf, count)
    out.check(want, what)
    d.unchanged(f"{what}: denoms")
    if not alias:
        a.unchanged(f"{what}: nums")
        out.free()
    a.free()
    d.free()
    return want


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_random_ratios_are_the_reference(hal, lookback, n, count, alias):
    want = run_case(hal, "random", n, count, alias, f"random n={n} count={count} alias={alias}")
    assert np.count_nonzero(want) >= 0.99 * want.size, "degenerate reference: a call that writes zeros could pass"


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_equal_numerators_and_denominators_give_ones(hal, lookback, n, count, alias):
    want = run_case(hal, "equal", n, count, alias, f"equal n={n} count={count} alias={alias}")
    assert np.array_equal(want.reshape(-1, 4), np.tile(np.array([ONE, 0, 0, 0], np.uint32), (n * count, 1)))


# every extreme pattern as numerators over the next one as denominators; the largest size takes the two that vary from word to word
EXTREME_PAIRS = [f"{a}/{b}" for a, b in zip(extreme_words.EXTREME, extreme_words.EXTREME[1:] + extreme_words.EXTREME[:1])]


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_extreme_words_are_the_reference(hal, lookback, n, count, alias):
    for kind in (EXTREME_PAIRS if n <= 4097 else ["edge_mix/alt_half", "alt_half_rows/edge_mix"]):
        run_case(hal, kind, n, count, alias, f"{kind} n={n} count={count} alias={alias}")


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in_place"])
def test_a_zero_denominator_zeroes_the_product_from_its_row_on(hal, lookback, alias):
    """n = 4097, one planting per sequence: chunk position 0, chunk position 7, a whole chunk, the last element of tile 0"""
    n, count = 4097, 4
    first = [800, 807, 1600, 2047]
    nums, dens = nonzero_ext(71, n * count), nonzero_ext(72, n * count).reshape(count, n, 4)
    dens[0][800] = dens[1][807] = dens[3][2047] = 0
    dens[2][1600:1608] = 0
    dens = dens.ravel()
    clean = cached("zeros_clean", lambda: R.ratio_products_big(nums, nonzero_ext(72, n * count), count)).reshape(count, n, 4)
    want = cached("zeros_want", lambda: R.ratio_products_big(nums, dens, count)).reshape(count, n, 4)
    for s, z in enumerate(first):  # on the reference too
        assert np.array_equal(want[s][:z], clean[s][:z]) and np.all(want[s][:z].any(axis=1)) and not want[s][z:].any()
    rng = np.random.default_rng(5)
    a, d = Placed(hal, rng, nums), Placed(hal, rng, dens)
    out = a if alias else Placed(hal, rng, np.full(nums.size, POISON, np.uint32))
    hal.batch_ratio_products(out.buf, a.buf, d.buf, count)
    got = out.words().reshape(count, n, 4)
    for s, z in enumerate(first):
        assert np.array_equal(got[s][:z], want[s][:z]), f"sequence {s}: words before the zero differ from the reference"
        assert not got[s][z:].any(), f"sequence {s}: a word at or after row {z} is not zero"
    d.unchanged("denoms")
    for b in {a, d, out}:
        b.free()


def _refused(msg, match):
    assert msg, f"the call was accepted (expected: {match})"
    text = msg.decode()
    assert text.startswith("bx_batch_ratio_products: ") and match in text, text
    return text


def test_refusals_return_a_message_and_write_nothing(hal, lookback):
    import ctypes as C

    n = 96  # elements
    w = 4 * n
    one = hal.copy_from(np.full(8 * w + 16, POISON, np.uint32))
    lib, ctx = hal.lib, hal.ctx
    base = 4 * w  # word offset of `out` inside `one` (16-byte aligned: an allocation is)

    def call(out, nums, dens, count=1):
        return lib.bx_batch_ratio_products(ctx, out.raw, nums.raw, dens.raw, C.c_size_t(count))

    out, far_a, far_d = one.slice(base, w), one.slice(0, w), one.slice(2 * w, w)
    # every partial overlap of out with nums, and every overlap of out with denoms (the same start included): one element, half, all but one
    for shift in (4, w // 2, w - 4):
        for sign in (-1, 1):
            moved = one.slice(base + sign * shift, w)
            _refused(call(out, moved, far_d), "out and nums overlap")
            _refused(call(out, far_a, moved), "out and denoms overlap")
            _refused(call(out, out, moved), "out and denoms overlap")  # in place, and the denominators reach into it
    _refused(call(out, far_a, out), "out and denoms overlap")
    _refused(call(out, out, out), "out and denoms overlap")
    # nums and denoms may overlap each other freely: not a refusal (checked below, after the poison)
    # a misaligned buffer, each operand in turn
    _refused(call(one.slice(base + 1, w), far_a, far_d), "16-byte aligned")
    _refused(call(out, one.slice(1, w), far_d), "16-byte aligned")
    _refused(call(out, far_a, one.slice(2 * w + 2, w)), "16-byte aligned")
    # length mismatches
    _refused(call(out, one.slice(0, w - 4), far_d), "same number of AoS ext elements")
    _refused(call(out, far_a, one.slice(2 * w, w + 4)), "same number of AoS ext elements")
    _refused(call(one.slice(base, w - 2), one.slice(0, w - 2), one.slice(2 * w, w - 2)), "same number of AoS ext elements")
    _refused(call(out, far_a, far_d, 7), "do not split")
    for count in (0, 65536, (1 << 64) - 1):
        _refused(call(out, far_a, far_d, count), "[1, 65535]")
    assert b"null ctx" in lib.bx_batch_ratio_products(None, out.raw, far_a.raw, far_d.raw, C.c_size_t(1))
    hal.sync()
    assert np.all(one.view() == POISON), "a refused call wrote"
    # the next call is correct: nums and denoms overlapping each other by half
    x = nonzero_ext(9, n + n // 2)
    one.slice(0, x.size).copy_from(x)
    nums, dens = one.slice(0, w), one.slice(w // 2, w)
    hal.batch_ratio_products(out, nums, dens, 3)
    got = one.view()
    assert np.array_equal(got[base:base + w], R.ratio_products_big(x[:w], x[w // 2:w // 2 + w], 3))
    assert np.array_equal(got[:x.size], x) and np.all(got[x.size:base] == POISON) and np.all(got[base + w:] == POISON)
    one.free()


def test_empty_buffers_are_accepted(hal, lookback):
    buf = hal.alloc(64)
    empty = buf.slice(16, 0)
    hal.batch_ratio_products(empty, empty, empty, 2)
    hal.sync()
    buf.free()


def test_profile_report_lists_ratio_products(hal, lookback):
    a, d = hal.copy_from(nonzero_ext(61, 4096)), hal.copy_from(nonzero_ext(62, 4096))
    hal.profile_reset()
    hal.profile_enable(True)
    try:
        hal.batch_ratio_products(a, a, d, 2)
        rep = hal.profile_report()
    finally:
        hal.profile_enable(False)
        hal.profile_reset()
    assert rep["ratio_products"]["calls"] == 1, rep
    a.free()
    d.free()
