"""GPU: bx_batch_invert_ext / bx_batch_invert_elem / bx_prefix_sums / bx_batch_prefix_sums / bx_logup_accumulate against the
big-integer reference of tests/logup_ref.py, word for word.

Every operand lives inside a larger device buffer at a word offset that is not the allocation's start (a multiple of 4 words for ext
buffers, any word for base-field ones), with random canary words on both sides that must come back untouched.  Every case runs under
the tunable scan_lookback = 1 (the one-launch look-back kernels) and 0 (the three-phase kernels); the two inversion entry points
do not read the tunable and run once.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extreme_words  # noqa: E402
import logup_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

P = R.P
ONE = R.encode(1)
PAD = 48  # canary words on each side
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, (1 << 16) + 1, 1 << 20]
COUNTS = [1, 3, 16]
SMALL = 1025  # up to here the reference is the term-by-term Python-int definition, above it the vectorised restatement of it


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
    """`data` inside a larger device buffer at word offset PAD + off (off a multiple of `granule` words), canaries around it"""

    def __init__(self, hal, rng, data, granule):
        data = np.ascontiguousarray(data, dtype=np.uint32)
        self.n = data.size
        self.off = PAD + int(rng.integers(1, 8)) * granule
        self.host = rng.integers(0, 1 << 32, self.off + self.n + PAD + 8, dtype=np.uint32)
        self.host[self.off:self.off + self.n] = data
        self.whole = hal.copy_from(self.host)
        self.buf = self.whole.slice(self.off, self.n)

    def check(self, want, what):
        got = self.whole.view()
        assert np.array_equal(got[:self.off], self.host[:self.off]) and np.array_equal(got[self.off + self.n:], self.host[self.off + self.n:]), \
            f"{what}: words outside the operand were written"
        got = got[self.off:self.off + self.n]
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


def rand_ext(seed, n):
    """n ext elements: random words, a few zero elements and a few from the base field sprinkled in"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, P, 4 * n, dtype=np.uint32).reshape(n, 4)
    if n > 4:
        x[rng.integers(0, n, max(1, n // 97))] = 0
        x[rng.integers(0, n, max(1, n // 89)), 1:] = 0
    return x.ravel()


def rand_elem(seed, n):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, P, n, dtype=np.uint32)
    if n > 4:
        x[rng.integers(0, n, max(1, n // 97))] = 0
    return x


def ref_invert_ext(x):
    return R.batch_invert_ext(x) if x.size <= 4 * SMALL else R.batch_invert_ext_big(x)


def ref_invert_elem(x):
    return R.batch_invert_elem(x) if x.size <= 4 * SMALL else R.batch_invert_elem_big(x)


def ref_logup(d, m, count):
    return R.logup_accumulate(d, m, count) if d.size <= 4 * SMALL else R.logup_accumulate_big(d, m, count)


# ---- the five entry points over the sizes around chunk (8), wave (512) and tile (2048) boundaries ----
@pytest.mark.parametrize("n", SIZES)
def test_batch_invert_ext(hal, n):
    x = cached(("x", n), lambda: rand_ext(100 + n, n))
    want = cached(("inv_ext", n), lambda: ref_invert_ext(x))
    io = Placed(hal, np.random.default_rng(n), x, 4)
    hal.batch_invert_ext(io.buf)
    io.check(want, f"batch_invert_ext n={n}")
    io.free()


@pytest.mark.parametrize("n", SIZES)
def test_batch_invert_elem(hal, n):
    x = cached(("e", n), lambda: rand_elem(200 + n, n))
    want = cached(("inv_elem", n), lambda: ref_invert_elem(x))
    for granule in (1, 4):  # any word offset (single-word accesses) and a 16-byte aligned one (16-byte accesses)
        io = Placed(hal, np.random.default_rng(n + granule), x, granule)
        hal.batch_invert_elem(io.buf)
        io.check(want, f"batch_invert_elem n={n} granule={granule}")
        io.free()


@pytest.mark.parametrize("n", SIZES)
def test_prefix_sums(hal, lookback, n):
    x = cached(("x", n), lambda: rand_ext(100 + n, n))
    io = Placed(hal, np.random.default_rng(n), x, 4)
    hal.prefix_sums(io.buf)
    io.check(R.prefix_sums(x), f"prefix_sums n={n}")
    io.free()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_batch_prefix_sums(hal, lookback, n, count):
    x = cached(("x", n * count), lambda: rand_ext(100 + n * count, n * count))
    io = Placed(hal, np.random.default_rng(n), x, 4)
    hal.batch_prefix_sums(io.buf, count)
    io.check(R.batch_prefix_sums(x, count), f"batch_prefix_sums n={n} count={count}")
    io.free()


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "alias"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_logup_accumulate(hal, lookback, n, count, alias):
    d = cached(("x", n * count), lambda: rand_ext(100 + n * count, n * count))
    m = cached(("e", n * count), lambda: rand_elem(200 + n * count, n * count))
    want = cached(("logup", n, count), lambda: ref_logup(d, m, count))
    rng = np.random.default_rng(n + count)
    den = Placed(hal, rng, d, 4)
    mul = Placed(hal, rng, m, 1)
    out = den if alias else Placed(hal, rng, np.zeros(4 * n * count, np.uint32), 4)
    hal.logup_accumulate(out.buf, den.buf, mul.buf, count)
    out.check(want, f"logup_accumulate n={n} count={count} alias={alias}")
    mul.unchanged("logup_accumulate: mults")
    if not alias:
        den.unchanged("logup_accumulate: denoms")
        out.free()
    den.free()
    mul.free()


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 131072, 131073])
def test_sums_at_the_tile_and_window_edges(hal, lookback, n, count):
    """the sizes the products are tested at: around the 2048-element tile, and the 64-tile look-back window (131072), which is also
    where the three-phase driver first recurses (131072 / 64 chunks > 2048)"""
    d = cached(("x", n * count), lambda: rand_ext(100 + n * count, n * count))
    m = cached(("e", n * count), lambda: rand_elem(200 + n * count, n * count))
    rng = np.random.default_rng(n + count)
    io = Placed(hal, rng, d, 4)
    hal.batch_prefix_sums(io.buf, count)
    io.check(R.batch_prefix_sums(d, count), f"batch_prefix_sums n={n} count={count}")
    io.free()
    want = cached(("logup", n, count), lambda: R.logup_accumulate_big(d, m, count))
    den = Placed(hal, rng, d, 4)
    mul = Placed(hal, rng, m, 1)
    out = Placed(hal, rng, np.zeros(4 * n * count, np.uint32), 4)
    hal.logup_accumulate(out.buf, den.buf, mul.buf, count)
    out.check(want, f"logup_accumulate n={n} count={count}")
    den.unchanged("logup_accumulate: denoms")
    mul.unchanged("logup_accumulate: mults")
    for b in (den, mul, out):
        b.free()


def test_two_to_the_22_once(hal):
    n = 1 << 22
    x = rand_ext(22, n)
    m = rand_elem(23, n)
    inv = R.batch_invert_ext_big(x)
    io = Placed(hal, np.random.default_rng(1), x, 4)
    hal.batch_invert_ext(io.buf)
    io.check(inv, "batch_invert_ext 2^22")
    io.free()
    io = Placed(hal, np.random.default_rng(2), x, 4)
    hal.prefix_sums(io.buf)
    io.check(R.prefix_sums(x), "prefix_sums 2^22")
    io.free()
    den = Placed(hal, np.random.default_rng(3), x, 4)
    mul = Placed(hal, np.random.default_rng(4), m, 1)
    hal.logup_accumulate(den.buf, den.buf, mul.buf, 1)
    den.check(R.batch_prefix_sums(R.scale_ext_big(inv, m)), "logup_accumulate 2^22")
    den.free()
    mul.free()
    e = Placed(hal, np.random.default_rng(5), m, 1)
    hal.batch_invert_elem(e.buf)
    e.check(R.batch_invert_elem_big(m), "batch_invert_elem 2^22")
    e.free()


# ---- adversarial inputs ----
N_ADV = 2 * 2048 + 77  # two whole tiles and a ragged third


def adversarial(kind, n, width):
    """n elements of `width` words"""
    x = np.random.default_rng(5).integers(1, P, (n, width), dtype=np.uint32)
    if kind == "all_zero":
        x[:] = 0
    elif kind == "all_one":
        x[:] = 0
        x[:, 0] = ONE
    elif kind == "all_p_minus_1":
        x[:] = P - 1
    elif kind == "zero_first":
        x[0] = 0
    elif kind == "zero_last":
        x[n - 1] = 0
    elif kind == "zero_chunk_boundaries":
        x[[7, 8, 511, 512, 2047, 2048, 4095, 4096]] = 0  # last / first element of a lane's chunk, of a wave, of a tile
    elif kind == "every_second_zero":
        x[::2] = 0
    elif kind == "every_other_second_zero":
        x[1::2] = 0
    elif kind == "whole_chunk_zero":
        x[16:24] = 0
        x[2048:2056] = 0
    elif kind == "whole_tile_zero":
        x[2048:4096] = 0
    elif kind in CENTRED:  # the words of largest magnitude for the centred arithmetic (tests/extreme_words.py)
        x = extreme_words.pattern(kind, (n, width) if width > 1 else n, seed=5).reshape(n, width)  # alt_half: within an ext element, else from element to element
    else:
        raise ValueError(kind)
    return x.ravel()


ADVERSARIAL = ["all_zero", "all_one", "all_p_minus_1", "zero_first", "zero_last", "zero_chunk_boundaries", "every_second_zero",
               "every_other_second_zero", "whole_chunk_zero", "whole_tile_zero"]


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_adversarial_inversion(hal, kind):
    x = adversarial(kind, N_ADV, 4)
    want = cached(("adv_ext", kind), lambda: R.batch_invert_ext_big(x))
    io = Placed(hal, np.random.default_rng(1), x, 4)
    hal.batch_invert_ext(io.buf)
    io.check(want, f"batch_invert_ext {kind}")
    zero = ~x.reshape(-1, 4).any(axis=1)
    got = io.whole.view()[io.off:io.off + io.n].reshape(-1, 4)
    assert not got[zero].any() and got[~zero].any(axis=1).all(), "zero maps to zero and nothing else does"
    io.free()
    e = adversarial(kind, 8 * N_ADV + 5, 1)
    want = cached(("adv_elem", kind), lambda: R.batch_invert_elem_big(e))
    for granule in (1, 4):
        io = Placed(hal, np.random.default_rng(2), e, granule)
        hal.batch_invert_elem(io.buf)
        io.check(want, f"batch_invert_elem {kind}")
        io.free()


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "alias"])
@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_adversarial_logup(hal, lookback, kind, alias):
    d = adversarial(kind, N_ADV, 4)
    for mkind in ("all_p_minus_1", kind):
        m = adversarial(mkind, N_ADV, 1)
        want = cached(("adv_logup", kind, mkind), lambda: R.logup_accumulate_big(d, m, 1))
        rng = np.random.default_rng(3)
        den = Placed(hal, rng, d, 4)
        mul = Placed(hal, rng, m, 1)
        out = den if alias else Placed(hal, rng, rng.integers(0, 1 << 32, 4 * N_ADV, dtype=np.uint32), 4)
        hal.logup_accumulate(out.buf, den.buf, mul.buf, 1)
        out.check(want, f"logup_accumulate {kind} x {mkind}")
        for b in {den, mul, out}:
            b.free()
    s = Placed(hal, np.random.default_rng(4), d, 4)
    hal.prefix_sums(s.buf)
    s.check(R.prefix_sums(d), f"prefix_sums {kind}")
    s.free()


# The ext inversion, the running sums and the fused LogUp call multiply and accumulate on centred operands: +-P/2 everywhere, +-P/2
# alternating within an element, and a draw from every extreme word, through the adversarial tests above — same N_ADV, same references
# ("all_p_minus_1" and friends centre to -1, 0 and 1: the smallest magnitudes).  An ext element of four equal words is no zero, and
# edge_mix holds zero words (zero base-field elements, and now and then a zero ext element).
CENTRED = ["all_half", "all_half1", "alt_half", "edge_mix"]


@pytest.mark.parametrize("kind", CENTRED)
def test_centred_extremes_inversion(hal, kind):
    test_adversarial_inversion(hal, kind)


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "alias"])
@pytest.mark.parametrize("kind", CENTRED)
def test_centred_extremes_logup(hal, lookback, kind, alias):
    test_adversarial_logup(hal, lookback, kind, alias)


# ---- relations between the calls ----
@pytest.mark.parametrize("n,count", [(5, 1), (2049, 3), ((1 << 16) + 1, 3), (1 << 17, 16)])
def test_fused_equals_the_three_calls(hal, lookback, n, count):
    """bx_batch_invert_ext, an element-wise scale (no entry point: done on the host between the two calls), bx_batch_prefix_sums —
    against bx_logup_accumulate on the same words, both as the device returns them"""
    d = rand_ext(31 + n, n * count)
    m = rand_elem(32 + n, n * count)
    rng = np.random.default_rng(n)
    a = Placed(hal, rng, d, 4)
    hal.batch_invert_ext(a.buf)
    inv = a.buf.view()
    a.buf.copy_from(R.scale_ext_big(inv, m))
    hal.batch_prefix_sums(a.buf, count)
    three = a.buf.view()
    den = Placed(hal, rng, d, 4)
    mul = Placed(hal, rng, m, 1)
    out = Placed(hal, rng, np.zeros(4 * n * count, np.uint32), 4)
    hal.logup_accumulate(out.buf, den.buf, mul.buf, count)
    out.check(three, f"fused against three calls n={n} count={count}")
    for b in (a, den, mul, out):
        b.free()


@pytest.mark.parametrize("n,count", [(1, 1), (7, 3), (2049, 3), ((1 << 16) + 1, 16), (1 << 20, 1)])
def test_fused_equals_its_unfused_device_path(hal, n, count):
    """The library has no entry point for a per-element scale, so the composition above scales on the host.  The device does hold a
    second, unfused path with its own scale: under scan_lookback = 0 bx_logup_accumulate is binv_ext_kernel<scale> (invert, then
    f4_scale by the multiplicity) followed by the three-phase sum kernels.  Both paths on the same words, as the device returns them."""
    d = rand_ext(35 + n, n * count)
    m = rand_elem(36 + n, n * count)
    rng = np.random.default_rng(n)
    got = []
    try:
        for lb in (1, 0):
            hal.set_tunable("scan_lookback", lb)
            den = Placed(hal, rng, d, 4)
            mul = Placed(hal, rng, m, 1)
            out = Placed(hal, rng, np.zeros(4 * n * count, np.uint32), 4)
            hal.logup_accumulate(out.buf, den.buf, mul.buf, count)
            got.append(out.buf.view())
            den.unchanged("denoms")
            for b in (den, mul, out):
                b.free()
    finally:
        hal.set_tunable("scan_lookback", 1)
    assert np.array_equal(got[0], got[1])
    assert got[0].any()


@pytest.mark.parametrize("n", [1, 9, 2048, 100003])
def test_inverting_twice_returns_the_input(hal, n):
    x = rand_ext(41 + n, n)
    io = Placed(hal, np.random.default_rng(n), x, 4)
    hal.batch_invert_ext(io.buf)
    once = io.buf.view()
    assert n < 8 or not np.array_equal(once, x)
    hal.batch_invert_ext(io.buf)
    io.check(x, "batch_invert_ext twice")
    io.free()
    e = rand_elem(42 + n, 3 * n)
    io = Placed(hal, np.random.default_rng(n), e, 1)
    hal.batch_invert_elem(io.buf)
    hal.batch_invert_elem(io.buf)
    io.check(e, "batch_invert_elem twice")
    io.free()


@pytest.mark.parametrize("n", [64, 5000, 1 << 16])
def test_logup_identity_on_the_device(hal, lookback, n):
    """sum_i 1 / (beta + a_i) = sum_i 1 / (beta + b_i) when b is a permutation of a, and not after one entry of b changes: the
    statement an accumulate stage proves, computed with logup_accumulate alone."""
    rng = np.random.default_rng(900 + n)
    a = rng.integers(0, P, n, dtype=np.uint64)
    b = a[rng.permutation(n)].copy()
    beta = rng.integers(0, P, 4, dtype=np.uint64)
    ones = np.full(n, ONE, dtype=np.uint32)

    def last(col):
        den = np.tile(beta, (n, 1))
        den[:, 0] = (den[:, 0] + col) % P  # beta + v: v is a base-field word, it adds to the constant coefficient
        d = Placed(hal, rng, den.astype(np.uint32).ravel(), 4)
        m = Placed(hal, rng, ones, 1)
        hal.logup_accumulate(d.buf, d.buf, m.buf, 1)
        got = d.buf.view()[-4:].copy()
        d.free()
        m.free()
        return got

    sa, sb = last(a), last(b)
    assert np.array_equal(sa, sb)
    b[n // 3] = (b[n // 3] + 1) % P
    assert not np.array_equal(sa, last(b))


@pytest.mark.parametrize("n,count", [(1, 1), (65, 1), (2049, 1), (1500, 3)])
def test_prefix_products_second_opinion(hal, lookback, n, count):
    """the existing multiplicative scans against this file's own reference: same words as before"""
    x = rand_ext(51 + n, n * count)
    want = cached(("pp", n, count), lambda: R.batch_prefix_products(x, count))
    io = Placed(hal, np.random.default_rng(n), x, 4)
    hal.batch_prefix_products(io.buf, count)
    io.check(want, f"batch_prefix_products n={n} count={count}")
    io.free()
    if count == 1:
        io = Placed(hal, np.random.default_rng(n + 1), x, 4)
        hal.prefix_products(io.buf)
        io.check(want, f"prefix_products n={n}")
        io.free()


# ---- refusals ----
def _refused(hal, msg):
    assert msg, "the call was accepted"
    text = msg.decode()
    assert text and "null ctx" not in text
    return text


def test_refusals_return_a_message_and_write_nothing(hal, lookback):
    rng = np.random.default_rng(77)
    n = 96
    ext = Placed(hal, rng, rand_ext(1, n), 4)
    out = Placed(hal, rng, rand_ext(2, n), 4)
    mul = Placed(hal, rng, rand_elem(3, n), 1)
    lib, ctx = hal.lib, hal.ctx
    short = ext.whole.slice(ext.off, 4 * n - 2).raw  # not a multiple of 4 words
    assert "AoS ext" in _refused(hal, lib.bx_batch_invert_ext(ctx, short))
    assert "AoS ext" in _refused(hal, lib.bx_prefix_sums(ctx, short))
    assert "AoS ext" in _refused(hal, lib.bx_batch_prefix_sums(ctx, short, 1))
    assert "AoS ext" in _refused(hal, lib.bx_logup_accumulate(ctx, short, short, mul.buf.raw, 1))
    # out and denoms of different lengths
    assert "same number" in _refused(hal, lib.bx_logup_accumulate(ctx, out.whole.slice(out.off, 4 * n - 4).raw, ext.buf.raw, mul.buf.raw, 1))
    # a count that does not divide
    assert "split" in _refused(hal, lib.bx_batch_prefix_sums(ctx, ext.buf.raw, 5))
    assert "split" in _refused(hal, lib.bx_logup_accumulate(ctx, out.buf.raw, ext.buf.raw, mul.buf.raw, 7))
    # mults too short
    assert "multiplicity" in _refused(hal, lib.bx_logup_accumulate(ctx, out.buf.raw, ext.buf.raw, mul.whole.slice(mul.off, n - 1).raw, 1))
    assert "multiplicity" in _refused(hal, lib.bx_logup_accumulate(ctx, out.buf.raw, ext.buf.raw, mul.whole.slice(mul.off, n - 1).raw, 3))
    # hostile scalars: 0, and counts whose product with 4 (or with n) wraps
    for count in (0, 1 << 62, (1 << 62) + 1, (1 << 63) + 3, (1 << 64) - 1, (1 << 64) // 96 + 1, 65536):
        assert "sequences" in _refused(hal, lib.bx_batch_prefix_sums(ctx, ext.buf.raw, C.c_size_t(count)))
        assert "sequences" in _refused(hal, lib.bx_logup_accumulate(ctx, out.buf.raw, ext.buf.raw, mul.buf.raw, C.c_size_t(count)))
    # an ext operand that is not 16-byte aligned
    odd = ext.whole.slice(ext.off + 1, 4 * (n - 1)).raw
    assert "aligned" in _refused(hal, lib.bx_batch_invert_ext(ctx, odd))
    assert "aligned" in _refused(hal, lib.bx_prefix_sums(ctx, odd))
    assert "aligned" in _refused(hal, lib.bx_logup_accumulate(ctx, odd, odd, mul.buf.raw, 1))
    hal.sync()
    for b, what in ((ext, "ext"), (out, "out"), (mul, "mults")):
        b.unchanged(f"after refusals: {what}")
        b.free()
    # the ctx still works
    io = Placed(hal, rng, rand_ext(4, n), 4)
    hal.prefix_sums(io.buf)
    io.check(R.prefix_sums(io.host[io.off:io.off + io.n]), "prefix_sums after refusals")
    io.free()


def test_empty_buffers_are_accepted(hal, lookback):
    buf = hal.alloc(64)
    empty = buf.slice(16, 0)
    hal.batch_invert_ext(empty)
    hal.batch_invert_elem(empty)
    hal.prefix_sums(empty)
    hal.batch_prefix_sums(empty, 3)
    hal.logup_accumulate(empty, empty, empty, 2)
    hal.sync()
    buf.free()


def test_profile_report_lists_the_new_ops(hal):
    x = rand_ext(61, 4096)
    m = rand_elem(62, 4096)
    a, b = hal.copy_from(x), hal.copy_from(m)
    hal.profile_reset()
    hal.profile_enable(True)
    try:
        hal.batch_invert_ext(a)
        hal.batch_invert_elem(b)
        hal.prefix_sums(a)
        hal.batch_prefix_sums(a, 2)
        hal.logup_accumulate(a, a, b, 4)
        rep = hal.profile_report()
    finally:
        hal.profile_enable(False)
        hal.profile_reset()
    text = str(rep)
    for name in ("batch_invert_ext", "batch_invert_elem", "prefix_sums", "logup_accumulate"):
        assert name in text, (name, rep)
    a.free()
    b.free()


def test_gathers_queued_before_a_call_are_flushed_first(hal):
    """the new calls go through the same entry bracket as their neighbours: a gather_sample queued just before reads the
    words as they were BEFORE the scan"""
    x = rand_ext(71, 64)
    src = hal.copy_from(x)
    dst = hal.alloc(4)
    hal.gather_sample(dst, src, 4 * 63, 4, 1)  # the last element, queued
    hal.prefix_sums(src)
    assert np.array_equal(dst.view(), x[-4:])
    assert np.array_equal(src.view(), R.prefix_sums(x))
    src.free()
    dst.free()
