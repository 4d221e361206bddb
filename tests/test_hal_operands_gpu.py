"""GPU: the two dimensions of a HAL call's operands the other suites never vary — how the operands lie to each other in memory, and
what the index operands hold — and the dispatch branches that only sizes beyond the other tests' reach.

Overlap.  include/bx_hal.h ("Operand overlap"): an output must not share a byte with another operand of its call, except that an
element-wise entry point accepts an output that IS an input.  Here every operand of a call is a slice of ONE device allocation whose
remaining words are random canaries, so two operands can touch, share one word at either end, contain one another or alias.  A refused
placement returns "<entry point>: <a> and <b> overlap", leaves every byte of the allocation as it was, and the ctx goes on to compute a
valid call correctly; a touching placement and an allowed alias give the words the oracle computes from copies of the inputs, canaries
intact.  The reference is the C oracle, tests/logup_ref.py or plain numpy indexing — never the library's own un-aliased result.

Index contents: in-range values only (a device-resident index out of range stays the caller's responsibility and would read outside a
buffer), at the patterns random draws do not produce: all equal, descending, unused ids, duplicates, first and last.

mix_poly_coeffs runs at count = 1000 (four coefficients per lane) and 1001 (one), fri_fold at 1000 and 1024.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from oracle import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hal_operand_sizes as sizes  # noqa: E402
import logup_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
P = ol.P
PAD = 16  # canary words around every operand that does not touch another


@pytest.fixture(scope="module")
def hal():
    from boundless_amd.hal import BxBuf, HipHal

    h = HipHal(0)
    ctx, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    for name, args in (("bx_merkle_query_gather", [ctx, BxBuf, BxBuf, BxBuf, sz, sz, BxBuf, sz, sz]),
                       ("bx_hash_fold_indexed", [ctx, BxBuf, BxBuf, BxBuf, sz]),
                       ("bx_poly_divide_batch_indexed", [ctx, BxBuf, sz, sz, u32p, u32p, BxBuf])):
        fn = getattr(h.lib, name)
        fn.argtypes, fn.restype = args, C.c_char_p
    yield h
    h.close()


def rnd(seed, n):
    return ol.random_elems(np.random.default_rng(seed), n)


def c(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def bitrev_perm(n):
    idx = np.arange(1 << n, dtype=np.uint64)
    r = np.zeros_like(idx)
    for b in range(n):
        r |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(n - 1 - b)
    return r.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- placement
class Arena:
    """One device allocation of random words; operands are slices of it at given word offsets, holding their data."""

    def __init__(self, hal, total, offsets, data, seed):
        self.hal, self.offsets = hal, offsets
        self.host = np.random.default_rng(seed).integers(0, 1 << 32, total, dtype=np.uint32)
        for name in sorted(offsets, key=lambda k: offsets[k]):  # where two operands overlap, the higher one's words stand
            self.host[offsets[name]:offsets[name] + data[name].size] = data[name]
        self.dev = hal.copy_from(self.host)
        self.raw = {name: self.dev.slice(off, data[name].size).raw for name, off in offsets.items()}

    def unchanged(self, what):
        assert np.array_equal(self.dev.view(), self.host), f"{what}: the allocation was written"

    def check(self, want, what, ignore=()):
        """`want`: name -> words; every other word of the allocation as uploaded"""
        exp, got = self.host.copy(), self.dev.view()
        for name, words in want.items():
            exp[self.offsets[name]:self.offsets[name] + len(words)] = words
        for name, lo, hi in ignore:
            exp[self.offsets[name] + lo:self.offsets[name] + hi] = got[self.offsets[name] + lo:self.offsets[name] + hi]
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{what}: {bad.size} words differ from the reference, first at word {int(bad[0])} of the allocation ({self.offsets})"

    def free(self):
        self.dev.free()


class Case:
    """An entry point with its operands (name -> words), the (output, other) pairs its rule names, the raw call, and the oracle's result."""

    def __init__(self, name, data, pairs, call, want, alias_ok=(), ignore=()):
        self.name, self.data, self.pairs, self.call, self.want = name, {k: c(v) for k, v in data.items()}, pairs, call, want
        self.alias_ok, self.ignore = set(alias_ok), ignore


def up(x, a):
    return (x + a - 1) // a * a


KINDS = ["touch_after", "touch_before", "over_hi", "over_lo", "contain", "alias"]


def layout(case, pair, kind):
    """Word offsets of every operand (16-byte aligned unless the placement shifts one) and the allocation's size; None where the
    placement cannot keep the pair's alignment."""
    o, i = pair
    lo, li, step = case.data[o].size, case.data[i].size, 1  # one word of overlap
    offsets, off = {}, PAD
    for name, words in case.data.items():
        if name not in pair:
            offsets[name] = off
            off = up(off + words.size + PAD, 8)
    base = off + 8
    if kind == "touch_after":  # the output starts where the other operand ends
        if li % 4:
            return None
        offsets[i], offsets[o] = base, base + li
    elif kind == "touch_before":
        if lo % 4:
            return None
        offsets[o], offsets[i] = base, base + lo
    elif kind == "over_hi":  # the output's first word(s) are the other operand's last
        offsets[i], offsets[o] = base, base + li - step
    elif kind == "over_lo":  # the output's last word(s) are the other operand's first
        offsets[o], offsets[i] = base, base + lo - step
    elif kind == "contain":  # the shorter one inside the longer one (equal lengths: shifted by a quarter)
        small, big = (o, i) if lo <= li else (i, o)
        offsets[big], offsets[small] = base, base + 4 * max(1, min(case.data[big].size // 16, (case.data[big].size - case.data[small].size) // 8))
    elif kind == "alias":
        offsets[o] = offsets[i] = base
    end = max(offsets[k] + case.data[k].size for k in offsets)
    return offsets, up(end + PAD, 8)


def place(hal, case, pair, kind, seed=1):
    lay = layout(case, pair, kind)
    if lay is None:
        return None
    return Arena(hal, lay[1], lay[0], case.data, seed)


def refused(msg, name):
    assert msg, f"{name}: the call was accepted"
    text = msg.decode()
    assert "overlap" in text and text.startswith(name + ":"), text
    return text


# ---------------------------------------------------------------------------------------------------------------- the cases
def lib_call(fn_name, order, *scalars_after, host=()):
    """call(hal, raw): the entry point with the operands `order` (names; an int n inserts scalars_after[n]; "h0".. a host array)"""
    host = [c(h) for h in host]

    def call(hal, raw):
        args = []
        for a in order:
            if isinstance(a, int):
                args.append(scalars_after[a])
            elif a.startswith("host"):
                args.append(u32p(host[int(a[4:])]))
            else:
                args.append(raw[a])
        return getattr(hal.lib, fn_name)(hal.ctx, *args)
    return call


def case_fri_fold(oracle, dev):
    count = 1024 if dev else 1000
    x, mix = rnd(11, 64 * count), rnd(12, 4)
    ref = np.zeros(4 * count, np.uint32)
    oracle.bxo_fri_fold(ref, x, mix, count)
    data = {"out": rnd(13, 4 * count), "in": x}
    if dev:
        data["mix_ext"] = mix
        return Case("fri_fold_dev", data, [("out", "in"), ("out", "mix_ext")], lib_call("bx_fri_fold_dev", ["out", "in", "mix_ext"]), {"out": ref})
    return Case("fri_fold", data, [("out", "in")], lib_call("bx_fri_fold", ["out", "in", "host0"], host=[mix]), {"out": ref})


def case_mix(oracle, count):
    npoly, ncombo = 5, 2
    inp, combos = rnd(21, npoly * count), np.array([1, 0, 1, 1, 0], np.uint32)
    start, mix, init = rnd(22, 4), rnd(23, 4), rnd(24, 4 * count * ncombo)
    ref = init.copy()
    oracle.bxo_mix_poly_coeffs(ref, start, mix, inp, combos, npoly, count)
    return Case("mix_poly_coeffs", {"out": init, "in": inp, "combos": combos}, [("out", "in"), ("out", "combos")],
                lib_call("bx_mix_poly_coeffs", ["out", "host0", "host1", "in", "combos", 0, 1], npoly, count, host=[start, mix]), {"out": ref})


def case_sum_ext(oracle):
    count, to_add = 1000, 3
    e = rnd(31, 4 * count * to_add)
    ref = np.zeros(4 * count, np.uint32)
    oracle.bxo_eltwise_sum_extelem(ref, e, count, to_add)
    return Case("eltwise_sum_extelem", {"out": rnd(32, 4 * count), "in": e}, [("out", "in")], lib_call("bx_eltwise_sum_extelem", ["out", "in"]), {"out": ref})


def case_hash_rows(oracle):
    rows, cols = 300, 5
    x = rnd(41, rows * cols)
    ref = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(ref, x, rows, cols)
    return Case("hash_rows", {"out": rnd(42, 8 * rows), "matrix": x}, [("out", "matrix")], lib_call("bx_hash_rows", ["out", "matrix"]), {"out": ref})


def oracle_tree(oracle, x, rows, cols):
    ref = np.zeros(16 * rows, np.uint32)
    leaves = np.zeros(8 * rows, np.uint32)
    oracle.bxo_hash_rows(leaves, x, rows, cols)
    ref[8 * rows:] = leaves
    size = rows
    while size > 1:
        oracle.bxo_hash_fold(ref, size, size // 2)
        size //= 2
    return ref


def case_merkle_build(oracle):
    rows, cols = 512, 5
    x = rnd(51, rows * cols)
    return Case("merkle_build", {"nodes": rnd(52, 16 * rows), "matrix": x}, [("nodes", "matrix")], lib_call("bx_merkle_build", ["nodes", "matrix", 0], rows),
                {"nodes": oracle_tree(oracle, x, rows, cols)}, ignore=[("nodes", 0, 8)])  # node 0 does not exist: its slot is unspecified


def hash_pairs(oracle, digs, sel):
    out = np.zeros((len(sel), 8), np.uint32)
    for j, (a, b) in enumerate(sel):
        oracle.bxo_hash_pair(out[j], c(digs[a]), c(digs[b]))
    return out.reshape(-1)


def case_hash_fold_indexed(oracle):
    n, count = 40, 300
    digs = rnd(61, 8 * n).reshape(n, 8)
    sel = np.random.default_rng(62).integers(0, n, (count, 2), dtype=np.uint32)
    return Case("hash_fold_indexed", {"out": rnd(63, 8 * count), "in": digs.reshape(-1), "sel": sel.reshape(-1)}, [("out", "in"), ("out", "sel")],
                lib_call("bx_hash_fold_indexed", ["out", "in", "sel", 0], count), {"out": hash_pairs(oracle, digs, sel)})


def case_evaluate_any(oracle, bitrev):
    npoly, evals = 2, 3
    size = 1 << 15 if bitrev else 40000  # whole 2^15 segments (16-byte loads) / two ragged segments (the dword kernel)
    coeffs, which, xs = rnd(71, npoly * size), np.array([1, 0, 1], np.uint32), rnd(72, 4 * evals)
    ref = np.zeros(4 * evals, np.uint32)
    oracle.bxo_batch_evaluate_any(coeffs, size, which, xs, ref, evals)
    stored = c(coeffs.reshape(npoly, size)[:, bitrev_perm(15)].reshape(-1)) if bitrev else coeffs
    fn = "bx_batch_evaluate_any_bitrev" if bitrev else "bx_batch_evaluate_any"
    return Case("batch_evaluate_any", {"out": rnd(73, 4 * evals), "coeffs": stored, "which": which, "xs": xs},
                [("out", "coeffs"), ("out", "which"), ("out", "xs")], lib_call(fn, ["coeffs", 0, "which", "xs", "out"], npoly), {"out": ref})


_keep = []  # device polynomials the pointer cases name: alive for the module


def case_evaluate_ptrs(oracle, hal):
    size, evals = 1 << 15, 3
    coeffs, xs = rnd(81, 2 * size), rnd(82, 4 * evals)
    dev = hal.copy_from(coeffs)  # the pointed-to polynomials are not operands of the call: their own allocation
    _keep.append(dev)
    cols, flags = [1, 0, 1], np.array([0, 0, 1], np.uint32)
    ptrs = []
    for col in cols:
        addr = dev.raw.dptr + 4 * col * size
        ptrs += [addr & 0xFFFFFFFF, addr >> 32]
    rev, ref = bitrev_perm(15), np.zeros(4 * evals, np.uint32)
    for e, col in enumerate(cols):
        poly = coeffs[col * size:(col + 1) * size]
        oracle.bxo_batch_evaluate_any(c(poly[rev]) if flags[e] else c(poly), size, np.zeros(1, np.uint32), c(xs[4 * e:4 * e + 4]), ref[4 * e:4 * e + 4], 1)
    return Case("batch_evaluate_ptrs", {"out": rnd(83, 4 * evals), "poly_ptrs": np.array(ptrs, np.uint32), "flags": flags, "xs": xs},
                [("out", "poly_ptrs"), ("out", "flags"), ("out", "xs")], lib_call("bx_batch_evaluate_ptrs", ["poly_ptrs", "flags", 0, "xs", "out"], size),
                {"out": ref})


def case_scatter(oracle):
    rng = np.random.default_rng(91)
    into_len, cycles = 1000, 40
    index = np.concatenate([[0], np.cumsum(rng.integers(0, 16, cycles))]).astype(np.uint32)  # ~300 entries: more than one workgroup
    total = int(index[-1])
    offsets, values, init = rng.permutation(into_len)[:total].astype(np.uint32), rnd(92, total), rnd(93, into_len)
    ref = init.copy()
    oracle.bxo_scatter(ref, index, offsets, values, cycles)
    return Case("scatter", {"into": init, "index": index, "offsets": offsets, "values": values}, [("into", "index"), ("into", "offsets"), ("into", "values")],
                lib_call("bx_scatter", ["into", "index", "offsets", "values"]), {"into": ref})


def query_gather_ref(matrix, nodes, rows, cols, positions, top_size):
    depth = int(np.log2(rows // top_size))
    out = np.zeros((len(positions), cols + 8 * depth), np.uint32)
    for q, pos in enumerate(positions):
        out[q, :cols] = matrix.reshape(cols, rows)[:, pos]
        for level in range(depth):
            idx = ((int(pos) + rows) >> level) ^ 1
            out[q, cols + 8 * level:cols + 8 * level + 8] = nodes[8 * idx:8 * idx + 8]
    return out.reshape(-1)


def case_query_gather(oracle):
    rows, cols, top, nq = 256, 3, 16, 8
    matrix, nodes, pos = rnd(101, rows * cols), rnd(102, 16 * rows), np.array([0, 255, 17, 17, 100, 0, 254, 1], np.uint32)  # the gather only copies: any words do
    ref = query_gather_ref(matrix, nodes, rows, cols, pos, top)
    return Case("merkle_query_gather", {"out": rnd(103, ref.size), "matrix": matrix, "nodes": nodes, "positions": pos},
                [("out", "matrix"), ("out", "nodes"), ("out", "positions")],
                lib_call("bx_merkle_query_gather", ["out", "matrix", "nodes", 0, 1, "positions", 2, 3], rows, cols, nq, top), {"out": ref})


def case_transcript(oracle):
    n_commit, n_ext = 2, 3
    state = np.zeros(25, np.uint32)
    state, _ = ol.transcript_step(state, rnd(111, 8).reshape(1, 8), 4)  # a state that has absorbed and handed out before
    digests = rnd(112, 8 * n_commit).reshape(n_commit, 8)
    after, want = ol.transcript_step(state.copy(), digests, 4 * n_ext)
    return Case("transcript_step", {"out_ext": rnd(113, 4 * n_ext), "state": np.concatenate([state, np.zeros(3, np.uint32)]), "digests": digests.reshape(-1)},
                [("out_ext", "state"), ("out_ext", "digests")], lib_call("bx_transcript_step", ["state", "digests", 0, "out_ext", 1], n_commit, n_ext),
                {"out_ext": want, "state": after})


def case_poly_divide(oracle, form):
    size, n_polys = 2049, {"one": 1, "batch": 3, "indexed": 4}[form]  # 2049: two look-back tiles
    polys, zs = rnd(121, 4 * size * n_polys), rnd(122, 4 * 3)
    which = np.array([3, 0, 2], np.uint32)
    divided = {"one": [0], "batch": [0, 1, 2], "indexed": which.tolist()}[form]
    ref, rems = polys.copy().reshape(n_polys, 4 * size), np.zeros((len(divided), 4), np.uint32)
    for q, k in enumerate(divided):
        oracle.bxo_poly_divide(ref[k], size, c(zs[4 * q:4 * q + 4]), rems[q])
    if form == "one":
        return Case("poly_divide", {"rem_out": rnd(123, 4), "poly": polys}, [("rem_out", "poly")], lib_call("bx_poly_divide", ["poly", "host0", "rem_out"], host=[zs]),
                    {"rem_out": rems.reshape(-1), "poly": ref.reshape(-1)})
    data = {"rems_out": rnd(123, 4 * len(divided)), "polys": polys}
    want = {"rems_out": rems.reshape(-1), "polys": ref.reshape(-1)}
    if form == "batch":
        return Case("poly_divide_batch", data, [("rems_out", "polys")], lib_call("bx_poly_divide_batch", ["polys", 0, "host0", "rems_out"], 3, host=[zs]), want)
    return Case("poly_divide_batch_indexed", data, [("rems_out", "polys")],
                lib_call("bx_poly_divide_batch_indexed", ["polys", 0, 1, "host0", "host1", "rems_out"], n_polys, 3, host=[which, zs]), want)


def case_gather(oracle):
    idx, size, stride = 5, 300, 3
    src = rnd(131, 1000)
    ref = np.zeros(size, np.uint32)
    oracle.bxo_gather_sample(ref, src, idx, size, stride)
    return Case("gather_sample", {"dst": rnd(132, size), "src": src}, [("dst", "src")], lib_call("bx_gather_sample", ["dst", "src", 0, 1, 2], idx, size, stride),
                {"dst": ref})


def case_add(oracle):
    n = 1000
    a, b = rnd(141, n), rnd(142, n)
    ref = np.zeros(n, np.uint32)
    oracle.bxo_eltwise_add(ref, a, b, n)
    return Case("eltwise_add_elem", {"out": rnd(143, n), "a": a, "b": b}, [("out", "a"), ("out", "b")], lib_call("bx_eltwise_add_elem", ["out", "a", "b"]),
                {"out": ref}, alias_ok=[("out", "a"), ("out", "b")])


def case_copy(oracle, d2d):
    n = 1000
    x = rnd(151, n)
    if d2d:
        return Case("bx_d2d", {"dst": rnd(152, n), "src": x}, [("dst", "src")], lib_call("bx_d2d", ["dst", "src", 0], n), {"dst": x}, alias_ok=[("dst", "src")])
    return Case("eltwise_copy_elem", {"out": rnd(152, n), "in": x}, [("out", "in")], lib_call("bx_eltwise_copy_elem", ["out", "in"]), {"out": x},
                alias_ok=[("out", "in")])


def case_logup(oracle):
    n, count = 700, 3  # 2100 elements: more than one 2048-element tile under both scan paths
    d, m = rnd(161, 4 * n * count), rnd(162, n * count)
    return Case("logup_accumulate", {"out": rnd(163, 4 * n * count), "denoms": d, "mults": m}, [("out", "denoms"), ("out", "mults")],
                lib_call("bx_logup_accumulate", ["out", "denoms", "mults", 0], count), {"out": R.logup_accumulate(d, m, count)},
                alias_ok=[("out", "denoms")])


def case_expand(oracle):
    n, bits = 1 << 12, 2
    x = rnd(171, n)
    ref = np.zeros(n << bits, np.uint32)
    oracle.bxo_batch_expand_into_evaluate_ntt(ref, x, 1, n, bits)
    return Case("batch_expand_into_evaluate_ntt", {"out": rnd(172, n << bits), "in": x}, [("out", "in")],
                lib_call("bx_batch_expand_into_evaluate_ntt", ["out", "in", 0, 1], 1, bits), {"out": ref})


BUILDERS = {
    "fri_fold": lambda o, h: case_fri_fold(o, False), "fri_fold_dev": lambda o, h: case_fri_fold(o, True),
    "mix_x4": lambda o, h: case_mix(o, 1000), "mix_one_word": lambda o, h: case_mix(o, 1001),
    "eltwise_sum_extelem": lambda o, h: case_sum_ext(o), "hash_rows": lambda o, h: case_hash_rows(o), "merkle_build": lambda o, h: case_merkle_build(o),
    "hash_fold_indexed": lambda o, h: case_hash_fold_indexed(o),
    "batch_evaluate_any": lambda o, h: case_evaluate_any(o, False), "batch_evaluate_any_bitrev": lambda o, h: case_evaluate_any(o, True),
    "batch_evaluate_ptrs": lambda o, h: case_evaluate_ptrs(o, h), "scatter": lambda o, h: case_scatter(o), "merkle_query_gather": lambda o, h: case_query_gather(o),
    "transcript_step": lambda o, h: case_transcript(o),
    "poly_divide": lambda o, h: case_poly_divide(o, "one"), "poly_divide_batch": lambda o, h: case_poly_divide(o, "batch"),
    "poly_divide_batch_indexed": lambda o, h: case_poly_divide(o, "indexed"), "gather_sample": lambda o, h: case_gather(o),
    "eltwise_add_elem": lambda o, h: case_add(o), "eltwise_copy_elem": lambda o, h: case_copy(o, False), "bx_d2d": lambda o, h: case_copy(o, True),
    "logup_accumulate": lambda o, h: case_logup(o), "batch_expand_into_evaluate_ntt": lambda o, h: case_expand(o),
}
_cases = {}


def get_case(key, oracle, hal):
    if key not in _cases:
        _cases[key] = BUILDERS[key](oracle, hal)
    return _cases[key]


def overlap_suite(hal, case):
    """every pair of the case: the four overlapping placements refused with nothing written, then the touching ones accepted and right"""
    for pair in case.pairs:
        for kind in ("over_hi", "over_lo", "contain", "alias"):
            if kind == "alias" and pair in case.alias_ok:
                continue  # the allowed aliases have tests of their own below
            a = place(hal, case, pair, kind)
            text = refused(case.call(hal, a.raw), case.name)
            assert pair[0] in text and pair[1] in text, text
            if kind == "over_hi":
                print(f"REFUSAL {case.name} [{pair[0]} / {pair[1]}, one word]: {text}")
            a.unchanged(f"{case.name} {pair} {kind}")
            a.free()
        touched = 0
        for kind in ("touch_after", "touch_before"):  # ... and the ctx goes on to compute a valid call
            a = place(hal, case, pair, kind, seed=2)
            if a is None:
                continue
            msg = case.call(hal, a.raw)
            assert msg is None, f"{case.name} {pair} {kind}: touching operands were refused: {msg}"
            a.check(case.want, f"{case.name} {pair} {kind}", case.ignore)
            a.free()
            touched += 1
            print(f"TOUCHING {case.name} [{pair[0]} / {pair[1]}, {kind}]: accepted")
        assert touched, "no touching placement keeps the operands aligned"


@pytest.mark.parametrize("key", [k for k in BUILDERS if k != "gather_sample"])
def test_overlapping_operands_are_refused_and_touching_ones_accepted(hal, oracle, key):
    overlap_suite(hal, get_case(key, oracle, hal))


@pytest.mark.parametrize("defer", [1, 0], ids=["queued", "direct"])
def test_gather_sample_refuses_a_dst_inside_its_src_on_both_paths(hal, oracle, defer):
    hal.set_tunable("gather_defer", defer)
    try:
        overlap_suite(hal, get_case("gather_sample", oracle, hal))
        # a queued gather is not lost to a refusal that follows it
        case = get_case("gather_sample", oracle, hal)
        ok, bad = place(hal, case, ("dst", "src"), "touch_after", seed=3), place(hal, case, ("dst", "src"), "contain", seed=4)
        assert case.call(hal, ok.raw) is None
        refused(case.call(hal, bad.raw), "gather_sample")
        ok.check(case.want, "a gather queued before a refused one")
        bad.unchanged("the refused gather")
        ok.free()
        bad.free()
    finally:
        hal.set_tunable("gather_defer", 1)


# ---------------------------------------------------------------------------------------------------------------- allowed aliases
@pytest.mark.parametrize("form", ["out_is_a", "out_is_b", "a_is_b", "all_three", "a_overlaps_b"])
def test_eltwise_add_elem_alias_forms(hal, oracle, form):
    n = 1000
    x, y, z = rnd(201, n), rnd(202, n), rnd(203, n + n // 2)
    a, b = {"out_is_a": (x, y), "out_is_b": (x, y), "a_is_b": (x, x), "all_three": (x, x), "a_overlaps_b": (z[:n], z[n // 2:])}[form]
    ref = np.zeros(n, np.uint32)
    oracle.bxo_eltwise_add(ref, c(a), c(b), n)  # from copies of the inputs
    host = np.random.default_rng(5).integers(0, 1 << 32, 4 * n + 5 * PAD, dtype=np.uint32)
    o1, o2, o3 = PAD, 2 * PAD + n, 3 * PAD + 2 * n  # three regions; o3 has room for 1.5 n
    off = {"out_is_a": (o1, o1, o2), "out_is_b": (o2, o1, o2), "a_is_b": (o1, o2, o2), "all_three": (o1, o1, o1), "a_overlaps_b": (o1, o3, o3 + n // 2)}[form]
    if form == "a_overlaps_b":
        host[o3:o3 + z.size] = z
    else:
        host[off[1]:off[1] + n] = a
        host[off[2]:off[2] + n] = b
    dev = hal.copy_from(host)
    hal.eltwise_add_elem(dev.slice(off[0], n), dev.slice(off[1], n), dev.slice(off[2], n))
    want = host.copy()
    want[off[0]:off[0] + n] = ref
    assert np.array_equal(dev.view(), want), form
    dev.free()


def test_a_copy_onto_itself_is_a_no_op_and_d2d_compares_the_words_it_moves(hal):
    host = np.random.default_rng(6).integers(0, 1 << 32, 1200, dtype=np.uint32)
    dev = hal.copy_from(host)
    hal.eltwise_copy_elem(dev.slice(100, 900), dev.slice(100, 900))
    assert hal.lib.bx_d2d(hal.ctx, dev.slice(100, 900).raw, dev.slice(100, 1000).raw, 900) is None  # same start: the len fields play no part
    assert np.array_equal(dev.view(), host)
    # two views whose len fields overlap, the 200 words moved do not: [100, 300) <- [300, 500)
    dst, src = dev.slice(100, 500).raw, dev.slice(300, 500).raw
    refused(hal.lib.bx_d2d(hal.ctx, dst, src, 201), "bx_d2d")
    refused(hal.lib.bx_d2d(hal.ctx, src, dst, 201), "bx_d2d")
    assert np.array_equal(dev.view(), host)
    assert hal.lib.bx_d2d(hal.ctx, dst, src, 200) is None
    want = host.copy()
    want[100:300] = host[300:500]
    assert np.array_equal(dev.view(), want)
    dev.free()


@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "three_phase"])
def test_logup_accumulate_out_is_denoms(hal, oracle, lookback):
    case = get_case("logup_accumulate", oracle, hal)
    hal.set_tunable("scan_lookback", lookback)
    try:
        a = place(hal, case, ("out", "denoms"), "alias")  # the higher name's words stand where two operands alias: "out" < "denoms" by offset tie
        a.host[a.offsets["denoms"]:a.offsets["denoms"] + case.data["denoms"].size] = case.data["denoms"]
        a.dev.copy_from(a.host)
        assert case.call(hal, a.raw) is None
        a.check({"out": case.want["out"]}, "logup_accumulate out = denoms")
        a.free()
    finally:
        hal.set_tunable("scan_lookback", 1)


def test_expand_in_place_only_without_expansion(hal, oracle):
    n = 1 << 12
    x = rnd(211, 4 * n)
    # in = the last quarter of out, expand_bits = 2: the natural way to expand in place, and a race between lanes
    host = np.concatenate([rnd(212, PAD), rnd(213, 3 * n), x[:n], rnd(214, PAD)])
    dev = hal.copy_from(host)
    text = refused(hal.lib.bx_batch_expand_into_evaluate_ntt(hal.ctx, dev.slice(PAD, 4 * n).raw, dev.slice(PAD + 3 * n, n).raw, 1, 2), "batch_expand_into_evaluate_ntt")
    print("REFUSAL batch_expand_into_evaluate_ntt [in = last quarter of out]:", text)
    refused(hal.lib.bx_batch_expand_into_evaluate_ntt(hal.ctx, dev.slice(PAD, 4 * n).raw, dev.slice(PAD, n).raw, 1, 2), "batch_expand_into_evaluate_ntt")
    assert np.array_equal(dev.view(), host)
    dev.free()
    # out = in, expand_bits = 0: batch_evaluate_ntt
    for count in (1, 4):
        host = np.concatenate([rnd(215, PAD), x, rnd(216, PAD)])
        dev = hal.copy_from(host)
        io = dev.slice(PAD, 4 * n)
        hal.batch_expand_into_evaluate_ntt(io, io, count, 0)
        ref = x.copy()
        oracle.bxo_batch_evaluate_ntt(ref, count, 4 * n // count, 0)
        want = host.copy()
        want[PAD:PAD + 4 * n] = ref
        assert np.array_equal(dev.view(), want), count
        # a partial overlap stays refused without expansion too
        refused(hal.lib.bx_batch_expand_into_evaluate_ntt(hal.ctx, dev.slice(PAD, 2 * n).raw, dev.slice(PAD + n, 2 * n).raw, 1, 0), "batch_expand_into_evaluate_ntt")
        dev.free()


# ---------------------------------------------------------------------------------------------------------------- index contents
def combo_patterns(rng, input_size):
    """name -> (combos, n_combos)"""
    i = np.arange(input_size)
    return {
        "all_same": (np.full(input_size, 1), 3),
        "descending": (3 - (4 * i) // input_size, 4),
        "one_unused": (rng.choice([0, 1, 3], input_size), 4),
        "first_unused": (rng.integers(1, 3, input_size), 3),
        "last_unused": (rng.integers(0, 2, input_size), 3),
        "more_combos_than_inputs": (rng.permutation(input_size + 1)[:input_size], input_size + 1),
    }


@pytest.mark.parametrize("count", [6, 1001, 8, 1000])
@pytest.mark.parametrize("input_size", [1, 1023, 1024, 1025, 1300])
def test_mix_poly_coeffs_combo_patterns(hal, oracle, input_size, count):
    """input_size crosses the two counting sorts of mix_prep_kernel (an LDS ranking up to 1024 columns, one thread's loop above); count 6 and
    1001 take the one-word kernel, 8 and 1000 the four-word one.  Rows of combos no column names come back as they were."""
    rng = np.random.default_rng(1000 * input_size + count)
    inp, start, mix = rnd(input_size + count, input_size * count), rnd(301, 4), rnd(302, 4)
    d_in = hal.copy_from(inp)
    for name, (combos, n_combos) in combo_patterns(rng, input_size).items():
        combos = c(combos)
        assert combos.max() < n_combos
        init = rng.integers(0, P, 4 * count * n_combos, dtype=np.uint32)
        ref = init.copy()
        oracle.bxo_mix_poly_coeffs(ref, start, mix, inp, combos, input_size, count)
        out, d_combos = hal.copy_from(init), hal.copy_from(combos)
        hal.mix_poly_coeffs(out, start, mix, d_in, d_combos, input_size, count)
        got = out.view().reshape(n_combos, 4 * count)
        assert np.array_equal(got.reshape(-1), ref), (name, input_size, count)
        unused = np.setdiff1d(np.arange(n_combos), combos)
        assert unused.size or name == "descending", name  # every other pattern leaves a combo without columns
        assert np.array_equal(got[unused], init.reshape(n_combos, 4 * count)[unused]), name
        out.free()
        d_combos.free()
    d_in.free()


def which_patterns(evals, poly_count):
    i = np.arange(evals)
    return {"all_first": 0 * i, "all_last": 0 * i + poly_count - 1, "all_duplicated": (i // 2) % poly_count if evals > 1 else 0 * i,
            "descending": np.sort(i % poly_count)[::-1]}


_eval_polys = {}


def eval_polys(hal, bitrev):
    """three polynomials, shared by every case: (host natural order, device buffer as the entry point wants it, size)"""
    if bitrev not in _eval_polys:
        size = 1 << 15 if bitrev else 300
        coeffs = rnd(311, 3 * size)
        stored = c(coeffs.reshape(3, size)[:, bitrev_perm(15)].reshape(-1)) if bitrev else coeffs
        _eval_polys[bitrev] = (coeffs, hal.copy_from(stored), size)
    return _eval_polys[bitrev]


@pytest.mark.parametrize("evals", [1, 63, 64, 65])
@pytest.mark.parametrize("entry", ["any", "bitrev", "ptrs"])
def test_batch_evaluate_which_patterns(hal, oracle, entry, evals):
    """duplicate and boundary `which` (or pointers) at the widths around eval_final_kernel's 64-lane block"""
    coeffs, dev, size = eval_polys(hal, entry != "any")
    xs = rnd(320 + evals, 4 * evals)
    d_xs = hal.copy_from(xs)
    rev = bitrev_perm(15)
    for name, which in which_patterns(evals, 3).items():
        which = c(which)
        out, ref = hal.copy_from(rnd(321, 4 * evals)), np.zeros(4 * evals, np.uint32)
        if entry == "ptrs":  # the same pointer repeated with differing flags: flag 1 reads the stored words as bit-reversed coefficients
            flags = c(np.arange(evals) % 2)
            addrs = [dev.raw.dptr + 4 * int(w) * size for w in which]
            ptrs = c([half for a in addrs for half in (a & 0xFFFFFFFF, a >> 32)])
            stored = coeffs.reshape(3, size)[:, rev]  # what the device holds
            for e in range(evals):
                poly = stored[which[e]][rev] if flags[e] else stored[which[e]]
                oracle.bxo_batch_evaluate_any(c(poly), size, np.zeros(1, np.uint32), c(xs[4 * e:4 * e + 4]), ref[4 * e:4 * e + 4], 1)
            hal.batch_evaluate_ptrs(hal.copy_from(ptrs), hal.copy_from(flags), size, d_xs, out)
        else:
            oracle.bxo_batch_evaluate_any(coeffs, size, which, xs, ref, evals)
            (hal.batch_evaluate_any_bitrev if entry == "bitrev" else hal.batch_evaluate_any)(dev, 3, hal.copy_from(which), d_xs, out)
        assert np.array_equal(out.view(), ref), (entry, name, evals)
        out.free()
    d_xs.free()


def test_hash_fold_indexed_selector_patterns(hal, oracle):
    n = 37
    digs = rnd(331, 8 * n).reshape(n, 8)
    base = [(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (3, 5), (3, 5), (3, 5), (7, 7), (0, 1), (n - 2, n - 1)]
    d_in = hal.copy_from(digs.reshape(-1))
    for sel in (base, base * 30, [(0, 0)] * 257, [(n - 1, n - 1)] * 257, [(3, 5)] * 300):  # 300 > one 256-lane workgroup
        sel = np.array(sel, np.uint32)
        count = len(sel)
        out = hal.copy_from(rnd(332, 8 * count))
        hal._check(hal.lib.bx_hash_fold_indexed(hal.ctx, out.raw, d_in.raw, hal.copy_from(sel.reshape(-1)).raw, count))
        uniq, inverse = np.unique(sel, axis=0, return_inverse=True)
        want = hash_pairs(oracle, digs, uniq).reshape(-1, 8)[inverse.reshape(-1)]
        assert np.array_equal(out.view(), want.reshape(-1)), count
        out.free()
    d_in.free()


@pytest.mark.parametrize("rows,cols,top_size", [(2, 1, 2), (2, 1, 1), (256, 3, 1), (256, 300, 16), (4096, 257, 4096)])
def test_merkle_query_gather_positions(hal, oracle, rows, cols, top_size):
    """depth 0 (top_size = rows), full depth (top_size = 1) and cols past one 256-lane trip, at the first and the last row, a repeated
    position and random ones.  The tree is bx_merkle_build's (oracle-checked elsewhere): fetched, and indexed with numpy."""
    rng = np.random.default_rng(rows + cols)
    matrix = rnd(341, rows * cols)
    d_matrix, d_nodes = hal.copy_from(matrix), hal.alloc_digest(2 * rows)
    hal.merkle_build(d_nodes, d_matrix, rows)
    nodes = d_nodes.view()
    depth = int(np.log2(rows // top_size))
    r = int(rng.integers(0, rows))
    fifty = np.concatenate([[0, rows - 1, r, r, rows - 1, 0], rng.integers(0, rows, 44)]).astype(np.uint32)
    for positions in ([0], [rows - 1], fifty):
        positions = c(positions)
        nq = positions.size
        want = query_gather_ref(matrix, nodes, rows, cols, positions, top_size)
        assert want.size == nq * (cols + 8 * depth)
        guard = rnd(342, want.size + 2 * PAD)
        dev = hal.copy_from(guard)
        hal._check(hal.lib.bx_merkle_query_gather(hal.ctx, dev.slice(PAD, want.size).raw, d_matrix.raw, d_nodes.raw, rows, cols, hal.copy_from(positions).raw, nq, top_size))
        guard[PAD:PAD + want.size] = want
        assert np.array_equal(dev.view(), guard), (rows, cols, top_size, nq)
        dev.free()
    assert np.array_equal(d_nodes.view(), nodes) and np.array_equal(d_matrix.view(), matrix)
    d_matrix.free()
    d_nodes.free()


@pytest.mark.parametrize("index", [[7, 7], [0, 0], [3, 6, 10], [0, 0, 4, 4, 4, 9, 9], [2, 2, 2], [5, 5, 12, 12]],
                         ids=["empty", "empty_at_0", "starts_above_0", "repeated_boundaries", "empty_cycles_only", "both"])
def test_scatter_index_shapes(hal, oracle, index):
    rng = np.random.default_rng(len(index))
    into_len, total = 600, 300
    index = c(index)
    offsets, values, init = rng.permutation(into_len)[:total].astype(np.uint32), rnd(351, total), rnd(352, into_len)
    ref = init.copy()
    oracle.bxo_scatter(ref, index, offsets, values, index.size - 1)
    assert (index[0] != index[-1]) or np.array_equal(ref, init)  # the empty range writes nothing
    dst = hal.copy_from(init)
    hal.scatter(dst, hal.copy_from(index), hal.copy_from(offsets), hal.copy_from(values))
    assert np.array_equal(dst.view(), ref)
    written = np.zeros(into_len, bool)
    written[offsets[index[0]:index[-1]]] = True
    assert np.array_equal(ref[~written], init[~written]) and np.array_equal(ref[offsets[index[0]:index[-1]]], values[index[0]:index[-1]])  # the oracle, by numpy
    dst.free()


@pytest.mark.parametrize("subset", ["reversed", "strided"])
@pytest.mark.parametrize("count", [1, 8, 9, 16])
def test_poly_divide_batch_indexed_subsets(hal, oracle, count, subset):
    """eight sequences per launch: 8, 9 and 16 divisions are one launch, one and a single, two full ones — over a permuted `which`"""
    n_polys, size = 20, 2049
    polys, zs = rnd(361, 4 * size * n_polys), rnd(362 + count, 4 * count)
    which = c(np.arange(n_polys)[::-1][:count] if subset == "reversed" else (7 * np.arange(count) + 3) % n_polys)
    assert np.unique(which).size == count
    ref, want_rems = polys.copy().reshape(n_polys, 4 * size), np.zeros((count, 4), np.uint32)
    for q, k in enumerate(which):
        oracle.bxo_poly_divide(ref[k], size, c(zs[4 * q:4 * q + 4]), want_rems[q])
    buf, rems = hal.copy_from(polys), hal.copy_from(rnd(363, 4 * count + 8))
    hal._check(hal.lib.bx_poly_divide_batch_indexed(hal.ctx, buf.raw, n_polys, count, u32p(which), u32p(zs), rems.slice(0, 4 * count).raw))
    got = buf.view().reshape(n_polys, 4 * size)
    assert np.array_equal(got, ref)
    untouched = np.setdiff1d(np.arange(n_polys), which)
    assert np.array_equal(got[untouched], polys.reshape(n_polys, 4 * size)[untouched])
    assert np.array_equal(rems.view()[:4 * count], want_rems.reshape(-1)) and np.array_equal(rems.view()[4 * count:], rnd(363, 4 * count + 8)[4 * count:])
    buf.free()
    rems.free()


def test_poly_divide_batch_indexed_refuses_bad_host_indices(hal):
    n_polys, size, count = 20, 2049, 9
    polys, zs, r0 = rnd(371, 4 * size * n_polys), rnd(372, 4 * count), rnd(373, 4 * count)
    buf, rems = hal.copy_from(polys), hal.copy_from(r0)
    dup = c([19, 3, 7, 0, 11, 3, 5, 1, 2])
    msg = hal.lib.bx_poly_divide_batch_indexed(hal.ctx, buf.raw, n_polys, count, u32p(dup), u32p(zs), rems.raw)
    assert msg and b"once per call" in msg, msg
    beyond = c([19, 3, 7, 0, 11, 4, 5, 1, n_polys])
    msg = hal.lib.bx_poly_divide_batch_indexed(hal.ctx, buf.raw, n_polys, count, u32p(beyond), u32p(zs), rems.raw)
    assert msg and b"out of range" in msg, msg
    assert np.array_equal(buf.view(), polys) and np.array_equal(rems.view(), r0)
    buf.free()
    rems.free()


@pytest.mark.parametrize("defer", [1, 0], ids=["queued", "direct"])
def test_gather_sample_index_edges(hal, oracle, defer):
    src = rnd(381, 10000)
    d_src = hal.copy_from(src)
    hal.set_tunable("gather_defer", defer)
    try:
        # (idx, size, stride): stride 0 with size > 1; the queue's limit and one past it; the last word; a stride past 32 bits (direct path)
        for idx, size, stride in ((77, 300, 0), (3, 4096, 2), (3, 4097, 2), (5, 4096, 1), (5, 4097, 1), (src.size - 1, 1, 1), (src.size - 1, 1, 0),
                                  (9, 1, (1 << 32) + 1), (0, 1, (1 << 63))):
            guard = rnd(382, size + 2 * PAD)
            dev = hal.copy_from(guard)
            hal.gather_sample(dev.slice(PAD, size), d_src, idx, size, stride)
            guard[PAD:PAD + size] = src[idx + np.arange(size) * (stride if size > 1 else 0)]
            assert np.array_equal(dev.view(), guard), (idx, size, stride)
            dev.free()
        from boundless_amd.hal import HalError

        with pytest.raises(HalError, match="out of range"):
            hal.gather_sample(hal.alloc(2), d_src, src.size - 1, 2, 1)
    finally:
        hal.set_tunable("gather_defer", 1)
    d_src.free()


# ---------------------------------------------------------------------------------------------------------------- branches beyond the workload's shapes
def mont_mul(x, f):
    """Montgomery product x * f * 2^-32 mod P over a whole array, in 64-bit integers"""
    rinv = np.uint64(pow(1 << 32, -1, P))
    t = (x.astype(np.uint64) * np.uint64(f)) % np.uint64(P)
    return ((t * rinv) % np.uint64(P)).astype(np.uint32)


def test_eltwise_kernels_take_a_second_grid_stride_trip(hal, oracle):
    """65536 blocks x 256 lanes + 5 words: the last five words are a lane's second trip (hal_operand_sizes.py; the thresholds are
    asserted against the sources by test_operand_overlap_check_cpu.py)"""
    n = sizes.ELTWISE_WORDS
    t0 = time.time()
    rng = np.random.default_rng(401)
    a, b = rng.integers(0, P, n, dtype=np.uint32), rng.integers(0, P, n, dtype=np.uint32)
    da, db, out = hal.copy_from(a), hal.copy_from(b), hal.alloc(n)
    hal.eltwise_add_elem(out, da, db)
    s = a.astype(np.uint64) + b
    assert np.array_equal(out.view(), np.where(s >= P, s - P, s).astype(np.uint32)), "eltwise_add_elem"
    ref = np.zeros(1000, np.uint32)
    oracle.bxo_eltwise_add(ref, c(a[-1000:]), c(b[-1000:]), 1000)  # the oracle on the tail, where the second trip is
    assert np.array_equal(out.slice(n - 1000, 1000).view(), ref)
    out.free()
    db.free()
    f = int(rnd(402, 1)[0])
    hal.eltwise_mul_factor(da, f)
    assert np.array_equal(da.view(), mont_mul(a, f)), "eltwise_mul_factor"
    assert int(mont_mul(a[-3:], f)[0]) == oracle.bxo_fp_mul(int(a[-3]), f)
    da.free()
    z = a
    z[::3] = 0xFFFFFFFF
    z[-5:] = [0xFFFFFFFF, 7, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]
    dz = hal.copy_from(z)
    hal.eltwise_zeroize_elem(dz)
    assert np.array_equal(dz.view(), np.where(z == 0xFFFFFFFF, 0, z).astype(np.uint32)), "eltwise_zeroize_elem"
    dz.free()
    print(f"WALL eltwise at {n} words: {time.time() - t0:.2f} s")


def test_poly_divide_takes_a_third_level(hal, oracle):
    """2^21 + 1 coefficients: divide_rec chunks three times before its one-workgroup kernel — under scan_lookback = 0, and under the
    default on a slice that is only word aligned (which the look-back kernel does not take)"""
    n = sizes.DIVIDE_N
    t0 = time.time()
    poly, z = rnd(411, 4 * n), rnd(412, 4)
    ref, ref_rem = poly.copy(), np.zeros(4, np.uint32)
    oracle.bxo_poly_divide(ref, n, c(z), ref_rem)
    whole = hal.alloc(4 * n + 8)
    rem = hal.alloc(4)
    try:
        for lookback, off in ((0, 0), (1, 1)):
            hal.set_tunable("scan_lookback", lookback)
            buf = whole.slice(off, 4 * n)
            buf.copy_from(poly)
            hal.poly_divide(buf, z, rem)
            assert np.array_equal(buf.view(), ref), (lookback, off)
            assert np.array_equal(rem.view(), ref_rem), (lookback, off)
    finally:
        hal.set_tunable("scan_lookback", 1)
    whole.free()
    rem.free()
    print(f"WALL poly_divide at {n} elements: {time.time() - t0:.2f} s")


def test_prefix_scans_take_a_third_level(hal, oracle):
    """2^23 + 1 elements under scan_lookback = 0: three_phase_rec chunks three times.  Products against the C oracle; sums against
    numpy's cumulative sum per coefficient plane (addition is the same in Montgomery form; 2^23 words below 2^31 fit 64 bits)"""
    n = sizes.SCAN_N
    t0 = time.time()
    x = np.random.default_rng(421).integers(0, P, 4 * n, dtype=np.uint32)
    buf = hal.alloc(4 * n)
    try:
        hal.set_tunable("scan_lookback", 0)
        buf.copy_from(x)
        hal.prefix_sums(buf)
        want = (np.cumsum(x.reshape(n, 4).astype(np.uint64), axis=0) % np.uint64(P)).astype(np.uint32).reshape(-1)
        assert np.array_equal(buf.view(), want), "prefix_sums"
        small = R.prefix_sums(x[:4 * 100])
        assert np.array_equal(want[:4 * 100], small)  # the numpy statement against the suite's big-integer reference
        del want
        buf.copy_from(x)
        hal.prefix_products(buf)
        oracle.bxo_prefix_products(x, n)
        assert np.array_equal(buf.view(), x), "prefix_products"
    finally:
        hal.set_tunable("scan_lookback", 1)
    buf.free()
    print(f"WALL prefix scans at {n} elements: {time.time() - t0:.2f} s")
