"""GPU: a witness program's sorted columns (include/bx_program.h "sorted columns", csrc/wit_sort.hip) — the device radix sort against
the definition-level reference of tests/wit_sort_ref.py and against the host executor, word for word over the whole data group with
the dests poisoned first; every key shape, key pattern, `rows` and payload count on one grid; extreme words; cells at or above
2^bits; a SET column as a key; a dest as a count's source; two sorts in one program; several workgroups with several tiles each; the
work space; the profile names; a generated per-row kernel followed by the sorts; the entry point's refusals; what a ctx holds; and a
sorted range check with no built-in circuit behind it against its all-numpy twin, seal for seal.

Sizes are the smallest at which each thing can break: po2 1 (two rows), 6 and 7 (less than one workgroup: lanes hold no element), 8 (one
workgroup's width), 9 (the prover's smallest), 12 (four tiles, two workgroups of two tiles), 14 for a pass of eight workgroups."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import wit_count_ref as cref  # noqa: E402
import wit_sort_ref as sref  # noqa: E402

from boundless_amd.circuit import CircuitOps  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P, POISON = sref.P, sref.POISON
W_CODE = sref.WIDTHS[0]
TILE = 1024  # WS_TILE of csrc/wit_sort.hip: 256 lanes x 4 trips; a workgroup takes at least two tiles when there are that many


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def _code(po2, seed=1):
    return sref.random_columns((W_CODE, 1 << po2), seed=seed)


def _check(hal, prog, po2, w_data, code, data, what, loaded=None, compiled=None):
    """the device, the host executor and the reference agree on every word of `data`; every column that is no dest and the rows at or
    above a sort's `rows` are left alone; a dest is a permutation of its source's words -> the data group after the run"""
    n = 1 << po2
    own = compiled is None
    if own:
        compiled = sref.compile_ref(prog)
        loaded = compiled.load(hal)
    try:
        want = sref.evaluate(prog, po2, code, data)
        host = data.copy()
        compiled.run_host(po2, code, W_CODE, host, w_data)
        dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        loaded.run(po2, dcode, W_CODE, ddata, w_data)
        got = ddata.view().reshape(w_data, n).copy()
        assert np.array_equal(dcode.view(), code.reshape(-1)), f"{what}: the code group was written"
        dcode.free()
        ddata.free()
    finally:
        if own:
            loaded.unload()
            compiled.close()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} data words differ from the reference, first at (column, row) {tuple(bad[0])}: " \
                          f"{int(got[tuple(bad[0])])} for {int(want[tuple(bad[0])])}"
    assert np.array_equal(host, want), f"{what}: the host executor differs from the reference"
    free = [c for c in range(w_data) if c not in prog.written()]
    assert np.array_equal(got[free], data[free]), f"{what}: a column that is no dest was written"
    for keys, payload, dests, rows in prog.sorts:
        rows = rows or n
        assert np.all(got[dests, rows:] == POISON), f"{what}: a row at or above rows = {rows} of a dest was written"
        for src, dst in zip([c for c, _ in keys] + payload, dests):
            assert np.array_equal(np.sort(got[dst, :rows]), np.sort(got[src, :rows])), f"{what}: dest {dst} is no permutation of source {src}"
    return got


KEY_SHAPES = ((1,), (8,), (9,), (13,), (31,), (24, 20), (16, 16, 16, 16))


def _grid_data(prog, po2, w_data, n_keys, n_payload, kind):
    n = 1 << po2
    data = sref.random_columns((w_data, n), seed=po2)
    for k in range(n_keys):
        data[k] = sref.key_column(kind, n, seed=7 * po2 + k)
    if n_payload:
        data[n_keys] = sref.encode_words(np.arange(n))  # the row itself rides along: stability is visible
    data[prog.written()] = POISON
    return data


@pytest.mark.parametrize("po2", [1, 6, 7, 8, 9, 12])
def test_run_is_the_reference_and_the_host_executor_on_the_whole_grid(hal, po2):
    """key shapes x payload counts {0, 1, 15 - n_keys} x rows {0, 1, 2, N - 3, N} x key patterns"""
    n = 1 << po2
    code = _code(po2)
    for bits in KEY_SHAPES:
        for n_payload in (0, 1, 15 - len(bits)):
            for rows in sorted({0, 1, 2, max(n - 3, 1), n}):
                prog, w_data = sref.sort_program(bits, n_payload, rows)
                compiled = sref.compile_ref(prog)
                loaded = compiled.load(hal)
                try:
                    for kind in sref.KEY_PATTERNS:
                        data = _grid_data(prog, po2, w_data, len(bits), n_payload, kind)
                        got = _check(hal, prog, po2, w_data, code, data, f"po2 {po2}, bits {bits}, payload {n_payload}, rows {rows}, {kind}", loaded, compiled)
                        eff, w = rows or n, len(bits) + n_payload
                        if (kind == "equal" or (kind == "ascending" and 1 << bits[0] >= n)) and n_payload:  # nothing moves: ties stay in row order
                            assert np.array_equal(got[w + len(bits), :eff], sref.encode_words(np.arange(eff)))
                        if kind == "descending" and bits == (31,) and n_payload:
                            assert np.array_equal(got[w + 1, :eff], sref.encode_words(np.arange(eff)[::-1]))
                finally:
                    loaded.unload()
                    compiled.close()


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_run_is_the_reference_on_extreme_columns(hal, pattern):
    po2, n = 7, 128
    prog = sref.two_sorts_program(rows_a=0, rows_b=125)
    data = np.zeros((8, n), np.uint32) if pattern == "zero" else extreme_words.pattern(pattern, (8, n), seed=3)
    data[prog.written()] = POISON
    _check(hal, prog, po2, 8, _code(po2), data, pattern)


def test_cells_at_or_above_two_to_the_bits_sort_by_their_low_bits(hal):
    po2, n = 8, 256
    for bits in (1, 3, 9):
        prog, w = sref.sort_program((bits,), 1)
        values = (np.arange(n) * 37 + (1 << bits) * (np.arange(n) % 5)) % 100000
        data = np.zeros((w, n), np.uint32)
        data[0], data[1] = sref.encode_words(values), sref.encode_words(np.arange(n))
        data[2:] = POISON
        got = _check(hal, prog, po2, w, _code(po2), data, f"bits {bits}")
        moved, from_row = np.array(sref.decode_ints(got[2])), np.array(sref.decode_ints(got[3]))
        keys = moved & ((1 << bits) - 1)
        assert (values >= 1 << bits).any() and np.all(np.diff(keys) >= 0) and len(set(keys.tolist())) > 1
        assert np.array_equal(moved, values[from_row]), "the word that moved is not the source's"
        assert all(from_row[i] < from_row[i + 1] for i in range(n - 1) if keys[i] == keys[i + 1]), "ties are not in ascending row order"


@pytest.mark.parametrize("po2", [6, 9])
def test_a_set_column_as_a_key_a_dest_as_a_counts_source_and_two_sorts(hal, po2):
    n = 1 << po2
    for name, prog in (("set_key", sref.set_key_program(rows=n - 3)), ("sorted_count", sref.sorted_count_program(40, rows=n - 1)),
                       ("two_sorts", sref.two_sorts_program(rows_a=n - 1, rows_b=0))):
        data = sref.random_columns((8, n), seed=po2)
        data[0] = sref.encode_words(np.random.default_rng(po2).integers(0, 60, n))  # small values: the count has something to count
        data[prog.written()] = POISON
        got = _check(hal, prog, po2, 8, _code(po2), data, f"{name} at po2 {po2}")
        if name == "set_key":
            assert not np.any(got[3] == POISON)
        if name == "sorted_count":  # the count saw the sorted column, not the poison that was there before the sorts
            assert int(cref.decode_words(got[6, :n - 1]).sum()) == int(np.sum(cref.decode_words(got[[5, 1], :n - 1]) < 40)) > n // 2


def test_several_workgroups_of_several_tiles_with_equal_digits_across_tile_boundaries(hal):
    """po2 14, rows N - 3 = 16 381: 16 tiles of TILE rows (the last one short), 8 workgroups of 2 tiles.  Keys r // 1000 give runs of
    1000 equal digits that straddle every tile boundary, r % 7 gives every wave the same few digits again and again, and 13 bits are
    two passes, the second with 5 live bits."""
    po2 = 14
    n = 1 << po2
    rows = n - 3
    assert rows > 8 * TILE and (rows + TILE - 1) // TILE == 16
    r = np.arange(n)
    for name, values in (("runs", r // 1000), ("mod7", r % 7), ("reversed_runs", (n - 1 - r) // 1000), ("random", np.random.default_rng(14).integers(0, P, n))):
        prog, w = sref.sort_program((13,), 1, rows)
        data = np.zeros((w, n), np.uint32)
        data[0], data[1] = sref.encode_words(values), sref.encode_words(r)
        data[2:] = POISON
        got = _check(hal, prog, po2, w, _code(po2), data, name)
        if name in ("runs", "mod7", "reversed_runs"):
            from_row = np.array(sref.decode_ints(got[3, :rows]))
            keys = np.asarray(values)[from_row] & 8191
            assert np.all(np.diff(keys) >= 0) and np.all((np.diff(from_row) > 0) | (np.diff(keys) > 0)), f"{name}: not stable"


def test_a_second_run_at_the_same_shape_allocates_nothing(hal):
    """a ctx exposes no counter for the program's own (unpooled) buffers: the device's free memory is what is compared"""
    import torch

    prog, w = sref.sort_program((24, 20), 1)
    compiled = sref.compile_ref(prog)
    loaded = compiled.load(hal)
    try:
        bufs = {}
        for po2 in (12, 18):
            n = 1 << po2
            data = sref.random_columns((w, n), seed=po2)
            bufs[po2] = (hal.copy_from(_code(po2).reshape(-1)), hal.copy_from(data.reshape(-1)), data)
        hal.sync()
        free0 = torch.cuda.mem_get_info(0)[0]
        free = []
        for po2 in (12, 12, 18, 18, 12):
            dcode, ddata, _ = bufs[po2]
            loaded.run(po2, dcode, W_CODE, ddata, w)
            hal.sync()
            free.append(torch.cuda.mem_get_info(0)[0])
        assert free[1] == free[0] <= free0, "a second run at po2 12 allocated"
        assert free[2] < free[1] - (4 << 20), "the work space of 2^18 rows (6 MiB of pairs) was not allocated when it was needed"
        assert free[4] == free[3] == free[2], "a run that fits the work space allocated"
        # the work space of 2^18 rows served 2^12 rows: the same words as ever (a dest is no source, so a repeated run repeats them)
        assert np.array_equal(bufs[12][1].view().reshape(w, -1), sref.evaluate(prog, 12, _code(12), bufs[12][2]))
        for dcode, ddata, _ in bufs.values():
            dcode.free()
            ddata.free()
    finally:
        loaded.unload()
        compiled.close()


def test_the_profile_names_the_pack_the_passes_and_the_gather(hal):
    prog = sref.two_sorts_program()
    compiled = sref.compile_ref(prog)
    loaded = compiled.load(hal)
    try:
        po2 = 8
        code, data = _code(po2), sref.random_columns((8, 1 << po2), seed=5)
        dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        hal.profile_reset()
        hal.profile_enable(True)
        loaded.run(po2, dcode, W_CODE, ddata, 8)
        hal.sync()
        hal.profile_enable(False)
        report = hal.profile_report()
        for op, calls in (("wit_program_run", 1), ("wit_program_sort_pack", 2), ("wit_program_sort", 2), ("wit_program_sort_gather", 2)):
            assert report[op]["calls"] == calls, (op, report.get(op), sorted(report))
        assert "wit_program_count" not in report
        assert np.array_equal(ddata.view().reshape(8, -1), sref.evaluate(prog, po2, code, data))
        dcode.free()
        ddata.free()
    finally:
        hal.profile_enable(False)
        loaded.unload()
        compiled.close()


def test_a_fixtures_generated_kernel_serves_the_program_under_a_sort_list(hal):
    """the steps of tests/golden/witgen/every_form.json plus a sort list: the same digest, so the code object built from the fixture
    attaches; the sorts run after it exactly as after the interpreter"""
    import witgen_cases
    from boundless_amd.consgen import witness_program_of

    desc = witgen_cases.description("every_form")  # SETs 3, 5, 6, 7, 2; reads 0, 1; the fixture's data group has 8 columns
    desc["sorts"] = [{"keys": [[7, 13]], "payload": [0, 3], "dests": [8, 9, 4], "rows": 253}]
    compiled = witness_program_of(desc)
    plain = witgen_cases.compiled("every_form")
    assert compiled.digest() == plain.digest() == witgen_cases.meta("every_form")["digest"]
    prog = sref.Program()
    base = witgen_cases.ref_program(desc)
    prog.steps, prog.taps, prog.cells, prog.n_fp = base.steps, base.taps, base.cells, base.n_fp
    prog.sort([(7, 13)], [0, 3], [8, 9, 4], 253)
    loaded = compiled.load(hal)
    try:
        po2 = 8
        code, data = _code(po2, seed=3), sref.random_columns((10, 1 << po2), seed=4)
        data[prog.written()] = POISON
        interpreted = _check(hal, prog, po2, 10, code, data, "interpreter + sorts", loaded, compiled)
        loaded.attach_kernel(witgen_cases.kernel_path("every_form"))
        assert loaded.kernel_attached
        hal.profile_reset()
        hal.profile_enable(True)
        generated = _check(hal, prog, po2, 10, code, data, "generated kernel + sorts", loaded, compiled)
        hal.sync()
        hal.profile_enable(False)
        report = hal.profile_report()
        assert report["wit_program_run_gen"]["calls"] == 1 and report["wit_program_sort"]["calls"] == 1 and "wit_program_run" not in report
        assert np.array_equal(interpreted, generated) and not np.any(generated[[8, 9, 4], :253] == POISON)
    finally:
        hal.profile_enable(False)
        loaded.unload()
        compiled.close()
        plain.close()


# ---- the device entry point's refusals ----
def _one(keys, payload, dests, rows=0):
    p = sref.Program()
    p.sort(keys, payload, dests, rows)
    return p


def test_run_refuses_what_does_not_fit_the_shape_by_message_and_touches_nothing(hal):
    po2 = 6
    n = 1 << po2
    good = sref.set_key_program()
    code, data = _code(po2), sref.random_columns((8, n), seed=9)
    data[good.written()] = POISON
    dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
    cases = ((_one([(0, 8)], [], [5], rows=n + 1), 8, "bx_wit_program_run: sort 0: rows 65 is above the trace's 64 rows"),
             (_one([(0, 8)], [7], [5, 6]), 7, "bx_wit_program_run: sort 0: source 1 is data column 7, the data group has 7 columns"),
             (_one([(0, 8)], [1], [5, 7]), 7, "bx_wit_program_run: sort 0: dest 1 is data column 7, the data group has 7 columns"),
             (sref.two_sorts_program(rows_b=2 * n), 8, "bx_wit_program_run: sort 1: rows 128 is above the trace's 64 rows"))
    for prog, w_data, match in cases:
        compiled = sref.compile_ref(prog)
        loaded = compiled.load(hal)
        try:
            with pytest.raises(HalError, match=match):
                loaded.run(po2, dcode, W_CODE, ddata.slice(0, w_data * n), w_data)
            # the checks that were there come first, with their messages
            with pytest.raises(HalError, match=r"bx_wit_program_run: buffer size mismatch \(groups N x width\)"):
                loaded.run(po2, dcode, W_CODE, ddata.slice(0, w_data * n - 1), w_data)
            with pytest.raises(HalError, match="bx_wit_program_run: code and data overlap"):
                loaded.run(po2, ddata.slice(0, W_CODE * n), W_CODE, ddata.slice(0, w_data * n), w_data)
        finally:
            loaded.unload()
            compiled.close()
    assert np.array_equal(ddata.view(), data.reshape(-1)) and np.array_equal(dcode.view(), code.reshape(-1)), "a refused call wrote"
    dcode.free()
    ddata.free()
    _check(hal, good, po2, 8, code, data, "after the refusals")  # the ctx is still good


# ---- what a ctx holds ----
def test_unload_returns_the_work_space_and_bx_free_releases_what_is_left():
    import torch

    po2 = 20
    n = 1 << po2
    prog, w = sref.sort_program((8,), 0)  # 24 MiB of pairs at 2^20 rows
    compiled = sref.compile_ref(prog)
    HipHal(0).close()  # the first ctx of a process loads the code objects: not part of what is measured
    h = HipHal(0)
    try:
        dcode, ddata = h.copy_from(np.zeros(W_CODE * n, np.uint32)), h.copy_from(sref.random_columns((w * n,), seed=1))
        compiled.load(h).unload()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        held = compiled.load(h)
        held.run(po2, dcode, W_CODE, ddata, w)
        h.sync()
        assert torch.cuda.mem_get_info(0)[0] <= free_before - (24 << 20), "the work space was not allocated by the run that needed it"
        held.unload()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before
        kept = [compiled.load(h) for _ in range(2)]  # still loaded, with their work space, when the ctx goes
        for k in kept:
            k.run(po2, dcode, W_CODE, ddata, w)
        h.sync()
        got = ddata.view().reshape(w, n)
        assert np.all(np.diff((cref.decode_words(got[1]) & np.uint64(255)).astype(np.int64)) >= 0)
        dcode.free()
        ddata.free()
    finally:
        h.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before
    for k in kept:
        dev, k.dev = k.dev, None  # released by bx_free: an unload of the freed handle is answered by message
        assert b"not a loaded program" in compiled.lib.bx_wit_program_unload(dev)


# ---- through a proof: a sorted range check with no built-in circuit behind it ----
def _range_circuit(lib, numpy, cheat, po2):
    import acc_ratio_ref
    from test_acc_ratio_gpu import FILL, MultisetRatioCircuit

    class SortedRangeCircuit(MultisetRatioCircuit):
        """numpy: the all-numpy twin fills every column itself.  Otherwise the base places a, the tags, the tail rows and the code group
        only: the sorted rows of b and q hold poison until the witness program has run, the accum group FILL until the accumulate
        program has"""

        def __init__(self):
            self.lib, self.numpy, self.cheat, self.calls = lib, numpy, cheat, []
            self.cons, self.acc, self.wit = sref.range_programs(po2)

        def normalize(self, shape):
            shape.cons_terms, shape.cons_degree = 5, 3

        def taps(self, shape, group, col):
            return [0, 1] if (group == 2 and col < 4) or (group == 1 and col == 2) else [0]

        def _code(self):
            return sref.range_code(self.po2)

        def witgen(self, ctx, code, data, segment, segment_dev):
            self.calls.append("witgen")
            free = sref.range_free_columns(self.po2, int.from_bytes(segment[20:28], "little") & 0xFFFFFFFF, self.cheat)
            self.data = sref.evaluate(self.wit, self.po2, self._code(), free)
            self._put(ctx, data, self.data if self.numpy else free)
            return []

        def accumulate(self, ctx, accum, mix):
            self.calls.append("accumulate")
            if self.numpy:
                self._put(ctx, accum, acc_ratio_ref.evaluate(self.acc, self.po2, self._code(), self.data, [], mix))
            else:
                self._put(ctx, accum, np.full(self.wa * self.n, FILL, np.uint32))

    return SortedRangeCircuit()


def _prove_range(numpy, cheat=False, wit=None, po2=9, seed=2024):
    from acc_ratio_cases import compile_ref as compile_acc
    from cons_program_cases import compile_ref as compile_cons
    from boundless_amd.hal import load_library

    circ = _range_circuit(load_library(), numpy, cheat, po2)
    circ.bind(po2, sref.RC_WIDTHS)
    ops = CircuitOps.from_object(circ, b"sorted-range-check")
    if not numpy:
        ops = CircuitOps.from_program(compile_cons(circ.cons), ops, witness=sref.compile_ref(circ.wit if wit is None else wit), accumulate=compile_acc(circ.acc))
    srv = HipProverServer(0, po2=po2, widths=sref.RC_WIDTHS, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_a_range_check_whose_sorted_columns_are_a_sort_proves_its_numpy_twins_seal():
    want, numpy_ops, numpy_ctx, twin = _prove_range(numpy=True)
    assert twin.calls == ["code_group", "witgen", "accumulate", "eval_check"]
    verify_seal(want.seal, circuit=numpy_ops, ctx=numpy_ctx)
    b = cref.decode_words(twin.data[2]).astype(np.int64)
    assert b[0] == 0 and b[-1] == sref.RC_B - 1 and set(np.diff(b).tolist()) == {0, 1}  # the twin's own column is a real sorted copy
    got, ops, vctx, circ = _prove_range(numpy=False)
    assert circ.calls == ["code_group", "witgen", "accumulate"]  # eval_check did not come from numpy
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # one a at B + 1: (b, q) is still a permutation of (a, p), z still closes, b does not end at B - 1
    receipt, ops, vctx, _ = _prove_range(numpy=False, cheat=True)
    with pytest.raises(HalError, match="constraint identity"):
        verify_seal(receipt.seal, circuit=ops, ctx=vctx)


def test_the_composite_table_checks_the_sorts_against_the_shape():
    for kw, match in ((dict(rows=1024), "cons circuit: witness program: sort 0: rows 1024 is above the trace's 512 rows"),
                      (dict(dests=(2, 4)), "cons circuit: witness program: sort 0: dest 1 is data column 4, the data group has 4 columns")):
        with pytest.raises(HalError, match=match):
            _prove_range(numpy=False, wit=sref.range_programs(9, **kw)[2])
