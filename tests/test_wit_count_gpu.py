"""GPU: a witness program's multiplicity columns (include/bx_program.h "multiplicity columns", csrc/wit_count.hip) — the device
histogram against the definition-level reference of tests/wit_count_ref.py and against the host executor, word for word over the whole
data group with the count columns poisoned first; both forms of the histogram at their boundary and with several workgroups flushing
into the same bins; a generated per-row kernel followed by the counts; the entry point's refusals; the built-in lookup circuit with
its multiplicity column from a count, seal for seal; a range-check circuit with no built-in table behind it against its all-numpy
twin; and what a ctx holds.

Sizes are the smallest at which each thing can break: po2 1 (two rows), 6 and 7 (less than one tile: lanes hold no value), 8 (one tile
of the global form), 9 (the prover's smallest), 12 (four tiles of the LDS form per column), 16 for the two bin counts on either side of
the 128 KiB of LDS; bins of 1, 2, 3 (every lane a peer of few leaders), 255, 256, 257 (around a workgroup's width) and `rows`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import wit_count_ref as cref  # noqa: E402

from boundless_amd.circuit import CircuitOps, encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P, POISON = cref.P, cref.POISON
W_CODE = cref.WIDTHS[0]


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def _columns(prog, po2, w_data, kind, bins, seed=0):
    """(code, data): `kind` of wit_count_ref.source_columns or a pattern of tests/extreme_words.py; every column the run writes poisoned"""
    n = 1 << po2
    code = cref.source_columns("random", (W_CODE, n), P, seed=seed + 1)
    if kind in extreme_words.EXTREME:
        data = extreme_words.pattern(kind, (w_data, n), seed=seed)
    else:
        data = cref.source_columns(kind, (w_data, n), bins, seed=seed)
    data[prog.written()] = POISON
    return code, data


def _check(hal, prog, po2, w_data, code, data, what, loaded=None, compiled=None):
    """the device, the host executor and the reference agree on every word of `data`; free columns and the rows at or above a count's
    `rows` are left alone; a count column sums to the number of in-range cells -> the data group after the run"""
    n = 1 << po2
    own = compiled is None
    if own:
        compiled = cref.compile_ref(prog)
        loaded = compiled.load(hal)
    try:
        want = cref.evaluate(prog, po2, code, data)
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
    assert np.array_equal(got[free], data[free]), f"{what}: a free column was written"
    for k, (col, _sources, _bins, rows) in enumerate(prog.counts):
        rows = rows or n
        assert np.all(got[col, rows:] == POISON), f"{what}: a row at or above rows = {rows} of count column {col} was written"
        assert int(cref.decode_words(got[col, :rows]).sum()) == cref.in_range_cells(prog, k, po2, got), f"{what}: the multiplicities do not sum to the in-range cells"
    return got


def _shapes(n):
    """every valid (bins, rows) of bins in {1, 2, 3, 255, 256, 257, rows} x rows in {0, 1, N - 3, N}"""
    out = []
    for rows in (0, 1, n - 3, n):
        if rows < 0:  # po2 1
            continue
        eff = rows or n
        for bins in (1, 2, 3, 255, 256, 257, eff):
            if 1 <= bins <= eff and (bins, rows) not in out:
                out.append((bins, rows))
    return out


@pytest.mark.parametrize("po2", [1, 6, 7, 8, 9, 12])
def test_run_is_the_reference_and_the_host_executor_for_every_bins_and_rows(hal, po2):
    n = 1 << po2
    shapes = _shapes(n)
    assert any(b == (r or n) for b, r in shapes) and any(r == 0 for _, r in shapes)
    for bins, rows in shapes:
        prog = cref.counts_only_program(bins, rows, sources=(0, 1, 4))
        compiled = cref.compile_ref(prog)
        loaded = compiled.load(hal)
        try:
            for kind in ("same", "mod", "random", "above"):
                code, data = _columns(prog, po2, 8, kind, bins, seed=po2)
                got = _check(hal, prog, po2, 8, code, data, f"po2 {po2}, bins {bins}, rows {rows}, {kind}", loaded, compiled)
                eff = rows or n
                if kind == "same":  # every lane of every wave a peer of its leader
                    assert int(cref.decode_words(got[6, bins - 1])) == 3 * eff
                if kind == "above":
                    assert not got[6, :eff].any()
                if kind == "random":
                    assert got[6, :eff].any(), "degenerate case: nothing was counted"
                if kind == "mod" and bins == eff:
                    assert np.all(cref.decode_words(got[6, :eff]) == 3)
        finally:
            loaded.unload()
            compiled.close()


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_run_is_the_reference_on_extreme_columns(hal, pattern):
    po2 = 7
    for bins in (2, 128):  # MONT_ONE decodes to 1, P - MONT_ONE to P - 1, P - 1 to a large value
        prog = cref.two_counts_program(bins, min(bins, 100), rows_a=0, rows_b=125)
        code, data = _columns(prog, po2, 8, "same" if pattern == "zero" else pattern, 1)  # "same" with bins 1: every cell 0
        _check(hal, prog, po2, 8, code, data, f"{pattern}, bins {bins}")


@pytest.mark.parametrize("po2", [6, 9])
def test_a_set_column_as_a_source_one_source_sixty_four_sources_and_two_counts(hal, po2):
    n = 1 << po2
    for name, prog, w_data in (("set_source", cref.set_source_program(5, rows=n - 3), 8),
                               ("one_source", cref.counts_only_program(n, sources=(2,)), 8),
                               ("sources_64", cref.wide_program(64, 257 if po2 == 9 else 9), 65),
                               ("two_counts", cref.two_counts_program(3, 40, rows_a=n - 1, rows_b=0), 8)):
        bins = max(c[2] for c in prog.counts)
        code, data = _columns(prog, po2, w_data, "random", bins, seed=7)
        got = _check(hal, prog, po2, w_data, code, data, f"{name} at po2 {po2}")
        assert got[prog.count_cols()].any(), "degenerate case: nothing was counted"
        if name == "set_source":
            assert not np.any(got[[3, 5]] == POISON)


@pytest.mark.parametrize("bins,po2,lds", [(32768, 16, 1), (32769, 16, 1), (256, 12, 1), (256, 12, 0), (256, 16, 1), (256, 16, 0), (32768, 16, 0)])
def test_both_forms_at_their_boundary_and_with_several_workgroups_on_the_same_bins(bins, po2, lds):
    """32 768 bins are the largest LDS form, 32 769 the global form whatever the tunable says; 256 bins at po2 12 and 16 are 32 and 512
    tiles of the LDS form over 8 sources: several workgroups flush into the same bins, under either setting of lookup_hist_lds"""
    h = HipHal(0)
    try:
        h.set_tunable("lookup_hist_lds", lds)
        prog = cref.wide_program(8, bins, rows=(1 << po2) - 3)
        for kind in ("random", "same"):
            code, data = _columns(prog, po2, 9, kind, bins, seed=bins)
            _check(h, prog, po2, 9, code, data, f"bins {bins} at po2 {po2}, lookup_hist_lds {lds}, {kind}")
    finally:
        h.close()


def test_the_profile_names_the_histogram_and_the_store(hal):
    prog = cref.two_counts_program(3, 40)
    compiled = cref.compile_ref(prog)
    loaded = compiled.load(hal)
    try:
        code, data = _columns(prog, 8, 8, "random", 40)
        dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        hal.profile_reset()
        hal.profile_enable(True)
        loaded.run(8, dcode, W_CODE, ddata, 8)
        hal.sync()
        hal.profile_enable(False)
        report = hal.profile_report()
        for op, calls in (("wit_program_run", 1), ("wit_program_count", 2), ("wit_program_count_store", 2)):
            assert report[op]["calls"] == calls, (op, report.get(op), sorted(report))
        assert np.array_equal(ddata.view().reshape(8, -1), cref.evaluate(prog, 8, code, data))
    finally:
        hal.profile_enable(False)
        loaded.unload()
        compiled.close()


def test_a_fixtures_generated_kernel_serves_the_program_under_a_count_list(hal):
    """the steps of tests/golden/witgen/every_form.json plus a count list: the same digest, so the code object built from the fixture
    attaches; the counts run after it exactly as after the interpreter"""
    import witgen_cases
    from boundless_amd.consgen import witness_program_of

    desc = witgen_cases.description("every_form")  # SETs 3, 5, 6, 7, 2; reads 0, 1; column 4 is free and never read
    desc["counts"] = [{"col": 4, "sources": [7, 0, 3], "bins": 100, "rows": 253}]
    compiled = witness_program_of(desc)
    plain = witgen_cases.compiled("every_form")
    assert compiled.digest() == plain.digest() == witgen_cases.meta("every_form")["digest"]
    prog = cref.Program()
    base = witgen_cases.ref_program(desc)
    prog.steps, prog.taps, prog.cells, prog.n_fp = base.steps, base.taps, base.cells, base.n_fp
    prog.count(4, [7, 0, 3], 100, 253)
    loaded = compiled.load(hal)
    try:
        po2 = 8
        code, data = _columns(prog, po2, 8, "random", 100, seed=3)
        data[[0, 1]] = cref.source_columns("random", (2, 1 << po2), 100, seed=4)
        interpreted = _check(hal, prog, po2, 8, code, data, "interpreter + counts", loaded, compiled)
        loaded.attach_kernel(witgen_cases.kernel_path("every_form"))
        assert loaded.kernel_attached
        hal.profile_reset()
        hal.profile_enable(True)
        generated = _check(hal, prog, po2, 8, code, data, "generated kernel + counts", loaded, compiled)
        hal.sync()
        hal.profile_enable(False)
        report = hal.profile_report()
        assert report["wit_program_run_gen"]["calls"] == 1 and report["wit_program_count"]["calls"] == 1 and "wit_program_run" not in report
        assert np.array_equal(interpreted, generated) and generated[4, :253].any()
    finally:
        hal.profile_enable(False)
        loaded.unload()
        compiled.close()
        plain.close()


# ---- the device entry point's refusals ----
def test_run_refuses_what_does_not_fit_the_shape_by_message_and_touches_nothing(hal):
    po2 = 6
    n = 1 << po2
    good = cref.set_source_program(5)
    code, data = _columns(good, po2, 8, "random", 5, seed=9)
    dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
    cases = ((cref.counts_only_program(2, rows=n + 1), 8, "bx_wit_program_run: count 0: rows 65 is above the trace's 64 rows"),
             (cref.counts_only_program(n + 1), 8, r"bx_wit_program_run: count 0: bins 65 is above the trace's 64 rows \(rows == 0 counts all of them\)"),
             (cref.counts_only_program(2, col=7), 7, "bx_wit_program_run: count 0 fills data column 7, the data group has 7 columns"),
             (cref.counts_only_program(2, sources=(1, 7)), 7, "bx_wit_program_run: count 0: source 1 is data column 7, the data group has 7 columns"),
             (cref.two_counts_program(2, 2, rows_b=2 * n), 8, "bx_wit_program_run: count 1: rows 128 is above the trace's 64 rows"))
    for prog, w_data, match in cases:
        compiled = cref.compile_ref(prog)
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


# ---- through a proof: the built-in lookup circuit, its multiplicity column from a count ----
@pytest.mark.parametrize("po2", [9, 12])
def test_the_lookup_circuit_with_its_multiplicities_from_a_count_proves_the_built_in_circuits_seal(po2):
    import cons_program_ref
    import lookup_ref
    from cons_program_cases import compile_ref as compile_cons

    widths, V = (3, 10, 20), 2
    sh = lookup_ref.Shape(po2, *widths)
    assert sh.V == V
    wit = cref.compile_ref(cref.lookup_count(V, sh.B, sh.A))
    assert wit.counts() == [{"col": 6, "bins": sh.B, "rows": sh.A, "sources": [1, 2, 4, 5]}]
    hal = HipHal(0)
    ops = CircuitOps.from_program(compile_cons(cons_program_ref.lookup_program(po2, widths)), lookup_circuit(), witness=wit)
    builtin, composite = HipProverServer(0, po2=po2, widths=widths, circuit="lookup"), HipProverServer(0, po2=po2, widths=widths, circuit=ops, hal=hal)
    try:
        planted = [(1, 5, sh.B + 3), (5, 7, sh.B), (2, 5, P - 1), (4, 0, 0)]  # limbs at and above B: not counted by either
        hal.profile_reset()
        hal.profile_enable(True)
        for seg in (Segment(index=0, po2=po2, seed=700 + po2), Segment(index=1, po2=po2, seed=800 + po2, payload=encode_cell_records(planted))):
            a, b = builtin.prove_segment(seg), composite.prove_segment(seg)
            assert np.array_equal(a.seal, b.seal), f"first differing seal word: {int(np.argmax(a.seal != b.seal))}"
            if seg.index == 0:  # the planted limbs are not in the table: that seal is the same and is refused by both
                verify_seal(b.seal, circuit=ops)
                verify_seal(b.seal, circuit="lookup")
        hal.profile_enable(False)
        report = hal.profile_report()
        for op in ("wit_program_count", "wit_program_count_store", "lookup_hist", "lookup_mult"):  # the base still fills the column first
            assert report[op]["calls"] == 2, (op, report.get(op), sorted(report))
    finally:
        builtin.close()
        composite.close()
        hal.close()


# ---- through a proof: a range check with no built-in table behind it ----
RC_B, RC_WIDTHS = 256, (3, 4, 12)


def _range_programs(rows=0, sources=(1, 2)):
    """v = lo + B hi with lo, hi < B looked up in the table t(r) = r.  code: first, last, t.  data: v (SET), lo, hi (free), m (count).
    accum: the LogUp sums of 1 / (alpha - lo), 1 / (alpha - hi) and m / (alpha - t); they close on the last row iff every limb is in the
    table with the multiplicity m says"""
    import acc_program_ref
    import cons_program_ref

    p = cons_program_ref.Program(1)  # one public word, m(0): a global cell of the count column (no constraint names it)
    xk = [None] + [p.const_ext(*[1 if i == k else 0 for i in range(4)]) for k in (1, 2, 3)]

    def ext_of(words):
        r = words[0]
        for k in (1, 2, 3):
            r = p.add(r, p.mul(xk[k], words[k]))
        return r

    alpha = ext_of([p.mix(k) for k in range(4)])
    first, last, t = p.get(0, 0), p.get(0, 1), p.get(0, 2)
    not_first = p.sub(p.const(1), first)
    v, lo, hi, m = (p.get(1, c) for c in range(4))
    cur = [ext_of([p.get(2, 4 * s + k, 0) for k in range(4)]) for s in range(3)]
    back = [ext_of([p.get(2, 4 * s + k, 1) for k in range(4)]) for s in range(3)]
    top = p.and_eqz(p.true(), p.sub(p.sub(v, lo), p.mul(p.const(RC_B), hi)))
    for s, (x, mult) in enumerate(((lo, p.const(1)), (hi, p.const(1)), (t, m))):  # (S(r) - (1 - first) S(r-1)) (alpha - x) - mult
        top = p.and_eqz(top, p.sub(p.mul(p.sub(cur[s], p.mul(not_first, back[s])), p.sub(alpha, x)), mult))
    top = p.and_eqz(top, p.mul(last, p.sub(p.add(cur[0], cur[1]), cur[2])))
    cons = p.done(top)

    a = acc_program_ref.Program(1)
    al, one = a.alpha(), a.const(1)
    a.sum_(0, one, a.sub(al, a.get(1, 1)))
    a.sum_(1, one, a.sub(al, a.get(1, 2)))
    a.sum_(2, a.get(1, 3), a.sub(al, a.get(0, 2)))  # taps the count column: keep runs after the counts

    w = cref.Program()
    w.set(0, w.add(w.get(1, 1), w.mul(w.const(RC_B), w.get(1, 2))))
    w.count(3, sources, RC_B, rows)
    w.global_cell(0, 3, 0)  # read after the counts: before them the cell holds the base's poison
    return cons, a, w


def _range_circuit(lib, numpy, cheat):
    import acc_program_ref
    from test_acc_program_gpu import FILL, MultisetCircuit

    class RangeCircuit(MultisetCircuit):
        """numpy: the all-numpy twin fills every column itself.  Otherwise the base places the free limbs and the code group only:
        v and m hold poison until the witness program has run, the accum group FILL until the accumulate program has"""

        def __init__(self):
            self.lib, self.numpy, self.cheat, self.calls = lib, numpy, cheat, []
            self.cons, self.acc, self.wit = _range_programs()

        def normalize(self, shape):
            shape.cons_terms, shape.cons_degree = 5, 3

        def n_globals(self, shape):
            return 1

        def taps(self, shape, group, col):
            return [0, 1] if group == 2 and col < 12 else [0]

        def _code(self):
            code = np.zeros((self.wc, self.n), np.uint32)
            code[0][0] = code[1][self.n - 1] = cref.encode(1)
            code[2] = cref.encode_words(np.arange(self.n))
            return code

        def witgen(self, ctx, code, data, segment, segment_dev):
            self.calls.append("witgen")
            rng = np.random.default_rng(int.from_bytes(segment[20:28], "little") & 0xFFFFFFFF)
            limbs = rng.integers(0, RC_B, (2, self.n)).astype(np.uint64)
            limbs[1] &= np.uint64(RC_B // 2 - 1) * (np.arange(self.n, dtype=np.uint64) % 2)  # half of the hi limbs are 0: one hot bin
            if self.cheat:
                limbs[0][5] = RC_B + 1  # v follows it, every local constraint holds, the table does not have it
            free = np.full((self.wd, self.n), POISON, np.uint32)
            free[1:3] = cref.encode_words(limbs)
            self.data = cref.evaluate(self.wit, self.po2, self._code(), free)
            self._put(ctx, data, self.data if self.numpy else free)
            return [int(self.data[3][0])] if self.numpy else [12345]  # the base's word is not the trace's: the global cell overrides it

        def accumulate(self, ctx, accum, mix):
            self.calls.append("accumulate")
            if self.numpy:
                self._put(ctx, accum, acc_program_ref.evaluate(self.acc, self.po2, self._code(), self.data, [], mix))
            else:
                self._put(ctx, accum, np.full(self.wa * self.n, FILL, np.uint32))

    return RangeCircuit()


def _prove_range(numpy, cheat=False, wit=None, po2=9, seed=2024):
    from acc_program_cases import compile_ref as compile_acc
    from cons_program_cases import compile_ref as compile_cons
    from boundless_amd.hal import load_library

    circ = _range_circuit(load_library(), numpy, cheat)
    circ.bind(po2, RC_WIDTHS)
    ops = CircuitOps.from_object(circ, b"range-check")
    if not numpy:
        ops = CircuitOps.from_program(compile_cons(circ.cons), ops, witness=cref.compile_ref(circ.wit if wit is None else wit), accumulate=compile_acc(circ.acc))
    srv = HipProverServer(0, po2=po2, widths=RC_WIDTHS, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_a_range_check_whose_multiplicities_are_a_count_proves_its_numpy_twins_seal():
    want, numpy_ops, numpy_ctx, twin = _prove_range(numpy=True)
    assert twin.calls == ["code_group", "witgen", "accumulate", "eval_check"]
    verify_seal(want.seal, circuit=numpy_ops, ctx=numpy_ctx)
    m = cref.decode_words(twin.data[3])
    assert int(m.sum()) == 2 * twin.n and int(m[0]) > twin.n // 2 and not m[RC_B:].any()  # the twin's own column is a real histogram
    got, ops, vctx, circ = _prove_range(numpy=False)
    assert circ.calls == ["code_group", "witgen", "accumulate"]  # eval_check did not come from numpy
    # the public word is m(0) as the count left it: the cell was read after the counts (before them it is POISON, the base's word 12345)
    assert int(got.public_words(1)[0]) == int(twin.data[3][0]) == cref.encode(int(m[0])) and int(m[0]) > 0
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # one limb at B + 1: v = lo + B hi still holds on every row, the limb is not counted, the sums do not close
    receipt, ops, vctx, _ = _prove_range(numpy=False, cheat=True)
    with pytest.raises(HalError, match="constraint identity"):
        verify_seal(receipt.seal, circuit=ops, ctx=vctx)


def test_the_composite_table_checks_the_counts_against_the_shape():
    for kw, match in ((dict(rows=1024), "cons circuit: witness program: count 0: rows 1024 is above the trace's 512 rows"),
                      (dict(sources=(1, 4)), "cons circuit: witness program: count 0: source 1 is data column 4, the data group has 4 columns")):
        with pytest.raises(HalError, match=match):
            _prove_range(numpy=False, wit=_range_programs(**kw)[2])


# ---- what a ctx holds ----
def test_load_and_unload_return_the_counters_and_bx_free_releases_what_is_left():
    import torch

    compiled = cref.compile_ref(cref.two_counts_program(1 << 20, 1 << 22, rows_a=1 << 20, rows_b=1 << 22))  # 20 MiB of counters
    HipHal(0).close()  # the first ctx of a process loads the code objects: not part of what is measured
    h = HipHal(0)
    try:
        compiled.load(h).unload()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        held = compiled.load(h)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] <= free_before - (20 << 20), "the counters were not allocated at load"
        held.unload()
        for _ in range(5):
            compiled.load(h).unload()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before
        kept = [compiled.load(h) for _ in range(2)]  # still loaded when the ctx goes
    finally:
        h.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before
    for k in kept:
        dev, k.dev = k.dev, None  # released by bx_free: an unload of the freed handle is answered by message
        assert b"not a loaded program" in compiled.lib.bx_wit_program_unload(dev)
