"""GPU: accumulate programs (include/bx_program.h "Accumulate programs", csrc/acc_program.hip) — keep + run against the
definition-level reference of tests/acc_program_ref.py and against the host executor, word for word over accum columns [0, 4 S), with
the columns above still poisoned; the reason `kept` exists; the lookup circuit's accumulate stage written as a program against
tests/lookup_ref.py; the entry points' refusals; a two-column multiset circuit whose accumulate is the program alone, against its
all-numpy twin, seal for seal; the built-in lookup circuit with both its constraints and its accumulate from programs; and what a
ctx holds.

Sizes are the smallest at which each thing can break: po2 1 (two rows: a tap 3 rows back wraps), 6 and 7 (less than one workgroup:
lanes return early), 8 (one workgroup exactly), 9 (two workgroups, and the prover's smallest), 12 (two scan tiles of 2048 elements)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_ref as ref  # noqa: E402
import extreme_words  # noqa: E402
import lookup_ref  # noqa: E402
from acc_program_cases import POISON, compile_ref, inputs, w_accum  # noqa: E402

from boundless_amd.circuit import CircuitOps, encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
WIDTHS = ref.WIDTHS


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def programs(hal):
    """name -> (reference program, the library's compiled program, the same loaded on the module's ctx): built once"""
    out = {}
    for name, make in ref.PROGRAMS.items():
        prog = make()
        compiled = compile_ref(prog)
        out[name] = (prog, compiled, compiled.load(hal))
    yield out
    for _, compiled, loaded in out.values():
        loaded.unload()
        compiled.close()


class Stage:
    """the device buffers of one keep + run, the work space and the accum group poisoned"""

    def __init__(self, hal, compiled, po2, code, data, wa, widths=WIDTHS):
        info = compiled.info()
        n = 1 << po2
        self.hal, self.po2, self.n, self.wa, self.widths, self.info = hal, po2, n, wa, widths, info
        self.code, self.data = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        # a slice does not own its memory: the whole buffers stay referenced here
        self._kept = hal.copy_from(np.full(max(n * info["kept"], 1), POISON, np.uint32))
        self._mults = hal.copy_from(np.full(max(n * info["sums"], 1), POISON, np.uint32))
        self.kept, self.mults = self._kept.slice(0, n * info["kept"]), self._mults.slice(0, n * info["sums"])
        self.run_ext = hal.copy_from(np.full(4 * n * info["sequences"], POISON, np.uint32))
        self.accum = hal.copy_from(np.full(wa * n, POISON, np.uint32))

    def keep(self, loaded):
        loaded.keep(self.po2, self.code, self.widths[0], self.data, self.widths[1], self.kept)

    def run(self, loaded, g, mix):
        loaded.run(self.po2, self.kept, g, mix, self.run_ext, self.mults, self.accum, self.wa)
        return self.accum.view().reshape(self.wa, self.n)


def _check_stage(hal, prog, compiled, loaded, po2, pattern, seed, what):
    code, data, g, mix = inputs(prog, po2, pattern=pattern, seed=seed)
    wa, S = w_accum(prog), len(prog.sequences())
    want = ref.evaluate(prog, po2, code, data, g, mix)
    host = np.full((wa, 1 << po2), POISON, np.uint32)
    compiled.run_host(po2, code, WIDTHS[0], data, WIDTHS[1], g, mix, host, wa)
    st = Stage(hal, compiled, po2, code, data, wa)
    st.keep(loaded)
    got = st.run(loaded, g, mix)
    bad = np.argwhere(got[:4 * S] != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} accum words differ from the reference, first at (column, row) {tuple(bad[0])}: {compiled.info()}"
    assert np.array_equal(host[:4 * S], want), f"{what}: the host executor differs from the reference"
    assert np.all(got[4 * S:] == POISON), f"{what}: an accum column at or above 4 S was written"
    assert np.array_equal(st.code.view(), code.reshape(-1)) and np.array_equal(st.data.view(), data.reshape(-1)), f"{what}: code or data was written"
    return want


@pytest.mark.parametrize("po2", [1, 6, 7, 8, 9, 12])
@pytest.mark.parametrize("name", list(ref.PROGRAMS))
def test_keep_and_run_are_the_reference_and_the_host_executor_on_every_word(hal, programs, name, po2):
    prog, compiled, loaded = programs[name]
    want = _check_stage(hal, prog, compiled, loaded, po2, "random", len(prog.steps), f"{name} at po2 {po2}")
    if po2 >= 6:
        assert len(np.unique(want[0])) > (1 << po2) // 2, "degenerate reference: a stage that writes a constant could pass"


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_keep_and_run_are_the_reference_on_extreme_columns(hal, programs, pattern):
    for name, (prog, compiled, loaded) in programs.items():
        _check_stage(hal, prog, compiled, loaded, 7, pattern, 0, f"{name} on {pattern}")


def test_overwriting_code_and_data_between_keep_and_run_changes_nothing(hal, programs):
    """the prover interpolates both groups in place right after witgen: this is why `kept` exists"""
    prog, compiled, loaded = programs["every_form"]
    po2 = 9
    code, data, g, mix = inputs(prog, po2, seed=11)
    want = ref.evaluate(prog, po2, code, data, g, mix)
    st = Stage(hal, compiled, po2, code, data, w_accum(prog))
    st.keep(loaded)
    st.code.copy_from(np.full(code.size, 1234567, np.uint32))
    st.data.copy_from(np.full(data.size, 7654321, np.uint32))
    got = st.run(loaded, g, mix)
    assert np.array_equal(got[:want.shape[0]], want)


@pytest.mark.parametrize("V,po2,widths", [(2, 9, (3, 10, 20)), (2, 12, (3, 10, 20)), (7, 9, (16, 256, 64))])
def test_the_lookup_accumulate_as_a_program_gives_lookup_refs_columns(hal, V, po2, widths):
    sh = lookup_ref.Shape(po2, *widths)
    assert sh.V == V
    code = lookup_ref.code_columns(sh)
    data, g = lookup_ref.data_columns(sh, seed=4321)
    alpha = np.random.default_rng(po2 + V).integers(0, P, 4, dtype=np.uint32).tolist()
    want = lookup_ref.accum_columns(sh, 4321, code, data, alpha)
    compiled = compile_ref(ref.lookup_program(V))
    loaded = compiled.load(hal)
    try:
        st = Stage(hal, compiled, po2, code, data, sh.wa, widths=(sh.wc, sh.wd))
        st.keep(loaded)
        got = st.run(loaded, g, alpha)
        bad = np.argwhere(got[:4 * sh.S] != want[:4 * sh.S])
        assert bad.size == 0, f"{len(bad)} accum words differ from lookup_ref, first at (column, row) {tuple(bad[0])}: {compiled.info()}"
        assert np.all(got[4 * sh.S:] == POISON)
    finally:
        loaded.unload()
        compiled.close()


# ---- the device entry points' refusals ----
def test_keep_and_run_refuse_what_does_not_fit_by_message_and_touch_nothing(hal, programs):
    prog, compiled, loaded = programs["every_form"]  # taps code column 2 and data column 5; 7 sequences, 4 of them sums
    po2 = 6
    n = 1 << po2
    code, data, g, mix = inputs(prog, po2, seed=5)
    wa = w_accum(prog)
    want = ref.evaluate(prog, po2, code, data, g, mix)
    st = Stage(hal, compiled, po2, code, data, wa)
    K, S, sums = st.info["kept"], st.info["sequences"], st.info["sums"]
    assert (S, sums) == (7, 4)
    # one allocation for the four buffers of run, so that neighbours can be made to overlap
    one = hal.copy_from(np.full(n * (K + 4 * S + sums + wa) + 4, POISON, np.uint32))
    o_kept, o_run, o_mults, o_accum = 0, n * K, n * (K + 4 * S), n * (K + 4 * S + sums)
    kept, run_ext, mults, accum = one.slice(o_kept, n * K), one.slice(o_run, 4 * n * S), one.slice(o_mults, n * sums), one.slice(o_accum, n * wa)

    def keep(**kw):
        a = dict(po2=po2, code=st.code, w_code=WIDTHS[0], data=st.data, w_data=WIDTHS[1], kept=kept)
        a.update(kw)
        loaded.keep(a["po2"], a["code"], a["w_code"], a["data"], a["w_data"], a["kept"])

    def run(**kw):
        a = dict(po2=po2, kept=kept, run_ext=run_ext, mults=mults, accum=accum, w_accum=wa)
        a.update(kw)
        loaded.run(a["po2"], a["kept"], g, mix, a["run_ext"], a["mults"], a["accum"], a["w_accum"])

    def untouched():
        return bool(np.all(one.view() == POISON)) and np.array_equal(st.code.view(), code.reshape(-1)) and np.array_equal(st.data.view(), data.reshape(-1))

    for bad in (0, 25):
        with pytest.raises(HalError, match=r"bx_acc_program_keep: po2 must be in \[1, 24\]"):
            keep(po2=bad)
        with pytest.raises(HalError, match=r"bx_acc_program_run: po2 must be in \[1, 24\]"):
            run(po2=bad)
    with pytest.raises(HalError, match=r"bx_acc_program_keep: buffer size mismatch"):
        keep(kept=one.slice(0, n * K - 1))
    with pytest.raises(HalError, match="bx_acc_program_keep: buffer size mismatch"):
        keep(po2=po2 + 1)
    with pytest.raises(HalError, match="bx_acc_program_keep: buffer size mismatch"):
        keep(data=st.data.slice(0, n * WIDTHS[1] - 1))
    with pytest.raises(HalError, match=r"bx_acc_program_keep: the program taps column 2 of group 0 \(kept column \d+\), which has 2 columns"):
        keep(code=st.code.slice(0, 2 * n), w_code=2)
    with pytest.raises(HalError, match=r"bx_acc_program_keep: the program taps column 5 of group 1 \(kept column \d+\), which has 5 columns"):
        keep(data=st.data.slice(0, 5 * n), w_data=5)
    with pytest.raises(HalError, match="bx_acc_program_keep: kept and data overlap"):
        keep(kept=st.data.slice(n, n * K))
    with pytest.raises(HalError, match="bx_acc_program_keep: kept and code overlap"):
        keep(code=one.slice(n, n * WIDTHS[0]))
    with pytest.raises(HalError, match="bx_acc_program_run: kept size mismatch"):
        run(kept=one.slice(0, n * K - 1))
    with pytest.raises(HalError, match="bx_acc_program_run: run_ext size mismatch"):
        run(run_ext=one.slice(o_run, 4 * n * S - 4))
    with pytest.raises(HalError, match="bx_acc_program_run: mults size mismatch"):
        run(mults=one.slice(o_mults, n * sums + 1))
    with pytest.raises(HalError, match="bx_acc_program_run: accum size mismatch"):
        run(accum=one.slice(o_accum, n * wa - 1))
    with pytest.raises(HalError, match="bx_acc_program_run: the program writes 28 accum columns, the accum group has 27"):
        run(accum=one.slice(o_accum, n * 27), w_accum=27)
    with pytest.raises(HalError, match="bx_acc_program_run: run_ext must be 16-byte aligned"):
        run(run_ext=one.slice(o_run + 1, 4 * n * S), mults=one.slice(o_mults + 1, n * sums), accum=one.slice(o_accum + 1, n * wa))
    for name, kw in (("run_ext and mults", dict(mults=one.slice(o_mults - 1, n * sums))),
                     ("run_ext and accum", dict(accum=one.slice(o_run + 4 * n, n * wa), mults=st.mults)),
                     ("run_ext and kept", dict(run_ext=one.slice(o_run - 4, 4 * n * S), mults=st.mults, accum=st.accum)),
                     ("mults and accum", dict(accum=one.slice(o_accum - 1, n * wa))),
                     ("mults and kept", dict(mults=one.slice(o_kept + n, n * sums), run_ext=st.run_ext, accum=st.accum)),
                     ("accum and kept", dict(accum=one.slice(0, n * wa), run_ext=st.run_ext, mults=st.mults))):
        with pytest.raises(HalError, match=f"bx_acc_program_run: {name} overlap"):
            run(**kw)
    other = HipHal(0)
    try:
        with pytest.raises(HalError, match="bx_acc_program_keep: the program was loaded on another ctx"):
            other.acc_program_keep(loaded, po2, st.code, WIDTHS[0], st.data, WIDTHS[1], kept)
        with pytest.raises(HalError, match="bx_acc_program_run: the program was loaded on another ctx"):
            other.acc_program_run(loaded, po2, kept, g, mix, run_ext, mults, accum, wa)
    finally:
        other.close()
    assert untouched() and np.all(st.accum.view() == POISON) and np.all(st.run_ext.view() == POISON)
    keep()  # still good after the refusals
    run()
    assert np.array_equal(accum.view().reshape(wa, n)[:4 * S], want)


# ---- through a proof: a multiset circuit whose accumulate is the program alone ----
FILL = 424242  # what the base's accumulate leaves in every accum cell


def _multiset_programs(n_globals=0, sequences=4, extra_tap=None):
    """constraints and accumulate of: a, b = data columns 0, 1; sequences 0, 1 the LogUp sums of 1 / (alpha - a) and 1 / (alpha - b),
    sequences 2, 3 the running products of alpha - a and alpha - b; both pairs agree on the last row iff b is a permutation of a"""
    import cons_program_ref

    p = cons_program_ref.Program(0)
    xk = [None] + [p.const_ext(*[1 if i == k else 0 for i in range(4)]) for k in (1, 2, 3)]

    def ext_of(words):
        r = words[0]
        for k in (1, 2, 3):
            r = p.add(r, p.mul(xk[k], words[k]))
        return r

    alpha = ext_of([p.mix(k) for k in range(4)])
    first, last = p.get(0, 0), p.get(0, 1)
    not_first = p.sub(p.const(1), first)
    x = [p.get(1, 0), p.get(1, 1)]
    cur = [ext_of([p.get(2, 4 * s + k, 0) for k in range(4)]) for s in range(4)]
    back = [ext_of([p.get(2, 4 * s + k, 1) for k in range(4)]) for s in range(4)]
    top = p.true()
    for s in (0, 1):  # (S(r) - (1 - first) S(r-1)) (alpha - x) - 1
        top = p.and_eqz(top, p.sub(p.mul(p.sub(cur[s], p.mul(not_first, back[s])), p.sub(alpha, x[s])), p.const(1)))
    for s in (2, 3):  # P(r) - (first + (1 - first) P(r-1)) (alpha - x)
        top = p.and_eqz(top, p.sub(cur[s], p.mul(p.add(p.mul(not_first, back[s]), first), p.sub(alpha, x[s - 2]))))
    top = p.and_eqz(top, p.mul(last, p.sub(cur[0], cur[1])))
    top = p.and_eqz(top, p.mul(last, p.sub(cur[2], cur[3])))
    cons = p.done(top)

    a = ref.Program(n_globals)
    al, one = a.alpha(), a.const(1)
    terms = [a.sub(al, a.get(1, 0)), a.sub(al, a.get(1, 1))]
    if extra_tap is not None:
        a.tap(*extra_tap)
    a.sum_(0, one, terms[0])
    a.sum_(1, one, terms[1])
    a.prod(2, terms[0])
    a.prod(3, terms[1])
    for s in range(4, sequences):
        a.prod(s, terms[0])
    return cons, a


class MultisetCircuit:
    """code: first, last selectors.  data: a random, b a permutation of it (or not: `cheat`).  accum: `numpy` = the reference's
    columns (the all-numpy twin, whose eval_check and constraints_at are the reference evaluators of the constraint program too);
    otherwise FILL everywhere — the accumulate program has to overwrite all of it."""

    def __init__(self, lib, numpy, cheat=False):
        self.lib, self.numpy, self.cheat, self.calls = lib, numpy, cheat, []
        self.cons, self.acc = _multiset_programs()

    def bind(self, po2, widths):
        self.po2, self.n, (self.wc, self.wd, self.wa) = po2, 1 << po2, widths

    def normalize(self, shape):
        shape.cons_terms, shape.cons_degree = 6, 3

    def taps(self, shape, group, col):
        return [0, 1] if group == 2 and col < 16 else [0]

    def n_globals(self, shape):
        return 0

    def _put(self, ctx, buf, words):
        m = np.ascontiguousarray(words, np.uint32).reshape(-1)
        assert m.size == buf.len
        msg = self.lib.bx_h2d(ctx, buf, m.ctypes.data, m.size)
        assert not msg, msg

    def _get(self, ctx, buf):
        out = np.empty(buf.len, np.uint32)
        msg = self.lib.bx_d2h(ctx, out.ctypes.data, buf, out.size)
        assert not msg, msg
        return out

    def _code(self):
        code = np.zeros((self.wc, self.n), np.uint32)
        code[0][0] = code[1][self.n - 1] = ref.encode(1)
        return code

    def code_group(self, ctx, code):
        self.calls.append("code_group")
        self._put(ctx, code, self._code())

    def witgen(self, ctx, code, data, segment, segment_dev):
        self.calls.append("witgen")
        rng = np.random.default_rng(int.from_bytes(segment[20:28], "little") & 0xFFFFFFFF)
        self.data = rng.integers(0, P, (self.wd, self.n), dtype=np.uint32)
        self.data[1] = rng.permutation(self.data[0])
        if self.cheat:
            self.data[1][5] = (int(self.data[1][5]) + 1) % P
        self._put(ctx, data, self.data)
        return []

    def accumulate(self, ctx, accum, mix):
        self.calls.append("accumulate")
        if self.numpy:
            self._put(ctx, accum, ref.evaluate(self.acc, self.po2, self._code(), self.data, [], mix))
        else:
            self._put(ctx, accum, np.full(self.wa * self.n, FILL, np.uint32))

    def eval_check(self, ctx, check, code_eval, data_eval, accum_eval, poly_mix, mix, globals_):
        import cons_program_ref

        self.calls.append("eval_check")
        dom = 4 * self.n
        evals = [self._get(ctx, b).reshape(-1, dom) for b in (code_eval, data_eval, accum_eval)]
        self._put(ctx, check, cons_program_ref.check_planes(self.cons, self.po2, evals, np.array(poly_mix, np.uint64), np.array(mix, np.uint64), []))

    def constraints_at(self, shape, tap, poly_mix, mix, globals_):
        import cons_program_ref

        return cons_program_ref.at_point(self.cons, tap, np.array(poly_mix, np.uint64), np.array(mix, np.uint64), [])


def _prove_multiset(numpy, cheat=False, acc=None, po2=9, widths=(2, 2, 16), seed=99):
    from cons_program_cases import compile_ref as compile_cons
    from boundless_amd.hal import load_library

    circ = MultisetCircuit(load_library(), numpy, cheat)
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, b"multiset")
    if not numpy:
        ops = CircuitOps.from_program(compile_cons(circ.cons), ops, accumulate=compile_ref(circ.acc if acc is None else acc))
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_a_circuit_whose_accumulate_is_a_program_proves_its_numpy_twins_seal():
    want, numpy_ops, numpy_ctx, twin = _prove_multiset(numpy=True)
    assert twin.calls == ["code_group", "witgen", "accumulate", "eval_check"]
    verify_seal(want.seal, circuit=numpy_ops, ctx=numpy_ctx)
    got, ops, vctx, circ = _prove_multiset(numpy=False)
    assert circ.calls == ["code_group", "witgen", "accumulate"]  # the base's accumulate ran (and wrote FILL), eval_check did not come from numpy
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # b is not a permutation of a: every local constraint holds, the sums and the products do not meet on the last row
    receipt, ops, vctx, _ = _prove_multiset(numpy=False, cheat=True)
    with pytest.raises(HalError, match="constraint identity"):
        verify_seal(receipt.seal, circuit=ops, ctx=vctx)


def test_the_composite_table_checks_the_accumulate_program_against_the_shape():
    for kw, match in ((dict(sequences=5), "accumulate program: 5 sequences need 20 accum columns, the shape has 16"),
                      (dict(extra_tap=(1, 2, 0)), r"accumulate program: the program taps column 2 of group 1 \(kept column 2\), which has 2 columns"),
                      (dict(extra_tap=(0, 2, 1)), r"accumulate program: the program taps column 2 of group 0 \(kept column 2\), which has 2 columns"),
                      (dict(n_globals=1), "accumulate program: the program has 1 globals, the base circuit 0")):
        with pytest.raises(HalError, match=match):
            _prove_multiset(numpy=False, acc=_multiset_programs(**kw)[1])


# ---- through a proof: the built-in lookup circuit, constraints and accumulate both from programs ----
@pytest.mark.parametrize("po2,widths,V", [(9, (3, 10, 20), 2)])
def test_the_lookup_circuit_with_both_programs_proves_the_built_in_circuits_seal(po2, widths, V):
    import cons_program_ref
    from cons_program_cases import compile_ref as compile_cons

    hal = HipHal(0)
    ops = CircuitOps.from_program(compile_cons(cons_program_ref.lookup_program(po2, widths)), lookup_circuit(), accumulate=compile_ref(ref.lookup_program(V)))
    builtin, composite = HipProverServer(0, po2=po2, widths=widths, circuit="lookup"), HipProverServer(0, po2=po2, widths=widths, circuit=ops, hal=hal)
    try:
        B = 1 << min(15, po2 - 1)
        records = [(0, 0, 7 + B * 9), (1, 0, 7), (2, 0, 9)]  # consistent in-range records for (v_0, lo_0, hi_0) at row 0
        hal.profile_reset()
        hal.profile_enable(True)
        for seg in (Segment(index=0, po2=po2, seed=500 + po2), Segment(index=1, po2=po2, seed=600 + po2, payload=encode_cell_records(records))):
            a, b = builtin.prove_segment(seg), composite.prove_segment(seg)
            assert np.array_equal(a.seal, b.seal), f"first differing seal word: {int(np.argmax(a.seal != b.seal))}"
            verify_seal(b.seal, circuit=ops)
            verify_seal(b.seal, circuit="lookup")
        hal.profile_enable(False)
        report = hal.profile_report()
        # the base's accumulate still ran (it owns the filler), so there are two LogUp scans per proof
        for op, calls in (("acc_program_keep", 2), ("acc_program_run", 2), ("acc_program_store", 2), ("lookup_build", 2), ("logup_accumulate", 4)):
            assert report[op]["calls"] == calls, (op, report.get(op), sorted(report))
    finally:
        builtin.close()
        composite.close()
        hal.close()


# ---- what a ctx holds ----
def test_load_and_unload_return_their_memory_and_bx_free_releases_what_is_left():
    import torch

    compiled = compile_ref(ref.PROGRAMS["steps_700"]())
    HipHal(0).close()  # the first ctx of a process loads the code objects: not part of what is measured
    h = HipHal(0)
    try:
        compiled.load(h).unload()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        for _ in range(10):
            compiled.load(h).unload()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before
        twice = compiled.load(h)
        dev = twice.dev
        twice.unload()
        with pytest.raises(HalError, match="bx_acc_program_unload: not a loaded program"):
            h._check(compiled.lib.bx_acc_program_unload(dev))
        kept = [compiled.load(h) for _ in range(3)]  # still loaded when the ctx goes
    finally:
        h.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before
    for k in kept:
        dev, k.dev = k.dev, None  # released by bx_free: an unload of the freed handle is answered by message
        assert b"not a loaded program" in compiled.lib.bx_acc_program_unload(dev)
