"""GPU: the RATIO step of accumulate programs (include/bx_program.h "Accumulate programs", csrc/acc_program.hip) — keep + run against
the definition-level reference of tests/acc_ratio_ref.py and against the host executor, word for word over accum columns [0, 4 S),
with the columns above still poisoned; the size of run_ext; what a ctx holds; and the two-column multiset circuit of
tests/test_acc_program_gpu.py once more with ONE ratio sequence — w_accum 4 where the two-products form needs 16 — against its
all-numpy twin, seal for seal.

Sizes as in tests/test_acc_program_gpu.py: po2 1 (a tap 3 rows back wraps), 6 and 7 (less than one workgroup), 8 (one exactly), 9 (two,
and the prover's smallest), 12 (two scan tiles of 2048 elements)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_program_ref as ref  # noqa: E402
import acc_ratio_ref as rref  # noqa: E402
import extreme_words  # noqa: E402
from acc_ratio_cases import POISON, compile_ref, inputs, w_accum  # noqa: E402

from boundless_amd.circuit import CircuitOps  # noqa: E402
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
    for name, make in rref.PROGRAMS.items():
        prog = make()
        compiled = compile_ref(prog)
        out[name] = (prog, compiled, compiled.load(hal))
    yield out
    for _, compiled, loaded in out.values():
        loaded.unload()
        compiled.close()


class Stage:
    """the device buffers of one keep + run, the work space and the accum group poisoned; run_ext holds S + R sequences"""

    def __init__(self, hal, compiled, po2, code, data, wa, widths=WIDTHS):
        info = compiled.info()
        n = 1 << po2
        self.hal, self.po2, self.n, self.wa, self.widths, self.info = hal, po2, n, wa, widths, info
        self.code, self.data = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        self._kept = hal.copy_from(np.full(max(n * info["kept"], 1), POISON, np.uint32))
        self._mults = hal.copy_from(np.full(max(n * info["sums"], 1), POISON, np.uint32))
        self.kept, self.mults = self._kept.slice(0, n * info["kept"]), self._mults.slice(0, n * info["sums"])
        self.run_ext = hal.copy_from(np.full(4 * n * (info["sequences"] + compiled.ratios()), POISON, np.uint32))
        self.accum = hal.copy_from(np.full(wa * n, POISON, np.uint32))

    def keep(self, loaded):
        loaded.keep(self.po2, self.code, self.widths[0], self.data, self.widths[1], self.kept)

    def run(self, loaded, g, mix, run_ext=None):
        loaded.run(self.po2, self.kept, g, mix, self.run_ext if run_ext is None else run_ext, self.mults, self.accum, self.wa)
        return self.accum.view().reshape(self.wa, self.n)


def _check_stage(hal, prog, compiled, loaded, po2, pattern, seed, what):
    code, data, g, mix = inputs(prog, po2, pattern=pattern, seed=seed)
    wa, S = w_accum(prog), len(prog.sequences())
    want = rref.evaluate(prog, po2, code, data, g, mix)
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
@pytest.mark.parametrize("name", list(rref.PROGRAMS))
def test_keep_and_run_are_the_reference_and_the_host_executor_on_every_word(hal, programs, name, po2):
    prog, compiled, loaded = programs[name]
    want = _check_stage(hal, prog, compiled, loaded, po2, "random", len(prog.steps), f"{name} at po2 {po2}")
    if name == "ratio_zero_denominator":
        for s, row in enumerate(rref.planted_zero_rows(1 << po2)):
            assert not want[4 * s:4 * s + 4, row:].any() and np.all(want[4 * s:4 * s + 4, :row].any(axis=0))
    elif po2 >= 6:
        assert len(np.unique(want[0])) > (1 << po2) // 2, "degenerate reference: a stage that writes a constant could pass"


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_keep_and_run_are_the_reference_on_extreme_columns(hal, programs, pattern):
    for name, (prog, compiled, loaded) in programs.items():
        _check_stage(hal, prog, compiled, loaded, 7, pattern, 0, f"{name} on {pattern}")


def test_run_ext_without_room_for_the_denominators_is_refused_by_message(hal, programs):
    prog, compiled, loaded = programs["all_three_kinds"]
    po2 = 6
    n = 1 << po2
    code, data, g, mix = inputs(prog, po2, seed=5)
    S, R = compiled.info()["sequences"], compiled.ratios()
    assert (S, R) == (6, 2)
    st = Stage(hal, compiled, po2, code, data, w_accum(prog))
    st.keep(loaded)
    with pytest.raises(HalError, match=r"bx_acc_program_run: run_ext size mismatch \(4 N words per sequence and 4 N more per RATIO: its denominators\)"):
        st.run(loaded, g, mix, run_ext=st.run_ext.slice(0, 4 * n * S))
    with pytest.raises(HalError, match="bx_acc_program_run: run_ext size mismatch"):
        st.run(loaded, g, mix, run_ext=st.run_ext.slice(0, 4 * n * (S + R) - 4))
    assert np.all(st.accum.view() == POISON) and np.all(st.run_ext.view() == POISON) and np.all(st._mults.view() == POISON)
    got = st.run(loaded, g, mix)  # still good after the refusals
    assert np.array_equal(got[:4 * S], rref.evaluate(prog, po2, code, data, g, mix))


def test_the_scans_of_a_program_with_all_three_kinds_are_one_call_each(hal, programs):
    prog, compiled, loaded = programs["all_three_kinds"]
    code, data, g, mix = inputs(prog, 9, seed=2)
    st = Stage(hal, compiled, 9, code, data, w_accum(prog))
    st.keep(loaded)
    hal.profile_reset()
    hal.profile_enable(True)
    try:
        st.run(loaded, g, mix)
        report = hal.profile_report()
    finally:
        hal.profile_enable(False)
        hal.profile_reset()
    for op in ("acc_program_run", "logup_accumulate", "prefix_products", "ratio_products", "acc_program_store"):
        assert report[op]["calls"] == 1, (op, report.get(op), sorted(report))


def test_load_and_unload_return_their_memory_and_bx_free_releases_what_is_left():
    import torch

    compiled = compile_ref(rref.every_ratio_form_program())
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


# ---- through a proof: the multiset circuit with one ratio sequence, w_accum 4 ----
FILL = 424242  # what the base's accumulate leaves in every accum cell


def _multiset_ratio_programs():
    """a, b = data columns 0, 1.  accumulate: ONE sequence z(r) = prod_{j <= r} (alpha - a(j)) / (alpha - b(j)).  constraints:
    z(r) (alpha - b(r)) = z(r-1) (alpha - a(r)), with 1 in place of z(r-1) on the first row, and z = 1 on the last row, which holds
    iff b is a permutation of a"""
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
    a, b = p.get(1, 0), p.get(1, 1)
    z = ext_of([p.get(2, k, 0) for k in range(4)])
    z_back = ext_of([p.get(2, k, 1) for k in range(4)])
    top = p.true()
    # z(r) (alpha - b) - (first + (1 - first) z(r-1)) (alpha - a)
    top = p.and_eqz(top, p.sub(p.mul(z, p.sub(alpha, b)), p.mul(p.add(p.mul(not_first, z_back), first), p.sub(alpha, a))))
    top = p.and_eqz(top, p.mul(last, p.sub(z, p.const(1))))
    return p.done(top), rref.permutation_program()


class MultisetRatioCircuit:
    """code: first, last selectors.  data: a random, b a permutation of it (or not: `cheat`).  accum (4 columns): `numpy` = the
    reference's columns (the all-numpy twin, whose eval_check and constraints_at are the reference evaluators of the constraint
    program too); otherwise FILL everywhere — the accumulate program has to overwrite all of it."""

    def __init__(self, lib, numpy, cheat=False):
        self.lib, self.numpy, self.cheat, self.calls = lib, numpy, cheat, []
        self.cons, self.acc = _multiset_ratio_programs()

    def bind(self, po2, widths):
        self.po2, self.n, (self.wc, self.wd, self.wa) = po2, 1 << po2, widths

    def normalize(self, shape):
        shape.cons_terms, shape.cons_degree = 2, 3

    def taps(self, shape, group, col):
        return [0, 1] if group == 2 and col < 4 else [0]

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
            self._put(ctx, accum, rref.evaluate(self.acc, self.po2, self._code(), self.data, [], mix))
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


def _prove_multiset(numpy, cheat=False, po2=9, widths=(2, 2, 4), seed=99):
    from cons_program_cases import compile_ref as compile_cons
    from boundless_amd.hal import load_library

    circ = MultisetRatioCircuit(load_library(), numpy, cheat)
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, b"multiset-ratio")
    if not numpy:
        ops = CircuitOps.from_program(compile_cons(circ.cons), ops, accumulate=compile_ref(circ.acc))
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_the_multiset_circuit_with_one_ratio_sequence_proves_its_numpy_twins_seal():
    want, numpy_ops, numpy_ctx, twin = _prove_multiset(numpy=True)
    assert twin.calls == ["code_group", "witgen", "accumulate", "eval_check"]
    verify_seal(want.seal, circuit=numpy_ops, ctx=numpy_ctx)
    got, ops, vctx, circ = _prove_multiset(numpy=False)
    assert circ.calls == ["code_group", "witgen", "accumulate"]
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # b is not a permutation of a: the transition holds on every row, z does not come back to 1 on the last
    receipt, ops, vctx, _ = _prove_multiset(numpy=False, cheat=True)
    with pytest.raises(HalError, match="constraint identity"):
        verify_seal(receipt.seal, circuit=ops, ctx=vctx)
