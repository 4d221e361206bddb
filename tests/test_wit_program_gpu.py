"""GPU: witness programs (include/bx_program.h "Witness programs", csrc/wit_program.hip) — the interpreting kernel against the
definition-level reference of tests/wit_program_ref.py and against the host executor, word for word over the whole data group; the
synthetic circuit's derive stage written as a program against tests/synth_ref.py; the entry point's refusals; the square circuit of
tests/test_circuit_plugin_gpu.py with its derived column from a witness program against the all-numpy original, seal for seal; a
second small circuit whose public word is a derived cell; and what a ctx holds.

Sizes are the smallest at which each thing can break: po2 1 (two rows: a tap 1 or 3 rows back wraps), 6 and 7 (less than one
workgroup: lanes return early), 8 (one workgroup exactly), 9 (two workgroups, and the prover's smallest); programs of one SET, about
40 and about 700 steps, every step form with a forwarded value used three columns later, and 32 live values (the whole 32 KiB of LDS);
and, at po2 1 and 9, the shortest stream there is (a constant, a store, padding) and a destination slot that is both its sources."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import synth_ref  # noqa: E402
import wit_program_ref as ref  # noqa: E402
from wit_program_cases import columns, compile_ref  # noqa: E402

from boundless_amd.circuit import CircuitOps, ConsProgram, WitnessProgram  # noqa: E402
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


def _three_ways(hal, prog, compiled, loaded, po2, code, data, widths=WIDTHS):
    """the data group after the program: by the kernel, by the reference and by the host executor"""
    want = ref.evaluate(prog, po2, code, data)
    host = data.copy()
    compiled.run_host(po2, code, widths[0], host, widths[1])
    dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
    loaded.run(po2, dcode, widths[0], ddata, widths[1])
    got = ddata.view().reshape(widths[1], -1)
    assert np.array_equal(dcode.view(), code.reshape(-1)), "the code group was written"
    dcode.free()
    ddata.free()
    return got, want, host


def _assert_same(prog, got, want, host, data, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} data words differ from the reference, first at (column, row) {tuple(bad[0])}"
    assert np.array_equal(host, want), f"{what}: the host executor differs from the reference"
    free = [c for c in range(data.shape[0]) if c not in prog.derived()]
    assert np.array_equal(got[free], data[free]), f"{what}: a free column was written"


@pytest.mark.parametrize("po2", [1, 6, 7, 8, 9])
@pytest.mark.parametrize("name", list(ref.PROGRAMS))
def test_run_is_the_reference_and_the_host_executor_on_every_row(hal, programs, name, po2):
    prog, compiled, loaded = programs[name]
    code, data = columns(prog, po2, WIDTHS, "random", seed=len(prog.steps))
    got, want, host = _three_ways(hal, prog, compiled, loaded, po2, code, data)
    assert not np.any(want[prog.derived()] == P - 1), "degenerate reference: a kernel that writes nothing could pass"
    _assert_same(prog, got, want, host, data, f"{name} at po2 {po2}: {compiled.info()}")


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_run_is_the_reference_on_extreme_columns(hal, programs, pattern):
    po2 = 7
    for name, (prog, compiled, loaded) in programs.items():
        code, data = columns(prog, po2, WIDTHS, pattern)
        got, want, host = _three_ways(hal, prog, compiled, loaded, po2, code, data)
        _assert_same(prog, got, want, host, data, f"{name} on {pattern}")


def _lone_constant_program():
    """one constant, one store, and two NOPs of padding: the shortest stream there is"""
    p = ref.Program()
    p.set(3, p.const(7))
    return p


def _aliased_destination_program():
    """x = data[0](r-1); y = x * x with x dead afterwards, so that y takes x's slot: an instruction whose destination is both its sources"""
    p = ref.Program()
    x = p.get(1, 0, 1)
    p.set(3, p.add(p.mul(x, x), p.get(0, 1, 0)))
    return p


@pytest.mark.parametrize("po2", [1, 9])  # two rows: most of the only wave returns at once, and row 0 wraps to the last row; two workgroups
def test_the_shortest_stream_and_a_destination_that_is_its_own_source(hal, programs, po2):
    assert programs["narrow_limit"][1].info()["narrow"] == ref.MAX_NARROW  # the named programs reach the whole slot file
    for name, make, instructions, text in (("lone constant", _lone_constant_program, 2, "at.store(3u, n0)"),
                                           ("aliased destination", _aliased_destination_program, 5, "n0 = fp_mul(n0, n0)")):
        prog = make()
        compiled = compile_ref(prog)
        assert compiled.info()["instructions"] == instructions and text in compiled.emit_hip(), f"{name}: the compiled stream is not the one this test is about"
        loaded = compiled.load(hal)
        try:
            code, data = columns(prog, po2, WIDTHS, "random", seed=3)
            got, want, host = _three_ways(hal, prog, compiled, loaded, po2, code, data)
            assert not np.any(want[prog.derived()] == P - 1), "degenerate reference: a kernel that writes nothing could pass"
            _assert_same(prog, got, want, host, data, f"{name} at po2 {po2}: {compiled.info()}")
        finally:
            loaded.unload()
            compiled.close()


# ---- the synthetic circuit's derive stage as a program ----
@pytest.mark.parametrize("T,G", [(8, 2), (64, 4)])
def test_the_synthetic_derive_stage_as_a_program_gives_synth_refs_columns(hal, T, G):
    po2, w = 9, 16
    sh = synth_ref.Shape(po2, w, w, w, T, G)
    prog = ref.synthetic_derive_program(w, w, T, G)
    compiled = compile_ref(prog)
    loaded = compiled.load(hal)
    try:
        want, _ = synth_ref.data_columns(sh, seed=4321)
        code = synth_ref.code_columns(sh)
        data = want.copy()
        data[sh.F:] = P - 1  # the free cells are synth_ref's, the derived ones poison
        dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
        loaded.run(po2, dcode, w, ddata, w)
        got = ddata.view().reshape(w, -1)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{len(bad)} data words differ from synth_ref, first at (column, row) {tuple(bad[0])}: {compiled.info()}"
    finally:
        loaded.unload()
        compiled.close()


# ---- the device entry point's refusals ----
def test_run_refuses_what_does_not_fit_by_message_and_touches_nothing(hal, programs):
    prog, compiled, loaded = programs["every_form"]  # taps code column 2 and data column 5, sets data column 7
    po2 = 6
    n = 1 << po2
    code, data = columns(prog, po2, WIDTHS, "random", seed=5)
    want = ref.evaluate(prog, po2, code, data)
    both = hal.alloc((WIDTHS[0] + WIDTHS[1]) * n)  # one allocation: code, then data
    dcode, ddata = both.slice(0, WIDTHS[0] * n), both.slice(WIDTHS[0] * n, WIDTHS[1] * n)

    def reset():
        dcode.copy_from(code.reshape(-1))
        ddata.copy_from(data.reshape(-1))

    def untouched():
        return np.array_equal(dcode.view(), code.reshape(-1)) and np.array_equal(ddata.view(), data.reshape(-1))

    reset()
    with pytest.raises(HalError, match=r"bx_wit_program_run: buffer size mismatch \(groups N x width\)"):
        loaded.run(po2, dcode, WIDTHS[0], ddata.slice(0, WIDTHS[1] * n - 1), WIDTHS[1])
    with pytest.raises(HalError, match="buffer size mismatch"):
        loaded.run(po2, dcode.slice(0, 2 * n), WIDTHS[0], ddata, WIDTHS[1])
    with pytest.raises(HalError, match="buffer size mismatch"):
        loaded.run(po2 + 1, dcode, WIDTHS[0], ddata, WIDTHS[1])
    with pytest.raises(HalError, match="bx_wit_program_run: the program sets data column 7, the data group has 7 columns"):
        loaded.run(po2, dcode, WIDTHS[0], ddata.slice(0, 7 * n), 7)
    with pytest.raises(HalError, match="bx_wit_program_run: the program taps column 2 of group 0, which has 2 columns"):
        loaded.run(po2, dcode.slice(0, 2 * n), 2, ddata, WIDTHS[1])
    with pytest.raises(HalError, match="bx_wit_program_run: code and data overlap"):
        loaded.run(po2, both.slice(n, WIDTHS[0] * n), WIDTHS[0], ddata, WIDTHS[1])  # the last code column is the first data column
    with pytest.raises(HalError, match="code and data overlap"):
        loaded.run(po2, both.slice(WIDTHS[0] * n, WIDTHS[0] * n), WIDTHS[0], ddata, WIDTHS[1])  # code inside data
    for bad in (0, 25):
        with pytest.raises(HalError, match=r"po2 must be in \[1, 24\]"):
            loaded.run(bad, dcode, WIDTHS[0], ddata, WIDTHS[1])
    other = HipHal(0)
    try:
        with pytest.raises(HalError, match="loaded on another ctx"):
            other.wit_program_run(loaded, po2, dcode, WIDTHS[0], ddata, WIDTHS[1])
    finally:
        other.close()
    assert untouched()
    loaded.run(po2, dcode, WIDTHS[0], ddata, WIDTHS[1])  # still good after the refusals
    assert np.array_equal(ddata.view().reshape(WIDTHS[1], n), want)
    both.free()


# ---- through a proof: the square circuit, its derived column from a witness program ----
def _square_classes():
    from oracle import oracle_lib as ol
    from test_circuit_plugin_gpu import Fp4, SquareCircuit, fmul

    class FreeCellsOnly(SquareCircuit):
        """the square circuit's base: witgen places the free cells (data columns 0 and 2) and leaves poison in the derived column"""

        def witgen(self, ctx, code, data, segment, segment_dev):
            self.calls.append("witgen")
            self.seed = seed = int.from_bytes(segment[20:28], "little")
            data_w = np.random.default_rng(seed & 0xFFFFFFFF).integers(0, P, (self.wd, self.n), dtype=np.uint64)
            data_w[1] = P - 1
            self._put(ctx, data, data_w.reshape(-1))
            return ol.encode([int(data_w[0][0])]).tolist()

    class CubeCircuit(SquareCircuit):
        """data[1] = data[0]^3 + code[0];  g = data[1][0], tied to the trace by first * (data[1] - g) with first = code[1]; all numpy"""

        def normalize(self, shape):
            shape.cons_terms, shape.cons_degree = 1, 3

        def taps(self, shape, group, col):
            return [0]

        def _free(self, segment):
            self.seed = seed = int.from_bytes(segment[20:28], "little")
            return np.random.default_rng(seed & 0xFFFFFFFF).integers(0, P, (self.wd, self.n), dtype=np.uint64)

        def witgen(self, ctx, code, data, segment, segment_dev):
            self.calls.append("witgen")
            data_w = self._free(segment)
            x = data_w[0]
            data_w[1] = (fmul(fmul(x, x), x) + self._code()[0]) % np.uint64(P)
            self._put(ctx, data, data_w.reshape(-1))
            return ol.encode([int(data_w[1][0])]).tolist()

        def eval_check(self, ctx, check, code_eval, data_eval, accum_eval, poly_mix, mix, globals_):
            self.calls.append("eval_check")
            from test_circuit_plugin_gpu import ROU_FWD2

            dom = 4 * self.n
            c0, first = self._get(ctx, code_eval, 0, dom), self._get(ctx, code_eval, dom, dom)
            d0, d1 = self._get(ctx, data_eval, 0, dom), self._get(ctx, data_eval, dom, dom)
            g = np.uint64(ol.decode(np.array(globals_, np.uint32))[0])
            pm = ol.decode(np.array(poly_mix, np.uint32)).astype(np.uint64)
            cons = (d1 + np.uint64(2 * P) - fmul(fmul(d0, d0), d0) - c0) % np.uint64(P)
            bound = fmul(first, (d1 + np.uint64(P) - g) % np.uint64(P))
            t3n = pow(3, self.n, P)
            zinv = np.array([pow((t3n * pow(ROU_FWD2, m, P) - 1) % P, -1, P) for m in range(4)], np.uint64)
            zi = zinv[np.arange(dom) % 4]
            planes = np.zeros(4 * dom, np.uint64)
            for k in range(4):
                tot = fmul(bound, pm[k])
                if k == 0:
                    tot = (tot + cons) % np.uint64(P)
                planes[k * dom:(k + 1) * dom] = fmul(tot, zi)
            self._put(ctx, check, planes)

        def constraints_at(self, shape, tap, poly_mix, mix, globals_):
            d0, d1, c0, first = (Fp4.from_mont(tap(*t)) for t in ((1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 1, 0)))
            g = Fp4([int(ol.decode(np.array(globals_, np.uint32))[0]), 0, 0, 0])
            return (d1 - d0 * d0 * d0 - c0 + Fp4.from_mont(poly_mix) * (first * (d1 - g))).to_mont()

    class CubeFreeCellsOnly(CubeCircuit):
        """the cube circuit's base: free cells only, poison in the derived column, and a public word that is NOT the trace's"""

        def witgen(self, ctx, code, data, segment, segment_dev):
            self.calls.append("witgen")
            data_w = self._free(segment)
            data_w[1] = P - 1
            self._put(ctx, data, data_w.reshape(-1))
            return [12345]  # overridden by the global cell

    return SquareCircuit, FreeCellsOnly, CubeCircuit, CubeFreeCellsOnly


def _square_witness(k=1):
    """data[1] = data[0]^2 + code[0] * data[0](r-1) + k * data[0](r-3); the circuit has k = 1"""
    w = WitnessProgram()
    x, xb, xb3, c0 = w.get(1, 0, 0), w.get(1, 0, 1), w.get(1, 0, 3), w.get(0, 0, 0)
    w.set(1, w.add(w.add(w.mul(x, x), w.mul(c0, xb)), w.mul(w.const(k), xb3)))
    return w.compile()


def _cube_programs(row=0, index=0):
    p = ConsProgram(n_globals=1)
    d0, d1, c0, first, g = p.get(1, 0, 0), p.get(1, 1, 0), p.get(0, 0, 0), p.get(0, 1, 0), p.global_(0)
    top = p.and_eqz(p.true(), p.sub(p.sub(d1, p.mul(p.mul(d0, d0), d0)), c0))
    cons = p.compile(ret=p.and_eqz(top, p.mul(first, p.sub(d1, g))))
    w = WitnessProgram()
    x = w.get(1, 0, 0)
    w.set(1, w.add(w.mul(w.mul(x, x), x), w.get(0, 0, 0)))
    w.global_cell(index, 1, row)
    return cons, w.compile()


def _prove(circ, po2, widths, seed, cons=None, witness=None, name=b"square-plus-back"):
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, name)
    if cons is not None:
        ops = CircuitOps.from_program(cons, ops, witness=witness)
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx
    finally:
        srv.close()


def test_the_square_circuit_with_its_derived_column_from_a_witness_program_proves_the_numpy_circuits_seal():
    import cons_program_ref
    from cons_program_cases import compile_ref as compile_cons
    from boundless_amd.hal import load_library

    SquareCircuit, FreeCellsOnly, _, _ = _square_classes()
    lib = load_library()
    po2, widths = 9, (2, 3, 2)
    want, numpy_ops, numpy_ctx = _prove(SquareCircuit(lib), po2, widths, 77)
    cons = compile_cons(cons_program_ref.square_program())
    base = FreeCellsOnly(lib)
    got, ops, vctx = _prove(base, po2, widths, 77, cons=cons, witness=_square_witness())
    assert base.calls == ["code_group", "witgen", "accumulate"]  # eval_check did not come from numpy
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # without the witness program the poison stays in the derived column; with one wrong constant the column is not the circuit's
    for witness in (None, _square_witness(k=2)):
        receipt, ops, vctx = _prove(FreeCellsOnly(lib), po2, widths, 77, cons=cons, witness=witness)
        with pytest.raises(HalError, match="constraint identity"):
            verify_seal(receipt.seal, circuit=ops, ctx=vctx)


def test_a_circuit_whose_public_word_is_a_derived_cell_proves_its_numpy_twins_seal():
    from oracle import oracle_lib as ol
    from boundless_amd.hal import load_library

    _, _, CubeCircuit, CubeFreeCellsOnly = _square_classes()
    lib = load_library()
    po2, widths = 9, (2, 3, 2)
    want, numpy_ops, numpy_ctx = _prove(CubeCircuit(lib), po2, widths, 31, name=b"cube")
    verify_seal(want.seal, circuit=numpy_ops, ctx=numpy_ctx)
    cons, wit = _cube_programs()
    got, ops, vctx = _prove(CubeFreeCellsOnly(lib), po2, widths, 31, cons=cons, witness=wit, name=b"cube")
    assert int(got.seal[6]) != 12345 and int(ol.decode(got.seal[6:7])[0]) < P  # the base's word was overridden by data[1][0]
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # the shape-dependent part of a description is checked when a prover is created
    for kw, match in (({"row": 1 << po2}, "witness program: global cell 0 reads row 512, the trace has 512 rows"),
                      ({"index": 1}, "witness program: global cell 0 names global 1, the base circuit has 1")):
        cons, wit = _cube_programs(**kw)
        with pytest.raises(HalError, match=match):
            _prove(CubeFreeCellsOnly(lib), po2, widths, 31, cons=cons, witness=wit, name=b"cube")
    w = WitnessProgram()
    w.set(3, w.get(1, 0, 0))
    with pytest.raises(HalError, match="witness program: the program sets data column 3, the data group has 3 columns"):
        _prove(CubeFreeCellsOnly(lib), po2, widths, 31, cons=cons, witness=w.compile(), name=b"cube")


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
        with pytest.raises(HalError, match="not a loaded program"):
            h._check(compiled.lib.bx_wit_program_unload(dev))
        kept = [compiled.load(h) for _ in range(3)]  # still loaded when the ctx goes
    finally:
        h.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before
    for k in kept:
        dev, k.dev = k.dev, None  # released by bx_free: an unload of the freed handle is answered by message
        assert b"bx_wit_program_unload: not a loaded program" in compiled.lib.bx_wit_program_unload(dev)
