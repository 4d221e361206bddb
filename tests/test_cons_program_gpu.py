"""GPU: constraint programs (include/bx_program.h, csrc/cons_program.hip) — the interpreting kernel against the definition-level
reference of tests/cons_program_ref.py, word for word over the whole 4N domain; the lookup circuit written as a program against
the built-in lookup circuit, seal for seal; the square circuit of tests/test_circuit_plugin_gpu.py with eval_check and constraints_at
from its program against the all-numpy original.

Sizes are the smallest at which each thing can break: po2 1 (a domain of 8 points: less than a wave, and a tap 3 rows back wraps
more than once), 6 (one workgroup exactly), 7 (two workgroups), 9 (the prover's smallest); programs of one constraint, about 40 and
about 700 steps, every opcode form, the two slot files at their limits (the wide one needs more than 64 KiB of LDS), and both at their limits
together (the 128 KiB ceiling)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_program_ref as ref  # noqa: E402
import extreme_words  # noqa: E402
from cons_program_cases import PROGRAMS, WIDTHS, compile_ref  # noqa: E402

from boundless_amd.circuit import CircuitOps, encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def programs(hal):
    """name -> (reference program, the library's compiled program, the same loaded on the module's ctx): built once"""
    out = {}
    for name, make in PROGRAMS.items():
        prog = make()
        compiled = compile_ref(prog)
        out[name] = (prog, compiled, compiled.load(hal))
    yield out
    for _, compiled, loaded in out.values():
        loaded.unload()
        compiled.close()


def _run(hal, loaded, po2, evals, poly_mix, mix, globals_, widths=WIDTHS):
    dom = 4 << po2
    dev = [hal.copy_from(np.ascontiguousarray(e.reshape(-1))) for e in evals]
    check = hal.alloc_elem_init(4 * dom, 0xFFFFFFFF)  # a word the kernel does not write is no field element
    hal.cons_program_eval_check(loaded, po2, check, dev[0], dev[1], dev[2], widths, poly_mix, mix, globals_)
    return check.view().reshape(4, dom)


def _scalars(rng):
    return ([int(v) for v in rng.integers(0, P, 4)], [int(v) for v in rng.integers(0, P, 4)], [int(v) for v in rng.integers(0, P, 2)])


@pytest.mark.parametrize("po2", [1, 6, 7, 9])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_eval_check_is_the_reference_on_every_domain_point(hal, programs, name, po2):
    prog, _, loaded = programs[name]
    dom = 4 << po2
    rng = np.random.default_rng([po2, len(prog.steps)])
    evals = [rng.integers(0, P, (w, dom), dtype=np.uint32) for w in WIDTHS]
    pm, mix, g = _scalars(rng)
    want = ref.check_planes(prog, po2, evals, pm, mix, g[:prog.n_globals])
    assert np.count_nonzero(want) >= 0.99 * want.size, "degenerate reference: a kernel that writes zeros could pass"
    got = _run(hal, loaded, po2, evals, pm, mix, g[:prog.n_globals])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} check words differ, first at (plane, point) {tuple(bad[0])}: {loaded.program.info}"


@pytest.mark.parametrize("pattern", ["zero", "all_pm1", "alt_half"])
def test_eval_check_is_the_reference_on_extreme_columns(hal, programs, pattern):
    po2 = 7
    dom = 4 << po2
    if pattern == "zero":
        evals = [np.zeros((w, dom), np.uint32) for w in WIDTHS]
    else:
        evals = [extreme_words.pattern(pattern, (w, dom), seed=q) for q, w in enumerate(WIDTHS)]
    half = extreme_words.HALF
    for name, (prog, _, loaded) in programs.items():
        for pm, mix, g in (([half + 1] * 4, [0, half, half + 1, half], [P - 1, half]), ([P - 1] * 4, [P - 1] * 4, [0, P - 1])):
            want = ref.check_planes(prog, po2, evals, pm, mix, g[:prog.n_globals])
            got = _run(hal, loaded, po2, evals, pm, mix, g[:prog.n_globals])
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{name}: {len(bad)} check words differ, first at (plane, point) {tuple(bad[0])}"


# ---- the lookup circuit as a program ----
def _lookup_pair(po2, widths):
    prog = compile_ref(ref.lookup_program(po2, widths))
    ops = CircuitOps.from_program(prog, lookup_circuit())
    return ops, HipProverServer(0, po2=po2, widths=widths, circuit="lookup"), HipProverServer(0, po2=po2, widths=widths, circuit=ops)


@pytest.mark.parametrize("po2,widths,V", [(9, (3, 10, 20), 2), (12, (3, 10, 20), 2), (9, (16, 256, 64), 7)])
def test_the_lookup_program_proves_the_built_in_circuits_seal_word_for_word(po2, widths, V):
    ops, builtin, composite = _lookup_pair(po2, widths)
    try:
        B = 1 << min(15, po2 - 1)
        records = [(0, 0, 7 + B * 9), (1, 0, 7), (2, 0, 9)]  # consistent in-range records for (v_0, lo_0, hi_0) at row 0
        for seg in (Segment(index=0, po2=po2, seed=500 + po2), Segment(index=1, po2=po2, seed=600 + po2, payload=encode_cell_records(records))):
            a, b = builtin.prove_segment(seg), composite.prove_segment(seg)
            assert np.array_equal(a.seal, b.seal), f"first differing seal word: {int(np.argmax(a.seal != b.seal))}"
            verify_seal(b.seal, circuit=ops)  # through the program's constraints_at (the code root through the base's check_code)
            verify_seal(b.seal, circuit="lookup")
        # a limb = B with v matched: every local constraint holds, the running sums do not close
        bad = Segment(index=2, po2=po2, seed=700, payload=encode_cell_records([(1, 50, B), (0, 50, B + B * 3), (2, 50, 3)]))
        a, b = builtin.prove_segment(bad), composite.prove_segment(bad)
        assert np.array_equal(a.seal, b.seal)
        for circuit in (ops, "lookup"):
            with pytest.raises(HalError, match="constraint identity"):
                verify_seal(b.seal, circuit=circuit)
    finally:
        builtin.close()
        composite.close()


def test_the_composite_table_checks_the_program_against_the_shape():
    prog = compile_ref(ref.lookup_program(9, (16, 256, 64)))  # names data columns up to 21 and accum columns up to 59
    ops = CircuitOps.from_program(prog, lookup_circuit())
    with pytest.raises(HalError, match="the program taps column 21 of group 1, the shape has 10 columns there"):
        HipProverServer(0, po2=9, widths=(3, 10, 20), circuit=ops)
    square = CircuitOps.from_program(compile_ref(ref.square_program()), lookup_circuit())  # one global against the lookup circuit's two
    with pytest.raises(HalError, match="the program has 1 globals, the base circuit 2"):
        HipProverServer(0, po2=9, widths=(3, 10, 20), circuit=square)


# ---- the square circuit: eval_check and constraints_at from its program, the other stages in numpy ----
def _square(circ_obj, po2, widths, seed, from_program):
    from boundless_amd.hal import load_library
    from test_circuit_plugin_gpu import SquareCircuit

    circ = SquareCircuit(load_library(), **circ_obj)
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, b"square-plus-back")
    if from_program:
        ops = CircuitOps.from_program(compile_ref(ref.square_program()), ops)
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_the_square_program_proves_the_numpy_circuits_seal():
    po2, widths = 10, (2, 3, 2)
    want, numpy_ops, numpy_ctx, _ = _square({}, po2, widths, 77, from_program=False)
    got, ops, vctx, circ = _square({}, po2, widths, 77, from_program=True)
    assert circ.calls == ["code_group", "witgen", "accumulate"]  # eval_check did not come from numpy
    assert np.array_equal(got.seal, want.seal)
    verify_seal(got.seal, circuit=ops, ctx=vctx)  # the program's constraints_at
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)  # the numpy one
    for cheat in ({"cheat_row": 123}, {"claim": 12345}):
        receipt, ops, vctx, _ = _square(cheat, po2, widths, 5, from_program=True)
        with pytest.raises(HalError, match="constraint identity"):
            verify_seal(receipt.seal, circuit=ops, ctx=vctx)


# ---- the device entry point's refusals, and what a ctx holds ----
def test_eval_check_refuses_what_does_not_fit_by_message(hal, programs):
    prog, compiled, loaded = programs["every_form"]  # taps (0, 0), (1, 4), (2, 7); two globals
    po2, dom = 6, 4 << 6
    bufs = {w: hal.alloc(dom * w) for w in (2, 3, 4, 5, 7, 8)}
    check = hal.alloc(4 * dom)
    pm = mix = [1, 2, 3, 4]

    def call(po2=po2, check=check, widths=WIDTHS, lens=None, g=(5, 6), on=hal, what=loaded):
        lens = lens or widths
        on.cons_program_eval_check(what, po2, check, bufs[lens[0]], bufs[lens[1]], bufs[lens[2]], widths, pm, mix, list(g))

    call()
    with pytest.raises(HalError, match="buffer size mismatch"):
        call(check=hal.alloc(4 * dom - 1))
    with pytest.raises(HalError, match="buffer size mismatch"):
        call(lens=(3, 5, 7))
    with pytest.raises(HalError, match="buffer size mismatch"):
        call(po2=7)
    with pytest.raises(HalError, match="taps column 7 of group 2, which has 7 columns"):
        call(widths=(3, 5, 7))
    with pytest.raises(HalError, match="taps column 4 of group 1, which has 4 columns"):
        call(widths=(3, 4, 8))
    with pytest.raises(HalError, match="1 globals given, the program needs 2"):
        call(g=(5,))
    for bad in (0, 25):
        with pytest.raises(HalError, match=r"po2 must be in \[1, 24\]"):
            call(po2=bad)
    other = HipHal(0)
    try:
        with pytest.raises(HalError, match="loaded on another ctx"):
            call(on=other)
    finally:
        other.close()
    call()  # still good after the refusals


def test_load_and_unload_return_their_memory_and_bx_free_releases_what_is_left():
    import torch

    compiled = compile_ref(PROGRAMS["steps_700"]())
    HipHal(0).close()  # the first ctx of a process loads the code objects: not part of what is measured
    h = HipHal(0)
    try:
        compiled.load(h).unload()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        for _ in range(10):
            loaded = compiled.load(h)
            loaded.unload()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before
        twice = compiled.load(h)
        dev = twice.dev
        twice.unload()
        with pytest.raises(HalError, match="not a loaded program"):
            h._check(compiled.lib.bx_cons_program_unload(dev))
        kept = [compiled.load(h) for _ in range(3)]  # still loaded when the ctx goes
    finally:
        h.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before
    for k in kept:
        dev, k.dev = k.dev, None  # released by bx_free: an unload of the freed handle is answered by message
        assert b"bx_cons_program_unload: not a loaded program" in compiled.lib.bx_cons_program_unload(dev)
