"""GPU: generated constraint-program kernels (include/bx_program.h, "Generated kernels"; csrc/cons_program_gen.hpp, program_gen.cpp)
— a kernel built off line from a program's description and attached to the loaded program, against the definition-level reference
of tests/cons_program_ref.py and against the interpreter on the same loaded program, word for word over the whole 4N domain; the
refusals of attach / detach by message; the lookup and square circuits proved through their generated kernels, seal for seal.

Descriptions and code objects are READ from tests/golden/consgen/ and tests/_build/consgen/ (tests/consgen_cases.py; build() compiles
them): nothing is generated or compiled here.  Sizes are those of tests/test_cons_program_gpu.py, for the same reasons: po2 1 (a
domain of 8 points: less than a wave, and a tap 3 rows back wraps more than once), 6 (one workgroup exactly), 7 (two workgroups), 9 (the
prover's smallest).  Beside the seven programs of that file runs one of 1 500 steps: longer than one function of the generated text,
so its kernel is two segments with the slot files handed from one to the other through memory."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_program_ref as ref  # noqa: E402
import consgen_cases as cases  # noqa: E402
import extreme_words  # noqa: E402

from boundless_amd.circuit import CircuitOps, encode_cell_records, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
WIDTHS = (3, 5, 8)  # of the seven programs (tests/cons_program_cases.py)


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def programs(hal):
    """name -> (reference program of the description, the library's compiled program, the same loaded on the module's ctx)"""
    out = {}
    for name in cases.SEVEN + cases.LONG:
        compiled = cases.compiled(name)
        out[name] = (cases.ref_program(cases.description(name)), compiled, compiled.load(hal))
    yield out
    for _, compiled, loaded in out.values():
        loaded.unload()
        compiled.close()


def _run(hal, loaded, po2, evals, poly_mix, mix, globals_, widths=WIDTHS):
    dom = 4 << po2
    dev = [hal.copy_from(np.ascontiguousarray(e.reshape(-1))) for e in evals]
    check = hal.alloc_elem_init(4 * dom, 0xFFFFFFFF)  # a word the kernel does not write is no field element
    hal.cons_program_eval_check(loaded, po2, check, dev[0], dev[1], dev[2], widths, poly_mix, mix, globals_)
    return check.view().reshape(4, dom).copy()


def _both(hal, loaded, name, *args):
    """the check planes from the attached kernel, then from the interpreter on the same loaded program"""
    loaded.attach_kernel(cases.kernel_path(name))
    try:
        assert loaded.kernel_attached
        gen = _run(hal, loaded, *args)
    finally:
        loaded.detach_kernel()
    assert not loaded.kernel_attached
    return gen, _run(hal, loaded, *args)


def _scalars(rng):
    return ([int(v) for v in rng.integers(0, P, 4)], [int(v) for v in rng.integers(0, P, 4)], [int(v) for v in rng.integers(0, P, 2)])


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} check words differ, first at (plane, point) {tuple(bad[0])}"


@pytest.mark.parametrize("po2", [1, 6, 7, 9])
@pytest.mark.parametrize("name", cases.SEVEN + cases.LONG)
def test_the_generated_kernel_is_the_reference_and_the_interpreter_on_every_domain_point(hal, programs, name, po2):
    prog, _, loaded = programs[name]
    dom = 4 << po2
    rng = np.random.default_rng([po2, len(prog.steps)])
    evals = [rng.integers(0, P, (w, dom), dtype=np.uint32) for w in WIDTHS]
    pm, mix, g = _scalars(rng)
    want = ref.check_planes(prog, po2, evals, pm, mix, g[:prog.n_globals])
    assert np.count_nonzero(want) >= 0.99 * want.size, "degenerate reference: a kernel that writes zeros could pass"
    gen, interp = _both(hal, loaded, name, po2, evals, pm, mix, g[:prog.n_globals])
    _same(gen, want, "generated kernel against the reference")
    _same(gen, interp, "generated kernel against the interpreter")


@pytest.mark.parametrize("pattern", ["zero", "all_pm1", "alt_half"])
def test_the_generated_kernel_is_the_reference_on_extreme_columns(hal, programs, pattern):
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
            gen, interp = _both(hal, loaded, name, po2, evals, pm, mix, g[:prog.n_globals])
            _same(gen, want, f"{name}: generated kernel against the reference")
            _same(gen, interp, f"{name}: generated kernel against the interpreter")


# ---- refusals: none of them reaches a launch, and HIP is never handed bytes that are not a code object ----
def test_attach_and_detach_refuse_by_message_and_the_interpreter_goes_on(hal, programs):
    prog, _, loaded = programs["one_constraint"]
    po2, dom = 6, 4 << 6
    rng = np.random.default_rng(6)
    evals = [rng.integers(0, P, (w, dom), dtype=np.uint32) for w in WIDTHS]
    pm, mix, _ = _scalars(rng)
    want = ref.check_planes(prog, po2, evals, pm, mix, [])

    def still_good():
        assert not loaded.kernel_attached
        _same(_run(hal, loaded, po2, evals, pm, mix, []), want, "the interpreter after a refusal")

    for junk in (b"", b"\x7fEL", b"not a code object at all, but long enough to hold a magic", bytes(64)):
        with pytest.raises(HalError, match="neither an ELF code object nor a clang offload bundle"):
            loaded.attach_kernel(junk)
        still_good()
    with pytest.raises(HalError, match="no kernel bx_cp_eval"):
        loaded.attach_kernel(cases.kernel_path("no_symbols"))
    still_good()
    with pytest.raises(HalError, match="built for ABI 2, this library launches ABI 1"):
        loaded.attach_kernel(cases.kernel_path("other_abi"))
    still_good()
    with pytest.raises(HalError, match="digest mismatch"):
        loaded.attach_kernel(cases.kernel_path("every_form"))
    still_good()
    with pytest.raises(HalError, match="no kernel is attached"):
        loaded.detach_kernel()
    still_good()
    with open(cases.kernel_path("one_constraint"), "rb") as f:
        image = f.read()
    loaded.attach_kernel(image)  # bytes as well as a path
    with pytest.raises(HalError, match="already attached"):
        loaded.attach_kernel(image)
    assert loaded.kernel_attached
    _same(_run(hal, loaded, po2, evals, pm, mix, []), want, "the attached kernel after a refused second attach")
    loaded.detach_kernel()
    with pytest.raises(HalError, match="no kernel is attached"):
        loaded.detach_kernel()
    still_good()


def test_unload_and_bx_free_detach_what_is_still_attached():
    compiled = cases.compiled("every_form")
    h = HipHal(0)
    try:
        a = compiled.load(h)
        a.attach_kernel(cases.kernel_path("every_form"))
        a.unload()  # with its kernel
        kept = compiled.load(h)
        kept.attach_kernel(cases.kernel_path("every_form"))
    finally:
        h.close()  # bx_free with a kernel still attached
    kept.dev = None  # released by bx_free
    compiled.close()


# ---- the lookup circuit through its generated kernel ----
@pytest.mark.parametrize("po2,widths", [(9, (3, 10, 20)), (12, (3, 10, 20)), (9, (16, 256, 64))])
def test_the_lookup_program_with_its_kernel_proves_the_built_in_circuits_seal_word_for_word(po2, widths):
    name = "lookup_%d_%d_%d_%d" % ((po2,) + widths)
    prog = cases.compiled(name)
    ops = CircuitOps.from_program(prog, lookup_circuit(), kernel=cases.kernel_path(name))
    builtin = HipProverServer(0, po2=po2, widths=widths, circuit="lookup")
    composite = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        B = 1 << min(15, po2 - 1)
        records = [(0, 0, 7 + B * 9), (1, 0, 7), (2, 0, 9)]  # consistent in-range records for (v_0, lo_0, hi_0) at row 0
        for seg in (Segment(index=0, po2=po2, seed=500 + po2), Segment(index=1, po2=po2, seed=600 + po2, payload=encode_cell_records(records))):
            a, b = builtin.prove_segment(seg), composite.prove_segment(seg)
            assert np.array_equal(a.seal, b.seal), f"first differing seal word: {int(np.argmax(a.seal != b.seal))}"
            verify_seal(b.seal, circuit=ops)
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


def test_the_composite_table_refuses_another_programs_kernel_at_create():
    prog = cases.compiled("lookup_9_3_10_20")
    ops = CircuitOps.from_program(prog, lookup_circuit(), kernel=cases.kernel_path("lookup_9_16_256_64"))
    with pytest.raises(HalError, match="digest mismatch"):
        HipProverServer(0, po2=9, widths=(3, 10, 20), circuit=ops)


# ---- the square circuit: eval_check from its generated kernel, the other stages in numpy ----
def _square(po2, widths, seed, from_program):
    from boundless_amd.hal import load_library
    from test_circuit_plugin_gpu import SquareCircuit

    circ = SquareCircuit(load_library())
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, b"square-plus-back")
    if from_program:
        ops = CircuitOps.from_program(cases.compiled("square"), ops, kernel=cases.kernel_path("square"))
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx, circ
    finally:
        srv.close()


def test_the_square_program_with_its_kernel_proves_the_numpy_circuits_seal():
    po2, widths = 10, (2, 3, 2)
    want, numpy_ops, numpy_ctx, _ = _square(po2, widths, 77, from_program=False)
    got, ops, vctx, circ = _square(po2, widths, 77, from_program=True)
    assert circ.calls == ["code_group", "witgen", "accumulate"]  # eval_check did not come from numpy
    assert np.array_equal(got.seal, want.seal)
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
