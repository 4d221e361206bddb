"""GPU: generated witness-program kernels (include/bx_program.h, "Generated witness kernels"; csrc/wit_program_gen.hpp,
program_gen.cpp) — a kernel built off line from a witness program's description and attached to the loaded program, against the
definition-level reference of tests/wit_program_ref.py, the host executor and the interpreter on the same loaded program, word for
word over the whole data group; the refusals of attach / detach by message; release with a kernel attached; the square and cube
circuits proved with their derived columns from the attached kernel, seal for seal.

Descriptions and code objects are READ from tests/golden/witgen/ and tests/_build/witgen/ (tests/witgen_cases.py; build() compiles
them): nothing is generated or compiled here.  Sizes are those of tests/test_wit_program_gpu.py, for the same reasons: po2 1 (two
rows: less than a wave, and a tap 3 rows back wraps more than once), 6 (one wave), 7 (less than a workgroup), 8 (one workgroup
exactly), 9 (two workgroups, and the prover's smallest).  Beside the five programs of that file run the synthetic circuit's derive
stage at (T, G) = (8, 2), one function, and (64, 4): three segments, the slots handed from one to the next through memory."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_words  # noqa: E402
import synth_ref  # noqa: E402
import wit_program_ref as ref  # noqa: E402
import witgen_cases as cases  # noqa: E402
from wit_program_cases import columns  # noqa: E402

from boundless_amd.circuit import CircuitOps  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402
from boundless_amd.prover import HipProverServer, Segment, verify_seal  # noqa: E402

pytestmark = pytest.mark.gpu
P = ref.P
# Of a derived column's words under random free columns, the share that is neither 0 nor the poison P - 1: a word is a sum or a
# product of uniform words, so each is 0 or P - 1 with probability about 2 / P; over the at most 8 * 512 derived words of a case the
# reference has none (checked on the CPU for every case below).  A kernel that writes nothing leaves the poison: share 0.
LIVE_SHARE = 0.999


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def programs(hal):
    """name -> (reference program of the description, the library's compiled program, the same loaded on the module's ctx)"""
    out = {}
    for name in cases.SEVEN:
        compiled = cases.compiled(name)
        out[name] = (cases.ref_program(cases.description(name)), compiled, compiled.load(hal))
    yield out
    for _, compiled, loaded in out.values():
        loaded.unload()
        compiled.close()


_REFERENCE = {}


def _reference(name, prog, po2, pattern):
    """(code, data, want) of a case, computed once and shared: callers copy what they change"""
    key = (name, po2, pattern)
    if key not in _REFERENCE:
        code, data = columns(prog, po2, cases.widths(name), pattern, seed=len(prog.steps))
        want = ref.evaluate(prog, po2, code, data)
        for a in (code, data, want):
            a.setflags(write=False)
        _REFERENCE[key] = (code, data, want)
    return _REFERENCE[key]


def _run(hal, loaded, po2, code, data, widths):
    dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))
    loaded.run(po2, dcode, widths[0], ddata, widths[1])
    got = ddata.view().reshape(widths[1], -1).copy()
    assert np.array_equal(dcode.view(), code.reshape(-1)), "the code group was written"
    dcode.free()
    ddata.free()
    return got


def _both(hal, loaded, name, po2, code, data):
    """the data group from the attached kernel, then from the interpreter on the same loaded program"""
    widths = cases.widths(name)
    loaded.attach_kernel(cases.kernel_path(name))
    try:
        assert loaded.kernel_attached
        gen = _run(hal, loaded, po2, code, data, widths)
    finally:
        loaded.detach_kernel()
    assert not loaded.kernel_attached
    return gen, _run(hal, loaded, po2, code, data, widths)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} data words differ, first at (column, row) {tuple(bad[0])}"


def _four_ways(hal, programs, name, po2, pattern):
    prog, compiled, loaded = programs[name]
    widths = cases.widths(name)
    code, data, want = _reference(name, prog, po2, pattern)
    gen, interp = _both(hal, loaded, name, po2, code, data)
    host = data.copy()
    compiled.run_host(po2, code, widths[0], host, widths[1])
    _same(gen, want, f"{name} at po2 {po2} on {pattern}: generated kernel against the reference")
    _same(host, want, f"{name} at po2 {po2} on {pattern}: host executor against the reference")
    _same(gen, interp, f"{name} at po2 {po2} on {pattern}: generated kernel against the interpreter")
    free = [c for c in range(widths[1]) if c not in prog.derived()]
    assert np.array_equal(gen[free], data[free]), f"{name} at po2 {po2} on {pattern}: a free column was written"
    return prog, want


@pytest.mark.parametrize("po2", [1, 6, 7, 8, 9])
@pytest.mark.parametrize("name", cases.SEVEN)
def test_the_generated_kernel_is_the_reference_the_host_executor_and_the_interpreter_on_every_word(hal, programs, name, po2):
    prog, _, _ = programs[name]
    _, _, want = _reference(name, prog, po2, "random")
    derived = want[prog.derived()]
    live = np.count_nonzero((derived != 0) & (derived != P - 1)) / derived.size
    assert live >= LIVE_SHARE, f"degenerate reference ({live:.4f} of the derived words are neither 0 nor poison): a kernel that writes nothing could pass"
    _four_ways(hal, programs, name, po2, "random")


def test_the_attached_kernel_is_what_ran(hal, programs):
    name, po2 = "every_form", 7
    prog, _, loaded = programs[name]
    widths = cases.widths(name)
    code, data, want = _reference(name, prog, po2, "random")
    hal.profile_reset()
    hal.profile_enable(True)
    try:
        loaded.attach_kernel(cases.kernel_path(name))
        for _ in range(3):
            _same(_run(hal, loaded, po2, code, data, widths), want, "attached")
        hal.sync()
        report = hal.profile_report()
        assert report["wit_program_run_gen"]["calls"] == 3 and "wit_program_run" not in report, sorted(report)
        loaded.detach_kernel()
        for _ in range(2):
            _same(_run(hal, loaded, po2, code, data, widths), want, "detached")
        hal.sync()
        report = hal.profile_report()
        assert report["wit_program_run_gen"]["calls"] == 3 and report["wit_program_run"]["calls"] == 2, sorted(report)
    finally:
        hal.profile_enable(False)
        hal.profile_reset()
        if loaded.kernel_attached:
            loaded.detach_kernel()


@pytest.mark.parametrize("pattern", ["zero"] + list(extreme_words.EXTREME))
def test_the_generated_kernel_is_the_reference_on_extreme_columns(hal, programs, pattern):
    for name in cases.SEVEN:
        _four_ways(hal, programs, name, 7, pattern)


@pytest.mark.parametrize("name,T,G", [("derive_8_2_16_16", 8, 2), ("derive_64_4_16_16", 64, 4)])
def test_the_derive_programs_with_their_kernels_give_synth_refs_columns(hal, programs, name, T, G):
    po2, w = 9, 16
    _, _, loaded = programs[name]
    sh = synth_ref.Shape(po2, w, w, w, T, G)
    want, _ = synth_ref.data_columns(sh, seed=4321)
    code = synth_ref.code_columns(sh)
    data = want.copy()
    data[sh.F:] = P - 1  # the free cells are synth_ref's, the derived ones poison
    gen, interp = _both(hal, loaded, name, po2, np.ascontiguousarray(code, np.uint32), np.ascontiguousarray(data, np.uint32))
    _same(gen, want, f"{name}: generated kernel against synth_ref")
    _same(interp, want, f"{name}: interpreter against synth_ref")


# ---- refusals: none of them reaches a launch, and HIP is never handed bytes that are not a code object ----
def test_attach_and_detach_refuse_by_message_and_the_interpreter_goes_on(hal, programs):
    name, po2 = "one_set", 6
    prog, _, loaded = programs[name]
    widths = cases.widths(name)
    code, data, want = _reference(name, prog, po2, "random")
    dcode, ddata = hal.copy_from(code.reshape(-1)), hal.copy_from(data.reshape(-1))

    def still_good(attached=False):
        assert loaded.kernel_attached == attached
        assert np.array_equal(ddata.view(), data.reshape(-1)) and np.array_equal(dcode.view(), code.reshape(-1)), "a refusal touched the buffers"
        _same(_run(hal, loaded, po2, code, data, widths), want, "the next call after a refusal")

    for junk in (b"", b"\x7fEL", bytes(64)):
        with pytest.raises(HalError, match="bx_wit_program_attach_kernel: the image is neither an ELF code object nor a clang offload bundle"):
            loaded.attach_kernel(junk)
        still_good()
    import consgen_cases

    with pytest.raises(HalError, match="bx_wit_program_attach_kernel: the code object has no kernel bx_wp_run"):
        loaded.attach_kernel(consgen_cases.kernel_path("one_constraint"))
    still_good()
    with pytest.raises(HalError, match="built for ABI 2, this library launches ABI 1"):
        loaded.attach_kernel(cases.kernel_path("other_abi"))
    still_good()
    with pytest.raises(HalError, match="bx_wit_program_attach_kernel: digest mismatch"):
        loaded.attach_kernel(cases.kernel_path("wrong_digest"))
    still_good()
    with pytest.raises(HalError, match="digest mismatch"):
        loaded.attach_kernel(cases.kernel_path("every_form"))
    still_good()
    with pytest.raises(HalError, match="bx_wit_program_detach_kernel: no kernel is attached"):
        loaded.detach_kernel()
    still_good()
    with open(cases.kernel_path(name), "rb") as f:
        image = f.read()
    loaded.attach_kernel(image)  # bytes as well as a path
    try:
        with pytest.raises(HalError, match="already attached"):
            loaded.attach_kernel(image)
        still_good(attached=True)
    finally:
        loaded.detach_kernel()
    with pytest.raises(HalError, match="no kernel is attached"):
        loaded.detach_kernel()
    still_good()
    dcode.free()
    ddata.free()


def test_run_refuses_what_does_not_fit_before_any_launch_with_a_kernel_attached(hal, programs):
    name, po2 = "every_form", 6  # taps code column 2 and data column 5, sets data column 7
    prog, _, loaded = programs[name]
    W = cases.widths(name)
    n = 1 << po2
    code, data, want = _reference(name, prog, po2, "random")
    both = hal.alloc((W[0] + W[1]) * n)  # one allocation: code, then data
    dcode, ddata = both.slice(0, W[0] * n), both.slice(W[0] * n, W[1] * n)
    dcode.copy_from(code.reshape(-1))
    ddata.copy_from(data.reshape(-1))
    loaded.attach_kernel(cases.kernel_path(name))
    try:
        hal.profile_reset()
        hal.profile_enable(True)
        with pytest.raises(HalError, match=r"bx_wit_program_run: buffer size mismatch \(groups N x width\)"):
            loaded.run(po2, dcode, W[0], ddata.slice(0, W[1] * n - 1), W[1])
        with pytest.raises(HalError, match="buffer size mismatch"):
            loaded.run(po2 + 1, dcode, W[0], ddata, W[1])
        with pytest.raises(HalError, match="bx_wit_program_run: the program sets data column 7, the data group has 7 columns"):
            loaded.run(po2, dcode, W[0], ddata.slice(0, 7 * n), 7)
        with pytest.raises(HalError, match="bx_wit_program_run: the program taps column 2 of group 0, which has 2 columns"):
            loaded.run(po2, dcode.slice(0, 2 * n), 2, ddata, W[1])
        with pytest.raises(HalError, match="bx_wit_program_run: code and data overlap"):
            loaded.run(po2, both.slice(n, W[0] * n), W[0], ddata, W[1])  # the last code column is the first data column
        hal.sync()
        report = hal.profile_report()
        assert "wit_program_run_gen" not in report and "wit_program_run" not in report, sorted(report)  # no launch
        assert np.array_equal(dcode.view(), code.reshape(-1)) and np.array_equal(ddata.view(), data.reshape(-1))
        loaded.run(po2, dcode, W[0], ddata, W[1])  # still good after the refusals
        hal.sync()
        assert hal.profile_report()["wit_program_run_gen"]["calls"] == 1
        _same(ddata.view().reshape(W[1], n), want, "the attached kernel after the refusals")
    finally:
        hal.profile_enable(False)
        hal.profile_reset()
        loaded.detach_kernel()
        both.free()


def test_unload_and_bx_free_unload_what_is_still_attached():
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


# ---- through a proof: the circuits of tests/test_wit_program_gpu.py, their derived columns from the attached kernels ----
def _prove(circ, po2, widths, seed, cons=None, name=b"square-plus-back", **kw):
    circ.bind(po2, widths)
    ops = CircuitOps.from_object(circ, name)
    if cons is not None:
        ops = CircuitOps.from_program(cons, ops, **kw)
    srv = HipProverServer(0, po2=po2, widths=widths, circuit=ops)
    try:
        vctx = srv.verifier_context()
        circ.calls.clear()
        return srv.prove_segment(Segment(index=0, po2=po2, seed=seed)), ops, vctx
    finally:
        srv.close()


def test_the_square_circuit_with_its_witness_kernel_proves_the_numpy_circuits_seal():
    import cons_program_ref
    from cons_program_cases import compile_ref as compile_cons
    from test_wit_program_gpu import _square_classes, _square_witness

    from boundless_amd.hal import load_library

    SquareCircuit, FreeCellsOnly, _, _ = _square_classes()
    lib = load_library()
    po2, widths = 9, (2, 3, 2)
    want, numpy_ops, numpy_ctx = _prove(SquareCircuit(lib), po2, widths, 77)
    cons = compile_cons(cons_program_ref.square_program())
    wit = _square_witness()
    fixture = cases.compiled("square")
    assert wit.digest() == fixture.digest() == cases.meta("square")["digest"]  # the committed description is that file's program
    fixture.close()
    base = FreeCellsOnly(lib)
    got, ops, vctx = _prove(base, po2, widths, 77, cons=cons, witness=wit, witness_kernel=cases.kernel_path("square"))
    assert base.calls == ["code_group", "witgen", "accumulate"]
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
    # another program's code object, and a kernel with no witness program: refused when the prover is created
    with pytest.raises(HalError, match="bx_wit_program_attach_kernel: digest mismatch"):
        _prove(FreeCellsOnly(lib), po2, widths, 77, cons=cons, witness=wit, witness_kernel=cases.kernel_path("cube"))
    with pytest.raises(HalError, match="cons circuit: a witness kernel is set but no witness program"):
        _prove(FreeCellsOnly(lib), po2, widths, 77, cons=cons, witness_kernel=cases.kernel_path("square"))


def test_the_cube_circuit_whose_public_word_is_a_derived_cell_proves_its_numpy_twins_seal_with_its_witness_kernel():
    from oracle import oracle_lib as ol
    from test_wit_program_gpu import _cube_programs, _square_classes

    from boundless_amd.hal import load_library

    _, _, CubeCircuit, CubeFreeCellsOnly = _square_classes()
    lib = load_library()
    po2, widths = 9, (2, 3, 2)
    want, numpy_ops, numpy_ctx = _prove(CubeCircuit(lib), po2, widths, 31, name=b"cube")
    cons, wit = _cube_programs()
    assert wit.digest() == cases.meta("cube")["digest"]
    got, ops, vctx = _prove(CubeFreeCellsOnly(lib), po2, widths, 31, cons=cons, name=b"cube", witness=wit, witness_kernel=cases.kernel_path("cube"))
    assert int(got.seal[6]) != 12345 and int(ol.decode(got.seal[6:7])[0]) < P  # the base's word was overridden by data[1][0]
    assert np.array_equal(got.seal, want.seal), f"first differing seal word: {int(np.argmax(got.seal != want.seal))}"
    verify_seal(got.seal, circuit=ops, ctx=vctx)
    verify_seal(got.seal, circuit=numpy_ops, ctx=numpy_ctx)
