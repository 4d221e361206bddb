"""CPU: generated witness-program kernels (include/bx_program.h, "Generated witness kernels") without a GPU.

* the emitter (csrc/cons_program_emit.cpp) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
  (tests/witgen_check.cpp): sizes, no write past `cap`, byte-equal emits, what the digest depends on and what it does not, the
  hand-corrupted streams, and the constraint emitter's refusal of a store;
* the generated text ITSELF, run on the CPU: for every fixture under tests/golden/witgen/ the text is compiled by g++ with the host
  wrapper of csrc/wit_program_gen.hpp into a second stand-alone program (tests/witgen_host_main.cpp, ASan + UBSan, linked with
  csrc/program_compile.cpp, csrc/cons_program_host.cpp) that derives the data columns at po2 1, 3 and 6 from random, all-0, all-(P - 1) and alternating columns
  with the derived ones poisoned; Python compares them word for word with tests/wit_program_ref.py, the program itself compares
  them with bx_wit_program_run_host;
* where hipcc is on PATH: every fixture compiles for gfx950, the one-function ones without scratch and without LDS, and
  derive_64_4_16_16 as three segments;
* the committed fixtures are what tools/witgen_fixtures.py writes.
Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wit_program_ref as ref  # noqa: E402
import witgen_cases as cases  # noqa: E402

CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
INC = os.path.join(ROOT, "include")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas",  # "#pragma unroll" of the shared arithmetic headers is hipcc's
       f"-I{CSRC}", f"-I{INC}"]
P = ref.P
PATTERNS = ("random", "zero", "all_pm1", "alternating")


def test_emitter_under_sanitizers(tmp_path):
    exe = str(tmp_path / "witgen_check")
    r = subprocess.run(SAN + [os.path.join(ROOT, "tests", "witgen_check.cpp"), os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"),
                              os.path.join(CSRC, "cons_program_emit.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the emitter compiles without a warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "witgen_check ok" in r.stdout


def _columns(prog, po2, widths, pattern, seed):
    n = 1 << po2
    rng = np.random.default_rng([seed, po2, PATTERNS.index(pattern)])
    if pattern == "random":
        code, data = (rng.integers(0, P, (w, n), dtype=np.uint32) for w in widths)
    elif pattern == "alternating":
        code, data = (np.broadcast_to(np.where(np.arange(n) & 1, P - 1, 0).astype(np.uint32), (w, n)).copy() for w in widths)
    else:
        code, data = (np.full((w, n), 0 if pattern == "zero" else P - 1, np.uint32) for w in widths)
    data[prog.derived()] = P - 1  # poison: a cell the body does not write shows
    return code, data


def _case_words(desc, po2, widths, code, data):
    head = [po2, widths[0], widths[1], len(desc["steps"]), len(desc["taps"]), len(desc["cells"])]
    flat = [v for s in desc["steps"] for v in s] + [v for t in desc["taps"] for v in t] + [v for g in desc["cells"] for v in g]
    return np.concatenate([np.array(head + flat, np.uint32), code.reshape(-1), data.reshape(-1)])


def _circuit_widths(name):
    return (2, 3) if name in cases.CIRCUITS else cases.widths(name)


@pytest.mark.parametrize("name", cases.NAMES)
def test_generated_text_run_on_the_cpu_is_the_reference_and_the_host_executor(tmp_path, name):
    desc = cases.description(name)
    prog = cases.compiled(name)
    try:
        text = prog.emit_hip()
        assert prog.digest()[:8] == "".join(f"{b:02x}" for b in bytes.fromhex(text.split("BX_WP_DIGEST_WORDS 0x")[1][:8])[::-1])
    finally:
        prog.close()
    (tmp_path / "bx_wp_generated.inc").write_text(text)
    exe = str(tmp_path / "witgen_host")
    # -g0: a body of hundreds of statements is one function, and gcc's variable tracking gives up on it with a note
    r = subprocess.run(SAN + ["-g0", f"-I{tmp_path}", os.path.join(ROOT, "tests", "witgen_host_main.cpp"), os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"),
                              os.path.join(CSRC, "cons_program_emit.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the generated text and its frame compile without a warning
    rp = cases.ref_program(desc)
    widths = _circuit_widths(name)
    free = [c for c in range(widths[1]) if c not in rp.derived()]
    runs, argv = [], [exe]
    for po2 in (1, 3, 6):
        for pattern in PATTERNS:
            code, data = _columns(rp, po2, widths, pattern, len(desc["steps"]))
            case, out = str(tmp_path / f"case_{po2}_{pattern}.bin"), str(tmp_path / f"data_{po2}_{pattern}.bin")
            _case_words(desc, po2, widths, code, data).astype("<u4").tofile(case)
            runs.append((po2, pattern, code, data, out))
            argv += [case, out]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"witgen_host ok: {len(runs)} cases" in r.stdout
    for po2, pattern, code, data, out in runs:
        want = ref.evaluate(rp, po2, code, data)
        got = np.fromfile(out, "<u4").reshape(widths[1], 1 << po2)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"po2 {po2}, {pattern}: {len(bad)} of {want.size} data words differ from the reference, first at (column, row) {tuple(bad[0])}"
        assert np.array_equal(got[free], data[free]), f"po2 {po2}, {pattern}: a free column was written"
        if pattern == "random":
            assert not np.any(want[rp.derived()] == P - 1), "degenerate reference: a body that writes nothing could pass"


def test_emit_is_a_pure_function_of_the_description_and_the_digest_tells_programs_apart():
    a, b = cases.compiled("every_form"), cases.compiled("every_form")
    try:
        assert a.emit_hip() == b.emit_hip() and a.digest() == b.digest()
        assert '#include "wit_program_gen.hpp"' in a.emit_hip() and "cons_program_gen.hpp" not in a.emit_hip()
    finally:
        a.close(), b.close()
    digests = {}
    for name in cases.NAMES:
        p = cases.compiled(name)
        digests[name] = p.digest()
        p.close()
    from boundless_amd.consgen import witness_program_of

    p = witness_program_of(cases.wrong_digest_description())
    digests["wrong_digest"] = p.digest()
    p.close()
    assert len(set(digests.values())) == len(digests), digests
    # the cells are not hashed: one code object serves a program under any cell list
    d = cases.description("every_form")
    d["cells"] = [[3, 2, 0], [1, 7, 1]]
    p = witness_program_of(d)
    assert p.digest() == digests["every_form"]
    p.close()


def test_committed_fixtures_are_what_the_generators_write_now():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "witgen_fixtures.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")


@needs_hipcc
def test_every_fixture_compiles_for_gfx950_and_one_function_stays_out_of_scratch(capsys):
    cases.build()
    for name in cases.NAMES:
        m = cases.meta(name)
        with capsys.disabled():
            print(f"\n  {name}: {m['vgprs']} VGPRs, {m['sgprs']} SGPRs, scratch {m['scratch_bytes']} B, {m['occupancy_waves_per_simd']} waves/SIMD, "
                  f"{m['instructions']} instructions, hipcc {m['hipcc_seconds']} s", end="")
        assert m["lds_bytes"] == 0 and isinstance(m["vgprs"], int) and m["vgprs"] <= 512
        p = cases.compiled(name)
        try:
            assert m["digest"] == p.digest()  # the object is this description's
            segments = p.emit_hip().count("BX_WP_SEG void bx_wp_seg")
        finally:
            p.close()
        if name in cases.ONE_FUNCTION:
            assert segments == 0 and m["scratch_bytes"] == 0, f"{name}: {m}"
        else:
            assert segments == cases.SEGMENTED[name], f"{name}: {segments} segments"
    for name in cases.REFUSALS:  # code objects too: what attach refuses about them is their symbols, not their bytes
        with open(cases.kernel_path(name), "rb") as f:
            head = f.read(24)
        assert head == b"__CLANG_OFFLOAD_BUNDLE__" or head[:4] == b"\x7fELF"
