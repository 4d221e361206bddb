"""CPU: generated constraint-program kernels (include/bx_program.h, "Generated kernels") without a GPU.

* the emitter (csrc/cons_program_emit.cpp) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
  (tests/consgen_check.cpp): sizes, no write past `cap`, byte-equal emits, digests;
* the generated text ITSELF, run on the CPU: for every program fixture the text is compiled by g++ with the host wrapper of
  csrc/cons_program_gen.hpp into a second stand-alone program (tests/consgen_host_main.cpp, ASan + UBSan, linked with
  csrc/program_compile.cpp, csrc/cons_program_host.cpp) that computes the four check planes over the whole domain at po2 1 and 6; Python compares them word for
  word with tests/cons_program_ref.py, the program itself compares every point with bx_cons_program_constraints_at;
* where hipcc is on PATH: every fixture compiles for gfx950, without scratch except possibly at the slot limits; a long program
  compiles;
* the committed fixtures are what tools/consgen_fixtures.py writes.
Nothing sanitized is loaded into Python."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_program_ref as ref  # noqa: E402
import consgen_cases as cases  # noqa: E402

CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
INC = os.path.join(ROOT, "include")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas",  # "#pragma unroll" of the shared arithmetic headers is hipcc's
       f"-I{CSRC}", f"-I{INC}"]
P = ref.P


def test_emitter_under_sanitizers(tmp_path):
    exe = str(tmp_path / "consgen_check")
    r = subprocess.run(SAN + [os.path.join(ROOT, "tests", "consgen_check.cpp"), os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"),
                              os.path.join(CSRC, "cons_program_emit.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the emitter compiles without a warning under -Wall -Wextra
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "consgen_check ok" in r.stdout


def _widths(desc):
    w = [1, 1, 1]
    for g, col, _ in desc["taps"]:
        w[g] = max(w[g], col + 1)
    return tuple(w)


def _case_words(desc, po2, widths, evals, pm, mix, g):
    head = [po2, *widths, desc["n_globals"], desc["ret"], len(desc["steps"]), len(desc["taps"])]
    flat = [v for s in desc["steps"] for v in s] + [v for t in desc["taps"] for v in t]
    zinv = ref.encode(ref.vanishing_inverses(po2))
    return np.concatenate([np.array(head + flat, np.uint32), np.array(g, np.uint32), np.array(mix, np.uint32), np.array(pm, np.uint32),
                           zinv.astype(np.uint32)] + [e.reshape(-1) for e in evals])


@pytest.mark.parametrize("name", cases.NAMES)
def test_generated_text_run_on_the_cpu_is_the_reference(tmp_path, name):
    desc = cases.description(name)
    prog = cases.compiled(name)
    try:
        text = prog.emit_hip()
        assert prog.digest()[:8] == "".join(f"{b:02x}" for b in bytes.fromhex(text.split("BX_CP_DIGEST_WORDS 0x")[1][:8])[::-1])
    finally:
        prog.close()
    (tmp_path / "bx_cp_generated.inc").write_text(text)
    exe = str(tmp_path / "consgen_host")
    # -g0: a body of hundreds of statements is one function, and gcc's variable tracking gives up on it with a note
    r = subprocess.run(SAN + ["-g0", f"-I{tmp_path}", os.path.join(ROOT, "tests", "consgen_host_main.cpp"), os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"),
                              os.path.join(CSRC, "cons_program_emit.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the generated text and its frame compile without a warning
    rp = cases.ref_program(desc)
    widths = _widths(desc)
    for po2 in (1, 6):
        dom = 4 << po2
        rng = np.random.default_rng([po2, len(desc["steps"])])
        evals = [rng.integers(0, P, (w, dom), dtype=np.uint32) for w in widths]
        pm, mix = [int(v) for v in rng.integers(0, P, 4)], [int(v) for v in rng.integers(0, P, 4)]
        g = [int(v) for v in rng.integers(0, P, desc["n_globals"])]
        want = ref.check_planes(rp, po2, evals, pm, mix, g)
        assert np.count_nonzero(want) >= 0.9 * want.size  # 8 points at po2 1: a zero word or two is chance, a zero plane is not
        case, out = str(tmp_path / f"case{po2}.bin"), str(tmp_path / f"planes{po2}.bin")
        _case_words(desc, po2, widths, evals, pm, mix, g).astype("<u4").tofile(case)
        r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, "<u4").reshape(4, dom)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"po2 {po2}: {len(bad)} of {want.size} check words differ, first at (plane, point) {tuple(bad[0])}"


def test_emit_is_a_pure_function_of_the_description_and_the_digest_tells_programs_apart():
    a, b = cases.compiled("every_form"), cases.compiled("every_form")
    try:
        assert a.emit_hip() == b.emit_hip() and a.digest() == b.digest()
    finally:
        a.close(), b.close()
    digests = {}
    for name in cases.NAMES:
        p = cases.compiled(name)
        digests[name] = p.digest()
        p.close()
    assert len(set(digests.values())) == len(digests), digests
    # one tap, one step, `ret` changed: another digest each time
    base = cases.description("every_form")
    seen = {digests["every_form"]}
    from boundless_amd.consgen import program_of

    for change in ("tap", "step", "ret"):
        d = json.loads(json.dumps(base))
        if change == "tap":
            d["taps"][0][2] += 1
        elif change == "step":
            k = next(i for i, s in enumerate(d["steps"]) if s[0] == ref.ADD)
            d["steps"][k][0] = ref.SUB
        else:
            d["ret"] -= 1
        p = program_of(d)
        seen.add(p.digest())
        p.close()
    assert len(seen) == 4


def test_committed_fixtures_are_what_the_generators_write_now():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "consgen_fixtures.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")


@needs_hipcc
def test_every_fixture_compiles_for_gfx950_and_stays_out_of_scratch(capsys):
    cases.build()
    for name in cases.NAMES:
        m = cases.meta(name)
        with capsys.disabled():
            print(f"\n  {name}: {m['vgprs']} VGPRs, {m['sgprs']} SGPRs, scratch {m['scratch_bytes']} B, {m['occupancy_waves_per_simd']} waves/SIMD, "
                  f"{m['instructions']} instructions, hipcc {m['hipcc_seconds']} s", end="")
        assert m["lds_bytes"] == 0 and isinstance(m["vgprs"], int) and m["vgprs"] <= 512
        p = cases.compiled(name)
        assert m["digest"] == p.digest()  # the object is this description's
        p.close()
        if name in cases.NO_SCRATCH:
            assert m["scratch_bytes"] == 0, f"{name}: {m}"
    for name in cases.REFUSALS:  # code objects too: what attach refuses about them is their symbols, not their bytes
        with open(cases.kernel_path(name), "rb") as f:
            head = f.read(24)
        assert head == b"__CLANG_OFFLOAD_BUNDLE__" or head[:4] == b"\x7fELF"


@needs_hipcc
def test_a_program_of_8000_steps_compiles(tmp_path, capsys):
    from boundless_amd import consgen

    prog = ref.random_program(8000, 8000, (3, 5, 8), nesting=2, ext_share=0.25, pressure=14, n_taps=30)
    desc = {"n_globals": prog.n_globals, "ret": prog.ret, "taps": [list(map(int, t)) for t in prog.taps], "steps": [list(map(int, s)) for s in prog.steps]}
    t0 = time.time()
    m = consgen.compile_program(desc, str(tmp_path / "long.hsaco"))
    with capsys.disabled():
        print(f"\n  {m['steps']} steps: hipcc {m['hipcc_seconds']} s (all {time.time() - t0:.1f} s), {m['vgprs']} VGPRs, scratch {m['scratch_bytes']} B", end="")
    assert m["steps"] >= 8000 and os.path.getsize(str(tmp_path / "long.hsaco")) > 0
