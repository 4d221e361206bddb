"""CPU: the NTT planner (csrc/ntt_plan.hpp, host-only) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/ntt_plan_check.cpp): every case of tests/golden/ntt_launches.json — the kernels, workgroup sizes and grids a kernel trace
recorded on the GPU (tools/ntt_launch_trace.py) — is planned again and must come out the same, and the planner's invariants hold for
every size and every tunable value in range.  Nothing is loaded into Python.  And ntt.hip launches each pass kernel from one place."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
TUNABLES = ["ntt_block_log", "ntt_tile_log", "ntt_fast", "ntt_tile_a_log", "ntt_tile_b_log", "ntt_cols_per_wg", "ntt_group_cols", "ntt_tile_b_wide"]

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ntt_launch_trace  # noqa: E402  (the case list the record was made from, and the reader of its reductions)


def golden():
    """the recorded cases: each with its parameters (ntt_launch_trace.cases()) and its launches"""
    return ntt_launch_trace.load(os.path.join(ROOT, "tests", "golden", "ntt_launches.json"))[0]


def test_planner_replays_the_recorded_launches_under_sanitizers(tmp_path):
    lines = []
    for case in golden():
        head = [str(case["tunables"][k]) for k in TUNABLES] + [case["entry"]] + [str(case[k]) for k in ("m", "count", "bits", "offset")]
        lines.append("case " + " ".join(head) + f" {len(case['launches'])}")
        lines += [f"{l['wg']} {l['grid'][0]} {l['grid'][1]} {l['kernel']}" for l in case["launches"]]
    cases_txt = tmp_path / "cases.txt"
    cases_txt.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "ntt_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", os.path.join(ROOT, "tests", "ntt_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # the planner compiles without a warning under -Wall -Wextra, and without a HIP header
    r = subprocess.run([exe, str(cases_txt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ntt_plan_check ok" in r.stdout
    assert f"{len(golden())} recorded cases replayed" in r.stdout and all(case["launches"] for case in golden())


def test_each_ntt_pass_kernel_is_launched_from_one_place():
    src = open(os.path.join(CSRC, "ntt.hip")).read()
    host = re.sub(r"//[^\n]*", "", src[src.index("// host side"):])  # the code below the kernels, without its comments
    plan = open(os.path.join(CSRC, "ntt_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", plan), "ntt_plan.hpp is host-only"
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", host)
    # each pass kernel is launched through a pointer that picks the instantiation, and is named nowhere else in the host code
    chosen = dict(re.findall(r"const (?:auto|R16Kernel) (\w+_kernel) = ([^;]+);", host))
    for pointer, kernel, mentions in (("block_kernel", "ntt_block_kernel<", 2), ("strided_kernel", "ntt_strided_kernel<", 2),
                                      ("multi_kernel", "ntt_passA_fwd12_multi_kernel<", 2), ("r16_kernel", "r16_geom_kernel(", 1)):
        assert launches.count(pointer) == 1, (pointer, launches)
        assert chosen[pointer].count(kernel) == mentions, (pointer, chosen[pointer])
        assert host.count(kernel) == mentions + (kernel == "r16_geom_kernel("), kernel  # + the dispatcher's own definition
    assert not [n for n in launches if n.startswith("ntt_")], "a pass kernel launched by name"
    assert len(re.findall(r"\bntt_r16_kernel<", host)) == 1, "ntt_r16_kernel is instantiated by the one dispatcher over NTT_GEOMS"
