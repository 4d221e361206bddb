"""CPU: trace layouts (include/bx_layout.h) — the create rules, the two host fills and the control IDs as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/trace_layout_check.cpp; nothing is loaded into Python under a sanitizer), the
Python builder and its host fills against the definition-level reference of tests/trace_layout_ref.py on eight layouts, the JSON form
of boundless_amd.consgen.layout_of, the header as pedantic C99 with its entry points exported, and — where hipcc is on PATH — the
compiler's resource report of the two new kernels beside the unchanged figures of the witness kernels.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_layout_ref as ref  # noqa: E402

from boundless_amd.circuit import TraceLayout, encode_records  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_create_rules_host_fills_and_control_ids_under_sanitizers(tmp_path):
    exe = str(tmp_path / "trace_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "trace_layout_check.cpp"),
                        os.path.join(CSRC, "trace_layout_host.cpp"), os.path.join(CSRC, "control_id.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trace_layout_check ok" in r.stdout and "runtime error" not in r.stderr


def test_the_header_is_pedantic_c99_and_its_entry_points_are_exported():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_layout.h"\nint main(void){bx_trace_layout_desc d; bx_layout_field f; (void)d; (void)f; '
                             "return BX_LAYOUT_WORD - 6 + BX_LAYOUT_MAX_STRIDE - 128;}\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from boundless_amd import hal

    lib = hal.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bx_layout.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bx_trace_layout_[a-z0-9_]+)\s*\(", text)))
    assert names == ["bx_trace_layout_code", "bx_trace_layout_code_host", "bx_trace_layout_control_id_host_hashfn", "bx_trace_layout_create", "bx_trace_layout_data_host",
                     "bx_trace_layout_destroy", "bx_trace_layout_info_get", "bx_trace_layout_load", "bx_trace_layout_ops", "bx_trace_layout_place", "bx_trace_layout_unload"]
    for n in names:
        assert getattr(lib, n) is not None


# ---- the builder and the host fills against the reference ----
LAYOUTS = {
    "every_kind": lambda: (ref.every_kind(), 4),
    "every_kind_no_noise": lambda: (ref.every_kind(noise_rows=0, stride=1), 3),
    "lookup_code": lambda: (ref.lookup_code(6), 1),
    "synthetic_code": lambda: (ref.synthetic_code(5), 2),
    "no_fields": lambda: (ref.no_fields(stride=33), 3),
    "every_column_65": lambda: (ref.every_column(65, 31), 65),
    "every_column_300_no_noise": lambda: (ref.every_column(300, 128, noise_rows=0), 300),
    "one_word_three_fields": lambda: (ref.one_word_three_fields(), 5),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_builders_host_fills_are_the_reference(name):
    """fails on a library without trace layouts: circuit has no TraceLayout"""
    layout, w_data = LAYOUTS[name]()
    compiled = ref.compile_ref(layout)
    try:
        info = compiled.info()
        assert info == {"n_code": len(layout.code), "n_table": len(layout.table), "n_fields": len(layout.fields), "stride": layout.stride,
                        "noise_rows": layout.noise_rows, "n_globals": layout.n_globals, "min_w_data": layout.min_w_data()}
        for po2 in (1, 3, 6, 9):
            n, act = 1 << po2, ref.active_rows(po2, layout.noise_rows)
            if any(k in (ref.LAST, ref.ACTIVE) and a >= act for k, a, _ in layout.code):
                with pytest.raises(HalError, match="bx_trace_layout_code_host: code column"):
                    compiled.code_host(po2)
            else:
                want = ref.code_group(layout, po2)
                got = compiled.code_host(po2)
                bad = np.argwhere(got != want)
                assert bad.size == 0, f"po2 {po2}: code cell {tuple(bad[0])} is {int(got[tuple(bad[0])])}, the reference has {int(want[tuple(bad[0])])}"
            for count in sorted({0, 1, act - 1, act}):
                for kind, noise_seed in (("random", None), ("ones", 0x0123456789ABCDEF)):
                    seg = ref.segment_bytes(po2, 77 + po2, ref.records(kind, count, layout.stride, seed=po2))
                    want = ref.data_group(layout, po2, seg, w_data, noise_seed)
                    got = compiled.data_host(po2, seg, w_data, noise_seed)
                    bad = np.argwhere(got != want)
                    assert bad.size == 0, f"po2 {po2}, R {count}, {kind}: data cell {tuple(bad[0])} is {int(got[tuple(bad[0])])}, the reference has {int(want[tuple(bad[0])])}"
                    assert int(got.max()) < P
    finally:
        compiled.close()


def test_data_host_refuses_the_two_payloads_by_message_and_writes_nothing():
    layout = ref.one_word_three_fields(stride=3)
    compiled = ref.compile_ref(layout)
    po2, w = 6, 4
    act = ref.active_rows(po2, layout.noise_rows)
    out = np.full((w, 1 << po2), ref.POISON, np.uint32)
    ragged = ref.segment_bytes(po2, 1, ref.records("random", 2, 3).tobytes() + b"\0" * 8)
    with pytest.raises(HalError, match=r"bx_trace_layout_data_host: the payload of 32 bytes is not a whole number of 12-byte records \(stride 3\)"):
        compiled.data_host(po2, ragged, w, out=out)
    with pytest.raises(ref.Refused):
        ref.data_group(layout, po2, ragged, w)
    long_one = ref.segment_bytes(po2, 1, ref.records("random", act + 1, 3))
    with pytest.raises(HalError, match=f"bx_trace_layout_data_host: the payload holds {act + 1} records, the trace has {act} active rows"):
        compiled.data_host(po2, long_one, w, out=out)
    with pytest.raises(ref.Refused):
        ref.data_group(layout, po2, long_one, w)
    with pytest.raises(HalError, match="w_data is 3, a field names data column 3"):
        compiled.data_host(po2, ref.segment_bytes(po2, 1, b""), 3, out=out[:3])
    with pytest.raises(HalError, match="the segment has po2 6, the fill was asked for po2 7"):
        compiled.data_host(7, ref.segment_bytes(po2, 1, b""), w, out=np.full((w, 128), ref.POISON, np.uint32))
    assert np.all(out == ref.POISON)
    compiled.close()


def test_the_builder_refuses_by_name_and_encode_records_is_little_endian():
    t = TraceLayout(stride=2)
    t.code_first()
    t.field(0, 2, bits=8)
    with pytest.raises(HalError, match="trace_layout: field 0: word 2 is not below the stride 2"):
        t.compile()
    t = TraceLayout(stride=2)
    with pytest.raises(HalError, match="trace_layout: n_code 0 is not in 1 .. 65535"):
        t.compile()
    t = TraceLayout()
    t.code_const(P)
    with pytest.raises(HalError, match=f"trace_layout: code column 0: CONST value {P} is not below P"):
        t.compile()
    t = TraceLayout()
    with pytest.raises(ValueError, match="power of two"):
        t.code_periodic([1, 2, 3])
    t.code_const(1 << 32)
    with pytest.raises(ValueError, match="not a 32-bit unsigned value"):
        t.compile()
    t = TraceLayout(stride=1, noise_rows=0)
    assert [t.code_first(), t.code_last(2), t.code_active(1), t.code_row(7), t.code_periodic([5, 6]), t.code_periodic([9]), t.code_word(ref.SYNTH_CODE_SEED), t.code_const(3)] == list(range(8))
    assert t.code[4:7] == [(ref.PERIODIC, 1, 0), (ref.PERIODIC, 0, 2), (ref.WORD, 0x524F4C21, 0x434F4E54)] and t.table == [5, 6, 9]
    assert encode_records([[1, 0x04030201], [0xFFFFFFFF, 2]]) == bytes([1, 0, 0, 0, 1, 2, 3, 4, 255, 255, 255, 255, 2, 0, 0, 0])
    assert encode_records(np.zeros((0, 5), np.uint32)) == b""
    with pytest.raises(ValueError):
        encode_records([1, 2, 3])
    with pytest.raises(ValueError):
        encode_records([[1 << 32]])


def test_layout_of_round_trips_a_description():
    import json

    from boundless_amd.consgen import layout_of

    layout = ref.every_kind(noise_rows=7, stride=5)
    layout.n_globals = 2
    desc = json.loads(json.dumps(ref.to_description(layout)))
    a, b = layout_of(desc), ref.compile_ref(layout)
    assert a.info() == b.info() and a.info()["n_globals"] == 2
    seg = ref.segment_bytes(6, 5, ref.records("random", 9, 5))
    assert np.array_equal(a.code_host(6), b.code_host(6)) and np.array_equal(a.code_host(6), ref.code_group(layout, 6))
    assert np.array_equal(a.data_host(6, seg, 3), ref.data_group(layout, 6, seg, 3))
    numbered = {"layout": {"stride": 1, "code": [[1], [2, 3], ["word", 9]]}}  # kinds by number, operands left out, the defaults
    c = layout_of(numbered)
    assert c.info() == {"n_code": 3, "n_table": 0, "n_fields": 0, "stride": 1, "noise_rows": 1994, "n_globals": 0, "min_w_data": 0}
    for x in (a, b, c):
        x.close()


def test_control_id_host_is_the_built_in_circuits_for_their_code_groups():
    """at po2 9 the lookup circuit's table ends at B = 256"""
    from boundless_amd import hal

    lib = hal.load_library()
    import ctypes as C

    want = (C.c_uint32 * 8)()
    lk, sy = ref.compile_ref(ref.lookup_code(4, po2=9)), ref.compile_ref(ref.synthetic_code(4))
    lib.bx_lookup_control_id_host_hashfn.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]
    lib.bx_lookup_control_id_host_hashfn.restype = C.c_char_p
    lib.bx_synthetic_control_id_host_hashfn.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]
    lib.bx_synthetic_control_id_host_hashfn.restype = C.c_char_p
    for suite in ("poseidon2", "sha-256"):
        assert not lib.bx_lookup_control_id_host_hashfn(9, 4, suite.encode(), want)
        assert list(lk.control_id_host(9, suite)) == list(want), suite
        assert not lib.bx_synthetic_control_id_host_hashfn(9, 4, suite.encode(), want)
        assert list(sy.control_id_host(9, suite)) == list(want), suite
    assert list(sy.control_id_host(9)) != list(lk.control_id_host(9))
    with pytest.raises(HalError, match=r"po2 in \[9, 24\]"):
        sy.control_id_host(8)
    lk.close()
    sy.close()


# ---- the compiler's resource report ----
def _report(src, tmp_path):
    from boundless_amd import build

    r = subprocess.run(["hipcc", "-x", "hip"] + build.FLAGS + [build.cuid_flag(src), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                               "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".co"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip().split(": ")[-1], m.group(2).strip()
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name:
            out[name][key] = int(val) if val.isdigit() else val
    return out


def _figures(report, kernel):
    rep = [v for k, v in report.items() if kernel in k]
    assert len(rep) == 1, (kernel, sorted(report))
    return (rep[0]["VGPRs"], rep[0]["TotalSGPRs"], rep[0]["LDS Size [bytes/block]"], rep[0]["ScratchSize [bytes/lane]"], rep[0]["SGPRs Spill"], rep[0]["VGPRs Spill"])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_layout_kernels_use_no_scratch_and_the_witness_kernels_are_unchanged(tmp_path):
    report = _report("trace_layout.hip", tmp_path)
    assert sorted(k for k in report if "layout_" in k and "kernel" in k) == sorted(report) and len(report) == 2, sorted(report)
    for kernel in ("layout_code_kernel", "layout_place_kernel"):
        vgprs, sgprs, lds, scratch, sspill, vspill = _figures(report, kernel)
        assert (scratch, sspill, vspill) == (0, 0, 0), (kernel, report)
        assert lds == 0, kernel  # the place tile is dynamic LDS, sized per stride at launch
        assert vgprs <= 64 and sgprs <= 80, (kernel, vgprs, sgprs)  # eight waves per SIMD, eight 256-lane workgroups per CU
    # (VGPRs, SGPRs, static LDS, scratch, SGPR spills, VGPR spills) of the commit before trace layouts
    parent = {"wit_program.hip": {"wit_program_kernel": (10, 37, 0, 0, 0, 0)},
              "wit_sort.hip": {"wit_sort_pack_kernel": (9, 18, 0, 0, 0, 0), "wit_sort_hist_kernel": (14, 19, 1024, 0, 0, 0), "wit_sort_sums_kernel": (12, 14, 16, 0, 0, 0),
                               "wit_sort_scan_kernel": (24, 26, 16, 0, 0, 0), "wit_sort_scatter_kernel": (18, 31, 5120, 0, 0, 0), "wit_sort_gather_kernel": (4, 18, 0, 0, 0, 0)}}
    for src, kernels in parent.items():
        report = _report(src, tmp_path)
        for kernel, want in kernels.items():
            assert _figures(report, kernel) == want, (src, kernel)
