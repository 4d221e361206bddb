"""CPU: a witness program's sorted columns (include/bx_program.h, "sorted columns") — create's refusals by name, what a sort list
leaves alone (info, digest, generated text), the host executor against the definition-level reference of tests/wit_sort_ref.py, the
compiler and host executor as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/wit_sort_check.cpp; nothing is loaded into Python under a sanitizer), consgen's pass-through, and the compiler's resource
report of the new kernels and of the kernels beside them.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wit_program_ref as ref  # noqa: E402
import wit_sort_ref as sref  # noqa: E402
from test_wit_count_cpu import _report  # noqa: E402
from wit_program_cases import compile_ref as compile_plain  # noqa: E402

from boundless_amd import circuit  # noqa: E402
from boundless_amd.circuit import WitnessProgram  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boundless_amd", "csrc")
P = ref.P


def test_the_header_is_pedantic_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){bx_wit_sort s; s.rows = BX_WIT_MAX_SORTS + BX_WIT_MAX_SORT_COLS + BX_WIT_MAX_SORT_KEYS + '
                             'BX_WIT_MAX_SORT_BITS; (void)s; return bx_wit_program_sorts(0) != 0;}\n', capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_compiler_and_host_executor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wit_sort_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "wit_sort_check.cpp"),
                        os.path.join(CSRC, "cons_program_host.cpp"), os.path.join(CSRC, "program_compile.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wit_sort_check ok" in r.stdout


# ---- refusals ----
def _raw_create(sorts, n_sorts=None):
    """bx_wit_program_create_sorted over an empty step list with raw (rows, n_keys, n_cols, bits, sources, dests) tuples: what the builder
    cannot say (n_keys above the number of sources, a null list)"""
    lib = circuit._wit_lib()
    u32p = C.POINTER(C.c_uint32)
    desc = circuit.WitProgramDesc(None, 0, None, 0, None, 0)
    keep = [[(C.c_uint32 * max(len(v), 1))(*v) for v in s[3:]] for s in sorts]
    arr = (circuit.WitSort * max(len(sorts), 1))(*[circuit.WitSort(s[0], s[1], s[2], *[C.cast(a, u32p) for a in k]) for s, k in zip(sorts, keep)])
    handle = C.c_void_p()
    msg = lib.bx_wit_program_create_sorted(C.byref(desc), None, 0, arr if sorts else None, len(sorts) if n_sorts is None else n_sorts, C.byref(handle))
    if not msg:
        lib.bx_wit_program_destroy(handle)
    return msg.decode() if msg else None


def test_create_refuses_every_rule_by_name():
    def refused(match, build):
        w = WitnessProgram()
        build(w)
        with pytest.raises(HalError, match=match):
            w.compile()

    refused(r"sort 0: dest column 4 is also SET \(step 1\)", lambda w: (w.const(1), w.set(4, 0), w.sort([(0, 8)], [], [4])))
    refused("sort 0: dest column 4 is read by the GET of step 1: a sorted column does not exist while the program runs",
            lambda w: (w.const(1), w.get(1, 4, 0), w.sort([(0, 8)], [], [4])))
    refused("sort 0: dest column 4 is read by the GET of step 0", lambda w: (w.get(1, 4, 3), w.sort([(0, 8)], [], [4])))  # any back
    refused("sort 0: dest column 4 is the column of count 0", lambda w: (w.count(4, [1], 2), w.sort([(0, 8)], [], [4])))
    refused("sort 0: dest column 0 is a source of sort 0", lambda w: w.sort([(0, 8)], [1], [2, 0]))
    refused("sort 0: dest column 5 is a source of sort 1", lambda w: (w.sort([(0, 8)], [], [5]), w.sort([(5, 8)], [], [6])))
    refused("sort 1: dest column 0 is a source of sort 0", lambda w: (w.sort([(0, 8)], [], [5]), w.sort([(1, 8)], [], [0])))
    refused("sort 0: dest column 5 is already a dest of sort 0", lambda w: w.sort([(0, 8)], [1], [5, 5]))
    refused("sort 1: dest column 5 is already a dest of sort 0", lambda w: (w.sort([(0, 8)], [], [5]), w.sort([(1, 8)], [], [5])))
    refused("sort 0: source column 4 is the column of count 0: the counts run after the sorts", lambda w: (w.count(4, [1], 2), w.sort([(0, 8)], [4], [5, 6])))
    refused("sort 0: source column 3 is named twice", lambda w: w.sort([(3, 8)], [1, 3], [5, 6, 7]))
    refused(r"sort 0: source 1: data column 65536 out of range \(at most 65535\)", lambda w: w.sort([(0, 8)], [65536], [5, 6]))
    refused(r"sort 0: dest 0: data column 65536 out of range \(at most 65535\)", lambda w: w.sort([(0, 8)], [], [65536]))
    refused("sort 0: n_keys is 0", lambda w: w.sort([], [1], [5]))
    refused("sort 0: 5 keys, more than BX_WIT_MAX_SORT_KEYS = 4", lambda w: w.sort([(c, 2) for c in range(5)], [], range(10, 15)))
    refused("sort 0: no sources", lambda w: w.sort([], [], []))
    refused("sort 0: 17 sources, more than BX_WIT_MAX_SORT_COLS = 16", lambda w: w.sort([(0, 8)], range(1, 17), range(20, 37)))
    refused(r"sort 0: key 0: bits 0 is outside \[1, 31\]", lambda w: w.sort([(0, 0)], [], [5]))
    refused(r"sort 0: key 1: bits 32 is outside \[1, 31\]", lambda w: w.sort([(0, 8), (1, 32)], [], [5, 6]))
    refused("sort 0: the keys have 65 bits, more than BX_WIT_MAX_SORT_BITS = 64", lambda w: w.sort([(0, 31), (1, 31), (2, 3)], [], [5, 6, 7]))
    refused(r"sort 0: rows 16777217 is above 2\^24", lambda w: w.sort([(0, 8)], [], [5], rows=(1 << 24) + 1))
    refused("9 sorts, more than BX_WIT_MAX_SORTS = 8", lambda w: [w.sort([(0, 8)], [], [100 + k]) for k in range(9)])
    refused("step 0: constant 2013265921 is not below P", lambda w: (w.const(P), w.sort([], [], [])))  # the step list is judged first
    refused("count 0: bins is 0", lambda w: (w.count(4, [0], 0), w.sort([], [], [])))  # then the counts
    assert "sort 0: 2 keys, above its 1 sources" in _raw_create([(0, 2, 1, [8, 8], [0], [5])])
    assert "null sort list" in _raw_create([], n_sorts=1)
    with pytest.raises(ValueError, match="2 dests for 1 key and payload columns"):
        WitnessProgram().sort([(0, 8)], [], [5, 6])
    for bad in (dict(keys=[((1 << 32) + 1, 8)]), dict(keys=[(0, -1)]), dict(rows=-8), dict(dests=[1 << 32])):  # nothing wraps into a valid value
        with pytest.raises(ValueError, match="is not a 32-bit unsigned value"):
            WitnessProgram().sort(**{**dict(keys=[(0, 8)], payload=[], dests=[5], rows=0), **bad})
    # the limits themselves are fine, and so are a key that is SET, a count over a dest, a cell that names a dest and a program of sorts alone
    w = WitnessProgram()
    w.set(3, w.get(1, 0, 0))
    w.sort([(3, 31), (0, 31), (1, 1), (2, 1)], range(4, 16), range(100, 116), rows=1 << 24)
    for k in range(1, 8):
        w.sort([(3, 1 + k)], [], [200 + k])
    w.count(300, [100, 0], 5)
    w.global_cell(0, 100, 5)
    prog = w.compile()
    assert len(prog.sorts()) == 8 and prog.sorts()[0] == {"rows": 1 << 24, "keys": [(3, 31), (0, 31), (1, 1), (2, 1)], "payload": list(range(4, 16)),
                                                          "dests": list(range(100, 116))}
    assert prog.sorts()[7] == {"rows": 0, "keys": [(3, 8)], "payload": [], "dests": [207]} and prog.counts()[0]["sources"] == [100, 0]
    w = WitnessProgram()
    w.sort([(0, 3)], [], [1])
    prog = w.compile()
    assert prog.info() == {"steps": 0, "sets": 0, "narrow": 0, "instructions": 0, "taps": 0, "cells": 0}
    assert prog.sorts() == [{"rows": 0, "keys": [(0, 3)], "payload": [], "dests": [1]}] and prog.counts() == []
    # an unused entry of the tap list is no GET
    w = WitnessProgram()
    w.tap(1, 4, 0)
    w.sort([(0, 2)], [], [4])
    w.compile()


def test_a_sort_list_changes_neither_info_nor_digest_nor_the_generated_text():
    for name, make in ref.PROGRAMS.items():
        plain = compile_plain(make())
        b = sref.to_builder(make())
        free = [c for c in range(ref.WIDTHS[1]) if c not in make().derived()]
        b.sort([(free[0], 13), (make().derived()[0], 7)], free[1:2], [40, 41, 42], rows=7)
        b.sort([(free[0], 1)], [], [43])
        b.count(44, [40], 5, rows=7)
        sorted_ = b.compile()
        assert sorted_.info() == plain.info(), name
        assert sorted_.digest() == plain.digest(), name
        assert sorted_.emit_hip() == plain.emit_hip(), name
        assert plain.sorts() == [] and len(sorted_.sorts()) == 2
        assert all(sorted_.derives(c) for c in (40, 41, 42, 43, 44)) and not plain.derives(40)
        assert all(sorted_.derives(c) for c in make().derived()) and not any(sorted_.derives(c) for c in free)


def test_create_sorted_with_no_sorts_is_create_counted():
    lib = circuit._wit_lib()
    b = sref.to_builder(ref.every_form_program())
    free = [c for c in range(ref.WIDTHS[1]) if c not in ref.every_form_program().derived()]
    b.count(40, free[:1], 3, rows=5)
    counted = b.compile()
    steps = (circuit.ConsStep * len(b.steps))(*[circuit.ConsStep(*s) for s in b.steps])
    taps = (circuit.ConsTap * len(b.tap_list))(*[circuit.ConsTap(*t) for t in b.tap_list])
    cells = (circuit.WitGlobalCell * max(len(b.cells), 1))(*[circuit.WitGlobalCell(*g) for g in b.cells])
    desc = circuit.WitProgramDesc(steps, len(b.steps), taps, len(b.tap_list), cells, len(b.cells))
    src = (C.c_uint32 * 1)(free[0])
    counts = (circuit.WitCount * 1)(circuit.WitCount(40, 3, 5, 1, C.cast(src, C.POINTER(C.c_uint32))))
    handle = C.c_void_p()
    assert not lib.bx_wit_program_create_sorted(C.byref(desc), counts, 1, None, 0, C.byref(handle))
    other = circuit.CompiledWitnessProgram(lib, handle)
    assert other.info() == counted.info() and other.digest() == counted.digest() and other.emit_hip() == counted.emit_hip()
    assert other.counts() == counted.counts() == [{"col": 40, "bins": 3, "rows": 5, "sources": free[:1]}] and other.sorts() == counted.sorts() == []
    assert b"null sort list" in lib.bx_wit_program_create_sorted(C.byref(desc), counts, 1, None, 1, C.byref(handle))


def test_consgen_passes_a_sort_list_through():
    from boundless_amd import consgen

    desc = {"taps": [[1, 0, 0]], "steps": [[2, 0, 0, 0, 0], [10, 1, 0, 0, 0]],
            "sorts": [{"keys": [[1, 9], [0, 4]], "payload": [2], "dests": [3, 4, 5], "rows": 6}, {"keys": [[0, 31]], "dests": [6]}],
            "counts": [{"col": 7, "sources": [3], "bins": 4, "rows": 6}]}
    prog = consgen.witness_program_of(desc)
    assert prog.sorts() == [{"rows": 6, "keys": [(1, 9), (0, 4)], "payload": [2], "dests": [3, 4, 5]}, {"rows": 0, "keys": [(0, 31)], "payload": [], "dests": [6]}]
    assert prog.counts() == [{"col": 7, "bins": 4, "rows": 6, "sources": [3]}]
    plain = consgen.witness_program_of({k: v for k, v in desc.items() if k not in ("sorts", "counts")})
    assert plain.digest() == prog.digest() and plain.emit_hip() == prog.emit_hip() and plain.sorts() == []
    with pytest.raises(HalError, match=r"sort 0: key 0: bits 40 is outside \[1, 31\]"):
        consgen.witness_program_of(dict(desc, sorts=[{"keys": [[0, 40]], "dests": [6]}]))


# ---- the host executor against the reference ----
def _columns(prog, po2, widths, kind, seed=0):
    n = 1 << po2
    code = sref.random_columns((widths[0], n), seed=seed + 1)
    data = sref.random_columns((widths[1], n), seed=seed)
    for keys, _payload, _dests, _rows in prog.sorts:
        for col, _bits in keys:
            if col not in prog.derived():
                data[col] = sref.key_column(kind, n, seed=seed + col)
    data[prog.written()] = sref.POISON
    return code, data


@pytest.mark.parametrize("name", list(sref.HOST_PROGRAMS))
def test_run_host_is_the_reference_on_every_row(name):
    for po2 in (1, 3, 6):
        n = 1 << po2
        prog, w_data = sref.HOST_PROGRAMS[name](n)
        compiled = sref.compile_ref(prog)
        for kind in sref.KEY_PATTERNS:
            code, data = _columns(prog, po2, (ref.WIDTHS[0], w_data), kind, seed=po2)
            want = sref.evaluate(prog, po2, code, data)
            got = data.copy()
            compiled.run_host(po2, code, ref.WIDTHS[0], got, w_data)
            assert np.array_equal(got, want), f"po2 {po2}, {kind}: first differing (column, row) {tuple(np.argwhere(got != want)[0])}"
            free = [c for c in range(w_data) if c not in prog.written()]
            assert np.array_equal(got[free], data[free])
            for keys, payload, dests, rows in prog.sorts:
                rows = rows or n
                assert np.all(got[dests, rows:] == sref.POISON), "a row at or above `rows` was written"
                for src, dst in zip([c for c, _ in keys] + payload, dests):  # a permutation of the source's words, unchanged
                    assert np.array_equal(np.sort(got[dst, :rows]), np.sort(got[src, :rows]))
        compiled.close()


def test_the_sort_is_stable_and_sorts_by_the_low_bits():
    po2, n = 6, 64
    prog, w = sref.sort_program((3,), 1)  # key 0, payload 1 -> 2, 3
    compiled = sref.compile_ref(prog)
    data = np.zeros((w, n), np.uint32)
    values = (np.arange(n) * 37 + 8 * (np.arange(n) % 5)) % 1000  # cells at or above 2^3: only the low three bits order them
    data[0] = sref.encode_words(values)
    data[1] = sref.encode_words(np.arange(n))
    data[2:] = sref.POISON
    compiled.run_host(po2, np.zeros((3, n), np.uint32), 3, data, w)
    keys, rows = cref_decode(data[2]) & 7, cref_decode(data[3])
    assert np.all(np.diff(keys) >= 0) and set(keys.tolist()) == set((values & 7).tolist()) and len(set(keys.tolist())) > 1
    assert all(rows[i] < rows[i + 1] for i in range(n - 1) if keys[i] == keys[i + 1]), "ties are not in ascending row order"
    assert np.array_equal(cref_decode(data[2]), values[rows.astype(np.int64)]), "the word that moved is not the source's"
    compiled.close()


def cref_decode(words):
    return np.array(sref.decode_ints(words), np.int64)


def test_run_host_refuses_what_does_not_fit_the_shape_by_message():
    code, data = np.zeros((3, 8), np.uint32), np.full((8, 8), 5, np.uint32)
    before = data.copy()

    def one(keys, payload, dests, rows=0):
        p = sref.Program()
        p.sort(keys, payload, dests, rows)
        return p

    for prog, match in ((one([(0, 8)], [], [5], rows=9), "bx_wit_program_run_host: sort 0: rows 9 is above the trace's 8 rows"),
                        (one([(0, 8)], [8], [5, 6]), "bx_wit_program_run_host: sort 0: source 1 is data column 8, the data group has 8 columns"),
                        (one([(0, 8)], [1], [5, 8]), "bx_wit_program_run_host: sort 0: dest 1 is data column 8, the data group has 8 columns"),
                        (sref.two_sorts_program(rows_b=16), "bx_wit_program_run_host: sort 1: rows 16 is above the trace's 8 rows")):
        with pytest.raises(HalError, match=match):
            sref.compile_ref(prog).run_host(3, code, 3, data, 8)
        assert np.array_equal(data, before), "written before the refusal"
    sref.compile_ref(one([(0, 8)], [], [5], rows=8)).run_host(3, code, 3, data, 8)  # exactly N is fine


# ---- the sorted range check of tests/test_wit_sort_gpu.py, before any prover sees it ----
def test_the_range_circuits_programs_compile_and_its_trace_satisfies_them():
    import acc_ratio_ref
    from acc_ratio_cases import compile_ref as compile_acc
    from cons_program_cases import compile_ref as compile_cons

    po2, n = 9, 512
    cons, acc, wit = sref.range_programs(po2)
    ccons, cacc, cwit = compile_cons(cons), compile_acc(acc), sref.compile_ref(wit)
    assert ccons.info["degree"] == 3 and ccons.info["constraints"] == 5 and cacc.ratios() == 1 and cacc.info()["sequences"] == 1
    assert cwit.sorts() == [{"rows": n - sref.RC_TAIL, "keys": [(0, sref.RC_BITS)], "payload": [1], "dests": [2, 3]}] and (1 << sref.RC_BITS) >= sref.RC_B > (1 << (sref.RC_BITS - 1))
    code = sref.range_code(po2)
    mix = [sref.encode(v) for v in (3, 5, 7, 11)]
    for cheat in (False, True):
        free = sref.range_free_columns(po2, 2024, cheat)
        data = sref.evaluate(wit, po2, code, free)
        host = free.copy()
        cwit.run_host(po2, code, sref.RC_WIDTHS[0], host, sref.RC_WIDTHS[1])
        assert np.array_equal(host, data) and not np.any(data == sref.POISON)
        b = cref_decode(data[2])
        z_last = acc_ratio_ref.evaluate(acc, po2, code, data, [], mix)[:, n - 1]
        assert z_last.tolist() == [sref.encode(1), 0, 0, 0], "(b, q) is a permutation of (a, p) with or without the planted cell"
        holds = b[0] == 0 and b[n - 1] == sref.RC_B - 1 and set(np.diff(b).tolist()) <= {0, 1}
        assert holds == (not cheat)


# ---- the compiler's resource report ----
SORT_KERNELS = ("pack_kernel", "hist_kernel", "sums_kernel", "scan_kernel", "scatter_kernel", "gather_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_the_sort_kernels_use_no_scratch_and_the_kernels_beside_them_are_unchanged(tmp_path):
    report = _report("wit_sort.hip", tmp_path)
    kernels = {k: v for k, v in report.items() if "wit_sort" in k}
    assert len(kernels) == 6 and all(any(n in k for k in kernels) for n in SORT_KERNELS), sorted(kernels)
    for name, rep in kernels.items():
        assert rep["ScratchSize [bytes/lane]"] == 0 and rep["SGPRs Spill"] == 0 and rep["VGPRs Spill"] == 0, (name, rep)
        assert rep["Occupancy [waves/SIMD]"] == 8, (name, rep)
    (rep,) = [v for k, v in _report("wit_program.hip", tmp_path).items() if "wit_program_kernel" in k]
    assert (rep["VGPRs"], rep["TotalSGPRs"], rep["ScratchSize [bytes/lane]"]) == (10, 37, 0), rep
    counts = {k: v for k, v in _report("wit_count.hip", tmp_path).items() if "wit_count" in k}
    got = {n: (rep["VGPRs"], rep["TotalSGPRs"], rep["ScratchSize [bytes/lane]"]) for k, rep in counts.items() for n in ("lds_kernel", "global_kernel", "store_kernel") if n in k}
    assert got == {"lds_kernel": (10, 32, 0), "global_kernel": (8, 30, 0), "store_kernel": (5, 14, 0)}, got  # the parent's report
