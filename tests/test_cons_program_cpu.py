"""CPU: constraint programs (include/bx_program.h) — the compiler's refusals and its bookkeeping, the tap sets, and the host executor
(the verifier's constraints_at) against the definition-level reference of tests/cons_program_ref.py and against the lookup
circuit's hand-written constraints_at.  No GPU: the compiler and the host executor are host code."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cons_program_ref as ref  # noqa: E402
from cons_program_cases import PROGRAMS, WIDTHS, compile_ref, to_builder  # noqa: E402

from boundless_amd.circuit import CONS_MAX_NARROW, CONS_MAX_WIDE, ConsProgram, TapReader, _TAP_AT, lookup_circuit  # noqa: E402
from boundless_amd.hal import HalError  # noqa: E402
from boundless_amd.prover import SegmentParams  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P


def test_the_header_is_pedantic_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", "-x", "c", "-"],
                       input='#include "bx_program.h"\nint main(void){bx_cons_program_desc d; bx_cons_program_info i; (void)d; (void)i; return 0;}\n',
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- refusals ----
def _chain(p, y):
    return p.and_eqz(p.true(), y)


def test_create_refuses_every_rule_by_name():
    def refused(match, build, ret=None):
        p = ConsProgram(2)
        build(p)
        with pytest.raises(HalError, match=match):
            p.compile(ret=ret)

    refused("operand b = 1 refers to a later or missing fp var", lambda p: p.add(p.const(1), 1))
    refused("operand a = 7 refers to a later or missing fp var", lambda p: (p.const(1), p.mul(7, 0)))
    refused("operand a = 0 refers to a later or missing mix var", lambda p: p.and_eqz(0, p.const(1)))  # no TRUE yet
    refused("operand b = 3 refers to a later or missing fp var", lambda p: p.and_eqz(p.true(), 3))  # a mix index is no fp var
    refused("operand c = 1 refers to a later or missing mix var", lambda p: p.and_cond(p.true(), p.const(1), 1))
    refused("tap index 1 out of range", lambda p: (p.get(0, 0, 0), _chain(p, p.get_tap(1))))
    refused("tap group 3 out of range", lambda p: _chain(p, p.get(3, 0, 0)))
    refused("tap column 65536 out of range", lambda p: _chain(p, p.get(0, 65536, 0)))
    refused("tap back 65536 out of range", lambda p: _chain(p, p.get(0, 0, 65536)))
    refused("global index 2 out of range", lambda p: _chain(p, p.global_(2)))
    refused("mix component 4 out of range", lambda p: _chain(p, p.mix(4)))
    refused("GET_GLOBAL table 2 out of range", lambda p: _chain(p, p._fp(3, 2, 0)))
    refused(f"constant {P} is not below P", lambda p: _chain(p, p.const(P)))
    refused("component not below P", lambda p: _chain(p, p.const_ext(0, 0, P, 0)))
    refused("ret = 2 is not a mix var", lambda p: _chain(p, p.const(1)), ret=2)
    refused(r"ret = 0 is not a mix var \(0 mix vars\)", lambda p: p.const(1), ret=0)
    refused("unknown op 10", lambda p: p._fp(10))
    refused("n_globals 65 is above BX_MAX_GLOBALS", lambda p: setattr(p, "n_globals", 65) or p.true())
    refused("more than BX_CONS_MAX_STEPS = 65536", lambda p: [p.true() for _ in range(65537)])
    # constraint counts add up through AND_COND: doubling 17 times passes the bound
    def doubling(p):
        m = _chain(p, p.const(1))
        for _ in range(17):
            m = p.and_cond(m, 0, m)
    refused("constraints, more than BX_CONS_MAX_STEPS", doubling)
    p = ConsProgram(0)
    p.compile(ret=[p.true() for _ in range(65536)][-1]).close()  # exactly the limit


def test_a_ninth_back_on_one_column_is_refused_and_taps_are_sorted():
    p = ConsProgram(0)
    top = p.true()
    for back in (5, 3, 0, 9, 1, 12, 7, 2):  # eight distinct backs, 0 among them
        top = p.and_eqz(top, p.get(1, 4, back))
    top = p.and_eqz(top, p.get(2, 0, 6))  # 0 is opened although the program does not name it
    prog = p.compile()
    assert prog.taps(1, 4) == [0, 1, 2, 3, 5, 7, 9, 12]
    assert prog.taps(2, 0) == [0, 6]
    assert prog.taps(1, 3) == [0] and prog.taps(0, 0) == [0] and prog.taps(2, 9999) == [0]  # never named
    p.and_eqz(top, p.get(1, 4, 4))
    with pytest.raises(HalError, match="more than BX_MAX_TAPS = 8 distinct backs on column 4 of group 1"):
        p.compile()
    q = ConsProgram(0)  # without 0 named, eight others are nine with it
    top = q.true()
    for back in range(1, 9):
        top = q.and_eqz(top, q.get(0, 1, back))
    with pytest.raises(HalError, match="more than BX_MAX_TAPS = 8 distinct backs on column 1 of group 0"):
        q.compile()


# ---- info ----
def test_info_counts_constraints_through_nested_and_cond():
    info = compile_ref(ref.every_form_program()).info
    # 14 AND_EQZ on the top chain; m3 = 2; m2 = 1 + m3 + 1 = 4; m1 = 1 + m2 = 5; then + m1, + 1
    assert info["constraints"] == 14 + 5 + 1
    assert info["degree"] == 5 and info["n_globals"] == 2 and info["taps"] == 3
    assert info["steps"] == len(ref.every_form_program().steps) and info["instructions"] == info["steps"]
    one = compile_ref(ref.one_constraint_program()).info
    assert (one["constraints"], one["degree"], one["narrow"], one["wide"]) == (1, 1, 1, 2)


def test_degree_five_is_accepted_and_six_refused():
    def power(p, n, combine):
        x = p.get(1, 0, 0)
        v = x
        for _ in range(n - 1):
            v = p.mul(v, x)
        return combine(p, v)

    via_eqz = lambda p, v: p.and_eqz(p.true(), v)  # noqa: E731
    for n in (5, 6):
        p = ConsProgram(0)
        power(p, n, via_eqz)
        if n == 5:
            assert p.compile().info["degree"] == 5
        else:
            with pytest.raises(HalError, match="degree 6 is above BX_CONS_MAX_DEGREE = 5"):
                p.compile()
    # AND_COND: cond + inner.  add / sub take the max
    for n, ok in ((2, True), (3, False)):
        p = ConsProgram(0)
        x = p.get(1, 0, 0)
        cube = p.mul(p.mul(x, x), x)
        inner = p.and_eqz(p.true(), p.sub(cube, p.add(x, p.const(3))))  # degree 3
        cond = x if n == 2 else cube
        cond = p.mul(cond, x) if n == 2 else cond  # degree 2 or 3
        p.and_cond(p.true(), cond, inner)
        if ok:
            assert p.compile().info["degree"] == 5
        else:
            with pytest.raises(HalError, match="degree 6 is above"):
                p.compile()


# ---- slot files ----
def test_programs_at_the_slot_limits_compile_and_one_more_live_value_is_refused():
    narrow = compile_ref(ref.narrow_limit_program()).info
    assert narrow["narrow"] == CONS_MAX_NARROW == ref.MAX_NARROW
    wide = compile_ref(ref.wide_limit_program()).info
    assert wide["wide"] == CONS_MAX_WIDE == ref.MAX_WIDE
    both = compile_ref(ref.both_limits_program()).info
    assert (both["narrow"], both["wide"]) == (CONS_MAX_NARROW, CONS_MAX_WIDE)  # the kernel's LDS ceiling: 32 + 4 * 24 KiB
    with pytest.raises(HalError, match=r"needs 33 live narrow \(base\) values, the limit is 32"):
        compile_ref(ref.narrow_limit_program(extra=1))
    with pytest.raises(HalError, match=r"needs 25 live wide \(ext and mix\) values, the limit is 24"):
        compile_ref(ref.wide_limit_program(extra=1))


def test_freed_slots_are_reused():
    info = compile_ref(PROGRAMS["steps_700"]()).info
    assert info["steps"] >= 700 and info["narrow"] <= 20 and info["wide"] <= 20  # hundreds of values went through a few slots


# ---- the host executor against the reference ----
def _random_taps(rng):
    cache = {}

    def tap(group, col, back):
        key = (group, col, back)
        if key not in cache:
            cache[key] = [int(v) for v in rng.integers(0, P, 4)]
        return cache[key]
    return tap


def _words(rng, n):
    return [int(v) for v in rng.integers(0, P, n)]


@pytest.mark.parametrize("block", range(5))
def test_constraints_at_is_the_reference_on_50_random_programs(block):
    for seed in range(10 * block, 10 * block + 10):
        rng = np.random.default_rng(seed)
        prog = ref.random_program(seed, steps=int(rng.integers(5, 160)), widths=WIDTHS, nesting=seed % 4, ext_share=(seed % 5) / 8, pressure=4 + seed % 12,
                                  n_taps=4 + seed % 20)
        compiled = compile_ref(prog)
        tap, pm, mix, g = _random_taps(rng), _words(rng, 4), _words(rng, 4), _words(rng, 2)
        got = compiled.constraints_at(tap, pm, mix, g)
        assert got == ref.at_point(prog, tap, pm, mix, g), f"seed {seed}: {compiled.info}"
        assert any(got)
        compiled.close()


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_constraints_at_is_the_reference_on_the_named_programs(name):
    prog = PROGRAMS[name]()
    rng = np.random.default_rng(5)
    tap, pm, mix, g = _random_taps(rng), _words(rng, 4), _words(rng, 4), _words(rng, 2)
    assert compile_ref(prog).constraints_at(tap, pm, mix, g) == ref.at_point(prog, tap, pm, mix, g)


@pytest.mark.parametrize("po2,widths,V", [(9, (3, 4, 12), 1), (12, (3, 10, 20), 2), (9, (16, 256, 64), 7)])
def test_the_lookup_program_is_the_lookup_circuits_constraints_at(po2, widths, V):
    prog = ref.lookup_program(po2, widths)
    compiled = compile_ref(prog)
    assert compiled.info["constraints"] == 3 * V + 4 and compiled.info["degree"] == 3
    ops = lookup_circuit().contents
    shape = SegmentParams(po2, *widths, 0, 0)
    for a in range(2 * V + 1):  # the tap sets are the built-in table's
        for col in (4 * a, 4 * a + 3):
            backs = (C.c_uint32 * 8)()
            n = ops.taps(None, C.byref(shape), 2, col, backs)
            assert compiled.taps(2, col) == list(backs[:n]) == [0, 1]
    assert compiled.taps(2, 4 * (2 * V + 1)) == [0] and compiled.taps(1, 0) == [0]
    rng = np.random.default_rng(po2 + V)
    for _ in range(3):
        tap, pm, mix, g = _random_taps(rng), _words(rng, 4), _words(rng, 4), _words(rng, 2)

        def at(_ctx, group, col, back, out):
            for i, v in enumerate(tap(group, col, back)):
                out[i] = v
            return None

        reader = TapReader(None, _TAP_AT(at))
        out = (C.c_uint32 * 4)()
        msg = ops.constraints_at(None, C.byref(shape), C.byref(reader), (C.c_uint32 * 4)(*pm), (C.c_uint32 * 4)(*mix), (C.c_uint32 * 2)(*g), out)
        assert not msg
        assert compiled.constraints_at(tap, pm, mix, g) == list(out) == ref.at_point(prog, tap, pm, mix, g)


def test_a_refusing_readers_message_comes_back():
    compiled = compile_ref(ref.square_program())

    def tap(group, col, back):
        if (group, col, back) == (1, 0, 3):
            raise KeyError("column 0 of group 1 is not opened 3 rows back")
        return [1, 2, 3, 4]

    with pytest.raises(HalError, match="column 0 of group 1 is not opened 3 rows back"):
        compiled.constraints_at(tap, [1, 2, 3, 4], [5, 6, 7, 8], [9])


def test_eight_threads_evaluate_one_program_at_once():
    prog = PROGRAMS["steps_700"]()
    compiled = compile_ref(prog)
    inputs, want, got = [], [], [None] * 8
    for k in range(8):
        rng = np.random.default_rng(100 + k)
        tap = _random_taps(rng)
        for t in prog.taps:
            tap(*t)  # fill the cache now: the threads only read it
        inputs.append((tap, _words(rng, 4), _words(rng, 4), _words(rng, 2)))
        want.append(ref.at_point(prog, *inputs[-1]))

    def work(k):
        for _ in range(20):
            got[k] = compiled.constraints_at(*inputs[k])

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == want and len({tuple(w) for w in want}) == 8


def test_the_builder_and_the_reference_builder_write_the_same_steps():
    """tests/cons_program_ref.py and boundless_amd.circuit.ConsProgram are written separately; the same calls must give the same
    step list (this is what lets the tests hand a reference program to the library)."""
    a, b = ref.Program(1), ConsProgram(1)
    for p in (a, b):
        x = p.get(1, 0, 2)
        e = p.const_ext(1, 2, 3, 4)
        inner = p.and_eqz(p.true(), p.sub(p.mul(x, e), p.add(p.global_(0), p.mix(3))))
        p.and_cond(p.true(), p.const(7), inner)
    assert [tuple(s) for s in a.steps] == [tuple(s) for s in b.steps] and a.taps == b.tap_list
    assert to_builder(a).steps == b.steps
