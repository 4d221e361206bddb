"""CPU: the constraint sums of csrc/circuit_dev.hpp (cons_sum<TT, GG>: a 64-bit chain per sum, folded hi * R + lo and reduced once at
the end; pairs at G = 4, factored at G = 3 and G >= 5, term by term at G <= 2), and what hipcc makes of the two kernels built on them.

  * tests/cons_sum_check.cpp, a stand-alone program: fold_r's identity and bound at the edges of 64 bits, the plans that run (FoldPlan
    over PairPlan's splits: every term once, no segment with a shared pair or beyond SEG terms, its bounds recomputed; ConsPlan: every
    term under its own first factor, its fold segments), cons_sum<TT, GG> through the centred entry and the canonical-pool signature
    against the run-time term-by-term loop on all 2^16 sign patterns of +-P/2, the constant pools, edge words and random ones, and
    the walk of 19 cells through centred registers against canonical ones.  Built plainly, with every bound asserted
    (-DBX_CHECK_BOUNDS: each entering pool entry within P/2, each pair, sredc operand, fold and chain), and with the bounds under the
    address and undefined-behaviour sanitizers, where a chain that left 64 bits is a signed overflow.
  * csrc/circuit.hip compiled to gfx950 assembly (no GPU needed; skipped without hipcc), read with tools/isa_mix.py: the walk loops of
    witness_derive_kernel<64,4> and eval_check_kernel<64,4> against the counts of the commit before the fold form (312 VALU
    instructions / 274 multiplies per cell and 54 VGPRs; 367 / 298 and 78 VGPRs): at least 30 VALU instructions and 50 multiplies
    fewer per cell, no v_mad_u64_u32 in the loop, no scratch, no more VGPRs.
"""
import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the walk loop per cell before the fold form, by tools/isa_mix.py: (VALU instructions, multiplies, VGPRs)
PARENT = {"witness_derive_kernel<64, 4>": (312, 274, 54), "eval_check_kernel<64, 4>": (367, 298, 78)}
LEAST_VALU_SAVED, LEAST_MUL_SAVED = 30, 50
MULTIPLIES = ("v_mad_i64", "v_mad_u64", "v_mul_lo", "v_mul_hi")


@pytest.mark.parametrize("flags", [[], ["-DBX_CHECK_BOUNDS"], ["-DBX_CHECK_BOUNDS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "bounds", "bounds-asan-ubsan"])
def test_plans_are_sound_and_every_form_equals_the_term_by_term_sum(tmp_path, flags):
    exe = str(tmp_path / "cons_sum_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O2", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}",
                        os.path.join(ROOT, "tests", "cons_sum_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cons_sum_check ok" in r.stdout
    print(r.stdout)
    # the bound every static_assert downstream rests on is live: an entry one step outside [-P/2, P/2] is refused where bounds are asserted
    r = subprocess.run([exe, "uncentred"], capture_output=True, text=True, timeout=60)
    if "-DBX_CHECK_BOUNDS" in flags:
        assert r.returncode != 0 and "a pool entry that is not centred" in r.stderr, (r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 0, r.stderr


_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$")


def _resources(asm_text, symbol):
    """(VGPRs, scratch bytes) hipcc reports after the body of kernel `symbol`"""
    at = asm_text.index("\n" + symbol + ":")
    vgprs = re.compile(r"; NumVgprs: (\d+)").search(asm_text, at)
    scratch = re.compile(r"; ScratchSize: (\d+)").search(asm_text, at)
    return int(vgprs.group(1)), int(scratch.group(1))


def _walk_loop(isa_mix, asm_text, symbol):
    """(issue classes, opcodes) of the walk over the derived columns: of the kernel's loops (the basic blocks hipcc annotates as a
    loop's header or as `in Loop: Header=` it) the one with the most signed multiply-adds.  The constraint sums are the only code of
    these kernels that multiplies signed words; eval_check's accumulator loop, which holds more instructions than the walk (321),
    multiplies unsigned ones."""
    at = asm_text.index("\n" + symbol + ":")
    cur, members = None, collections.defaultdict(list)
    for line in asm_text[at:asm_text.index("s_endpgm", at)].split("\n"):
        m = _BLOCK.match(line)
        if m:
            note = m.group(2) or ""
            header = re.search(r"Header=(BB\d+_\d+)", note)
            cur = header.group(1) if header else (m.group(1) if "Loop Header" in note else None)
            continue
        word = line.strip()
        if cur and word and not word.startswith((";", ".")):
            members[cur].append((None, word.split()[0], ""))
    return max((isa_mix.mix(block) for block in members.values()), key=lambda m: m[1]["v_mad_i64_i32"])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc to compile csrc/circuit.hip to gfx950 assembly")
def test_compiled_walk_loops_lost_the_reduction_levels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix

    asm = isa_mix.compile_asm(os.path.join(ROOT, "boundless_amd", "csrc", "circuit.hip"))
    try:
        text = open(asm).read()
        bodies = list(isa_mix.kernels(asm))
    finally:
        os.unlink(asm)
    names = isa_mix.demangle([sym for sym, _ in bodies])
    found = {}
    for sym, _ in bodies:
        for kernel in PARENT:
            if names[sym].startswith("void bx::" + kernel + "("):
                cls, ops = _walk_loop(isa_mix, text, sym)
                multiplies = sum(n for op, n in ops.items() if op.startswith(MULTIPLIES))
                found[kernel] = (cls["mul"] + cls["cheap"], multiplies, ops, cls["nop"], *_resources(text, sym))
    assert sorted(found) == sorted(PARENT), sorted(found)
    for kernel, (valu, mul, ops, nops, vgprs, scratch) in found.items():
        print(f"{kernel}: walk loop {valu} VALU ({mul} multiplies), v_mad_i64_i32 {ops['v_mad_i64_i32']}, v_mad_u64_u32 {ops['v_mad_u64_u32']}, "
              f"v_lshl_add_u64 {ops['v_lshl_add_u64']}, v_mov_b32 {ops['v_mov_b32']}, s_nop {nops}; {vgprs} VGPRs, scratch {scratch}")
    for kernel, (valu, mul, ops, nops, vgprs, scratch) in found.items():
        parent_valu, parent_mul, parent_vgprs = PARENT[kernel]
        assert ops["v_mad_i64_i32"] >= 100, (kernel, "not the walk", dict(ops))
        assert valu <= parent_valu - LEAST_VALU_SAVED, (kernel, valu, parent_valu)
        assert mul <= parent_mul - LEAST_MUL_SAVED, (kernel, mul, parent_mul)
        assert ops["v_mad_u64_u32"] == 0, (kernel, ops["v_mad_u64_u32"])
        assert scratch == 0, (kernel, scratch)
        assert vgprs <= parent_vgprs, (kernel, vgprs, parent_vgprs)
