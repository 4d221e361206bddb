"""CPU: the centred entry point of the constraint sum of csrc/circuit_dev.hpp and the walk that feeds it (DerivedRegs<true>: a pool
entry is centred once, where it is loaded or produced), and what hipcc makes of the two kernels built on them.

  * tests/cons_levels_check.cpp, a stand-alone program: the centred entry against the plain canonical loop and against the
    canonical-pool signature on the +-P/2, 0, P - 1 and random pools, and a walk of 19 cells through centred registers against
    the same walk through canonical ones.  Built plainly, with every bound asserted (-DBX_CHECK_BOUNDS: each entering pool entry within
    P/2, each sredc operand, each level's sum), and with the bounds under the address and undefined-behaviour sanitizers.
  * csrc/circuit.hip compiled to gfx950 assembly (no GPU needed; skipped without hipcc), read with tools/isa_mix.py: the walk loops
    of witness_derive_kernel<64,4> and eval_check_kernel<64,4> against the counts of the commit before the r·R levels were kept as
    multiply-adds and the pool was centred on entry (412 and 467 VALU instructions per cell, 65 / 87 VGPRs, no scratch).
"""
import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the walk loop per cell before this change (VALU instructions), and the least it has to lose: 64 (levels) + 36 (centring) by the
# instruction lists, less some room for scheduling differences
PARENT_LOOP = {"witness_derive_kernel<64, 4>": 412, "eval_check_kernel<64, 4>": 467}
PARENT_VGPRS = {"witness_derive_kernel<64, 4>": 65, "eval_check_kernel<64, 4>": 87}
LEAST_SAVED = 90


@pytest.mark.parametrize("flags", [[], ["-DBX_CHECK_BOUNDS"], ["-DBX_CHECK_BOUNDS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "bounds", "bounds-asan-ubsan"])
def test_centred_entry_and_centred_walk_equal_the_canonical_ones(tmp_path, flags):
    exe = str(tmp_path / "cons_levels_check")
    csrc = os.path.join(ROOT, "boundless_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O2", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}",
                        os.path.join(ROOT, "tests", "cons_levels_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cons_levels_check ok" in r.stdout
    # the bound every static_assert downstream rests on is live: an entry one step outside [-P/2, P/2] is refused where bounds are asserted
    r = subprocess.run([exe, "uncentred"], capture_output=True, text=True, timeout=60)
    if "-DBX_CHECK_BOUNDS" in flags:
        assert r.returncode != 0 and "a pool entry that is not centred" in r.stderr, (r.returncode, r.stdout, r.stderr)
    else:
        assert r.returncode == 0, r.stderr


def _resources(asm_text, symbol):
    """(VGPRs, scratch bytes) hipcc reports after the body of kernel `symbol`"""
    at = asm_text.index("\n" + symbol + ":")
    vgprs = re.compile(r"; NumVgprs: (\d+)").search(asm_text, at)
    scratch = re.compile(r"; ScratchSize: (\d+)").search(asm_text, at)
    return int(vgprs.group(1)), int(scratch.group(1))


_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$")


def _largest_loop(isa_mix, asm_text, symbol):
    """(issue classes, opcodes) of the kernel's largest loop: the basic blocks hipcc annotates as the loop's header or as `in Loop:
    Header=` it.  tools/isa_mix.py's loop summary lists the span of every backward branch, and in these kernels the blocks of the
    initial loads are laid out behind the walk and jump back to labels in front of it, so the largest spans there are no loops; its
    entries for the walk's own labels (.LBB7_43: 412, .LBB12_28: 467 before this change) are the counts this returns."""
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
    return max((isa_mix.mix(block) for block in members.values()), key=lambda m: m[0]["mul"] + m[0]["cheap"])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc to compile csrc/circuit.hip to gfx950 assembly")
def test_compiled_walk_loops_lost_the_emulated_levels_and_the_per_cell_centring():
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
    for sym, body in bodies:
        for kernel in PARENT_LOOP:
            if names[sym].startswith("void bx::" + kernel + "("):
                # the walk is the kernel's largest loop (eval_check's accumulator loop holds 321 VALU instructions, its pair loop 183)
                cls, ops = _largest_loop(isa_mix, text, sym)
                multiplies = sum(n for op, n in ops.items() if op.startswith(("v_mad_i64", "v_mad_u64", "v_mul_lo", "v_mul_hi")))
                found[kernel] = (cls["mul"] + cls["cheap"], multiplies, ops, *_resources(text, sym))
    assert sorted(found) == sorted(PARENT_LOOP), sorted(found)
    for kernel, (valu, mul, ops, vgprs, scratch) in found.items():
        print(f"{kernel}: walk loop {valu} VALU ({mul} multiplies), v_mad_u64_u32 {ops['v_mad_u64_u32']}, v_ashrrev_i32 {ops['v_ashrrev_i32']}, "
              f"v_lshl_add_u64 {ops['v_lshl_add_u64']}, v_mov_b32 {ops['v_mov_b32']}, v_cndmask_b32 {ops['v_cndmask_b32']}; {vgprs} VGPRs, scratch {scratch}")
    for kernel, (valu, mul, ops, vgprs, scratch) in found.items():
        assert valu <= PARENT_LOOP[kernel] - LEAST_SAVED, (kernel, valu, PARENT_LOOP[kernel])
        assert scratch == 0, (kernel, scratch)
        assert vgprs <= PARENT_VGPRS[kernel], (kernel, vgprs, PARENT_VGPRS[kernel])
    assert found["witness_derive_kernel<64, 4>"][2]["v_mad_u64_u32"] == 0
