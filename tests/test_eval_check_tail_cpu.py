"""CPU: what hipcc makes of eval_check_kernel (csrc/circuit.hip) once the constraints behind the walk — the accumulators', the
permutation pairs' and the two boundary ones — run on the lazy ext arithmetic of csrc/lazy_ext.hpp (WeightedExtAcc, the folded
LazyExtAcc) instead of fp.hpp's canonical f4_mul / f4_scale / f4_add.

csrc/circuit.hip is compiled to gfx950 assembly (no GPU needed; skipped without hipcc) and read with tools/isa_mix.py.  The kernel has
three loops, in this order: the walk over the derived columns, the accumulator constraints, the pair constraints.  PARENT holds what the
same tool counted in the commit before this form, per loop (VALU instructions, v_mad_u64_u32) and per kernel (VGPRs).
"""
import collections
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# eval_check_kernel<64, 4> before the lazy tail, by tools/isa_mix.py: loop -> (VALU instructions, v_mad_u64_u32 among them)
PARENT = {"walk": (317, 0), "accumulators": (321, 84), "pairs": (183, 46)}
# VGPRs of the dispatched shapes before the lazy tail (none of them with scratch)
PARENT_VGPRS = {"<64, 4>": 70, "<48, 3>": 62, "<16, 3>": 62, "<8, 2>": 62, "<0, 0>": 62}
SEVEN_WAVES = 70  # VGPRs: 512 / 7 rounded down to the allocation granule of 8 is 72

_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$")


def _resources(asm_text, symbol):
    at = asm_text.index("\n" + symbol + ":")
    vgprs = re.compile(r"; NumVgprs: (\d+)").search(asm_text, at)
    scratch = re.compile(r"; ScratchSize: (\d+)").search(asm_text, at)
    return int(vgprs.group(1)), int(scratch.group(1))


def _loops(isa_mix, asm_text, symbol):
    """[(issue classes, opcodes)] of the kernel's loops in the order of their headers: the basic blocks hipcc annotates as a loop's
    header or as `in Loop: Header=` it"""
    at = asm_text.index("\n" + symbol + ":")
    cur, members, order = None, collections.defaultdict(list), []
    for line in asm_text[at:asm_text.index("s_endpgm", at)].split("\n"):
        m = _BLOCK.match(line)
        if m:
            note = m.group(2) or ""
            header = re.search(r"Header=(BB\d+_\d+)", note)
            cur = header.group(1) if header else (m.group(1) if "Loop Header" in note else None)
            if cur and cur not in order:
                order.append(cur)
            continue
        word = line.strip()
        if cur and word and not word.startswith((";", ".")):
            members[cur].append((None, word.split()[0], ""))
    return [isa_mix.mix(members[h]) for h in order]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc to compile csrc/circuit.hip to gfx950 assembly")
def test_compiled_tail_loops_are_half_the_parents_and_the_walk_no_longer():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix

    asm = isa_mix.compile_asm(os.path.join(ROOT, "boundless_amd", "csrc", "circuit.hip"))
    try:
        text = open(asm).read()
        bodies = list(isa_mix.kernels(asm))
    finally:
        os.unlink(asm)
    names = isa_mix.demangle([sym for sym, _ in bodies])
    seen = {}
    for sym, _ in bodies:
        for shape in PARENT_VGPRS:
            if names[sym].startswith("void bx::eval_check_kernel" + shape + "("):
                seen[shape] = sym
    assert sorted(seen) == sorted(PARENT_VGPRS), sorted(seen)
    for shape, sym in seen.items():
        vgprs, scratch = _resources(text, sym)
        print(f"eval_check_kernel{shape}: {vgprs} VGPRs (parent {PARENT_VGPRS[shape]}), scratch {scratch}")
        assert scratch == 0, (shape, scratch)
        assert vgprs <= PARENT_VGPRS[shape], (shape, vgprs)
        assert vgprs <= SEVEN_WAVES, (shape, vgprs)

    # the three loops of <64, 4>: only loops that load from memory (every one of the three reads its columns), in the order of the source
    loops = [(cls, ops) for cls, ops in _loops(isa_mix, text, seen["<64, 4>"]) if cls["vmem"] > 0]
    assert len(loops) == 3, [(cls["mul"] + cls["cheap"], cls["vmem"]) for cls, _ in loops]
    found = dict(zip(("walk", "accumulators", "pairs"), loops))
    for name, (cls, ops) in found.items():
        print(f"{name}: {cls['mul'] + cls['cheap']} VALU (parent {PARENT[name][0]}), v_mad_i64_i32 {ops['v_mad_i64_i32']}, v_mad_u64_u32 {ops['v_mad_u64_u32']} "
              f"(parent {PARENT[name][1]}), v_mul_lo_u32 {ops['v_mul_lo_u32']}, {cls['vmem']} loads")
    # that these are the loops they are taken for: the walk holds the constraint sum (by far the most signed multiply-adds), an
    # accumulator reads its ext column at two rows and a data word (nine loads), a pair two ext columns (eight)
    assert found["walk"][1]["v_mad_i64_i32"] >= 100 and found["walk"][1]["v_mad_i64_i32"] > 2 * found["accumulators"][1]["v_mad_i64_i32"], dict(found["walk"][1])
    assert found["accumulators"][0]["vmem"] == 9 and found["pairs"][0]["vmem"] == 8, (found["accumulators"][0]["vmem"], found["pairs"][0]["vmem"])
    valu = {name: cls["mul"] + cls["cheap"] for name, (cls, _) in found.items()}
    assert 2 * valu["accumulators"] <= PARENT["accumulators"][0], valu
    assert 2 * valu["pairs"] <= PARENT["pairs"][0], valu
    assert valu["walk"] <= PARENT["walk"][0], valu
    for name, (_, ops) in found.items():
        assert ops["v_mad_u64_u32"] <= PARENT[name][1], (name, ops["v_mad_u64_u32"])
