"""Which kernels the NTT entry points launch, case by case: the record behind tests/golden/ntt_launches.json.

    rocprofv3 --kernel-trace --output-format csv -d out -o kt -- python tools/ntt_launch_trace.py run
    python tools/ntt_launch_trace.py reduce <kernel_trace.csv> <launches.json>
    python tools/ntt_launch_trace.py diff <parent.json> <this.json> <result.json>

`run` drives the fixed list of cases() through HipHal on zeroed buffers (a launch depends on shape, alignment and tunables, never
on values).  One batch_bit_reverse of a 2-word buffer stands before the first case and after every case: no case launches
bit_reverse_kernel otherwise, so that kernel marks the boundaries in the trace.  `reduce` cuts the trace at the markers and lists per
case, in stream order, each NTT pass kernel with its template arguments, workgroup size, grid (in workgroups) and LDS bytes; the
table builders (twist_build_kernel, zk_tab_kernel, zk_full_kernel) run when a cache misses, not per case, and are only counted.
The planner's CPU check (tests/ntt_plan_check.cpp) replays every case of the golden file without a GPU.
"""
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULTS = {"ntt_block_log": 12, "ntt_tile_log": 14, "ntt_fast": 1, "ntt_tile_a_log": 12, "ntt_tile_b_log": 13, "ntt_cols_per_wg": 8,
            "ntt_group_cols": 0, "ntt_tile_b_wide": 1}  # csrc/ntt_plan.hpp
ENTRIES = ("interpolate", "interpolate_zk", "evaluate", "expand")  # batch_interpolate_ntt, batch_interpolate_zk, batch_evaluate_ntt, batch_expand_into_evaluate_ntt
PASS_KERNELS = ("ntt_block_kernel", "ntt_strided_kernel", "ntt_r16_kernel", "ntt_passA_fwd12_multi_kernel", "zk_shift_kernel")
TABLE_KERNELS = ("twist_build_kernel", "zk_tab_kernel", "zk_full_kernel")
MAX_WORDS = (1 << 26) + 8


def cases():
    """[{entry, m (log2 of the transformed column), count, bits (expand_bits), offset (words), tunables}]"""
    out = []

    def add(entry, m, count, bits=0, offset=0, **tunables):
        assert entry in ENTRIES and (count << m) + offset <= MAX_WORDS and set(tunables) <= set(DEFAULTS)
        out.append({"entry": entry, "m": m, "count": count, "bits": bits, "offset": offset, "tunables": dict(DEFAULTS, **tunables)})

    def all_entries(m, count, offset=0, **t):
        add("interpolate", m, count, 0, offset, **t)
        add("interpolate_zk", m, count, 0, offset, **t)
        add("evaluate", m, count, 0, offset, **t)
        if m >= 2:
            add("evaluate", m, count, 2, offset, **t)
            add("expand", m, count, 2, offset, **t)

    # default tunables, every size
    for m in range(1, 27):
        for count in ((1, 3) if m <= 20 else (1,)):
            all_entries(m, count)
    # tests/test_hal_gpu.py::test_ntt_full_size_vs_oracle_and_roundtrip
    for fast, block_log, tile_log, tile_a, tile_b in [(0, 12, 14, 12, 13), (0, 13, 14, 12, 13), (0, 11, 13, 12, 13), (0, 10, 12, 12, 13), (1, 12, 14, 12, 13),
                                                      (1, 12, 14, 12, 14), (1, 13, 14, 13, 13), (1, 11, 14, 12, 12), (1, 10, 14, 11, 13), (1, 12, 14, 13, 11)]:
        t = {"ntt_fast": fast, "ntt_block_log": block_log, "ntt_tile_log": tile_log, "ntt_tile_a_log": tile_a, "ntt_tile_b_log": tile_b}
        add("interpolate", 20, 7, **t)
        add("interpolate_zk", 20, 7, **t)
        add("expand", 22, 7, 2, **t)
        add("evaluate", 20, 7, 0, **t)
    # tests/test_hal_gpu.py::test_lde_columns_per_workgroup
    for cpw, count in [(1, 5), (2, 5), (4, 7), (8, 3), (8, 17), (16, 16)]:
        add("expand", 16, count, 2, ntt_cols_per_wg=cpw)
        add("evaluate", 14, count, 0, ntt_cols_per_wg=cpw)
    # tests/test_selectable_paths_gpu.py::test_ntt_column_groups
    for bits in (12, 14):
        for g, count in [(1, 3), (2, 5), (3, 7), (5, 7), (4, 4), (8, 3)]:
            for cpw in (8, 4):
                t = {"ntt_group_cols": g, "ntt_cols_per_wg": cpw}
                add("expand", bits + 2, count, 2, **t)
                add("evaluate", bits + 2, count, 0, **t)
                add("evaluate", bits + 2, count, 2, **t)
    # tests/test_selectable_paths_gpu.py::test_ntt_pass_b_without_the_widened_tile
    for m, tile_b in [(22, 13), (23, 13), (22, 12)]:
        add("interpolate", m, 2, ntt_tile_b_wide=0, ntt_tile_b_log=tile_b)
        add("expand", m, 2, 2, ntt_tile_b_wide=0, ntt_tile_b_log=tile_b)
    # expand_bits = 1: the v1 contiguous pass in front of the radix-16 strided pass
    add("expand", 15, 1, 1)
    add("evaluate", 15, 1, 1)
    # a slice that is only word-aligned: the same mix, in both directions
    for m in (13, 14):
        all_entries(m, 2, offset=1)
    return out


def run():
    from boundless_amd.hal import HipHal

    hal = HipHal(0)
    io, out, two = hal.alloc_zeroed(MAX_WORDS), hal.alloc_zeroed(MAX_WORDS), hal.alloc_zeroed(2)
    hal.batch_bit_reverse(two, 1)
    for case in cases():
        for name, value in case["tunables"].items():
            hal.set_tunable(name, value)
        m, count, bits, off = case["m"], case["count"], case["bits"], case["offset"]
        buf = io.slice(off, count << m)
        if case["entry"] == "interpolate":
            hal.batch_interpolate_ntt(buf, count)
        elif case["entry"] == "interpolate_zk":
            hal.batch_interpolate_zk(buf, count)
        elif case["entry"] == "evaluate":
            hal.batch_evaluate_ntt(buf, count, bits)
        else:  # from the (possibly offset) slice into an aligned output
            hal.batch_expand_into_evaluate_ntt(out.slice(0, count << m), io.slice(off, count << (m - bits)), count, bits)
        hal.batch_bit_reverse(two, 1)
    hal.sync()
    hal.close()
    print(json.dumps({"cases": len(cases())}))


def short_name(kernel_name):
    """'void bx::ntt_r16_kernel<false, true, 2, 12, 0, 512>(bx::R16Args)' -> 'ntt_r16_kernel<false, true, 2, 12, 0, 512>'"""
    name = re.sub(r"\(.*\)\s*(\[.*\])?$", "", kernel_name.strip())
    name = re.sub(r"^void\s+", "", name)
    return re.sub(r"\bbx::", "", name).replace(".kd", "")


def reduce(trace_csv, out_json):
    with open(trace_csv, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    per_case, tables, current = [], {k: 0 for k in TABLE_KERNELS}, None
    for r in rows:
        name = short_name(r["Kernel_Name"])
        base = name.split("<")[0]
        if base == "bit_reverse_kernel":
            if current is not None:
                per_case.append(current)
            current = []
        elif base in TABLE_KERNELS:
            tables[base] += 1
        elif base in PASS_KERNELS and current is not None:
            wg = [int(r[f"Workgroup_Size_{d}"]) for d in "XYZ"]
            grid = [int(r[f"Grid_Size_{d}"]) // w for d, w in zip("XYZ", wg)]  # the trace counts work-items
            assert wg[1] == wg[2] == 1 and grid[2] == 1
            current.append({"kernel": name, "wg": wg[0], "grid": grid[:2], "lds": int(r["LDS_Block_Size"])})
    assert len(per_case) == len(cases()), (len(per_case), len(cases()))
    kernels = sorted({l["kernel"] for c in per_case for l in c})
    packed = [[[kernels.index(l["kernel"]), l["wg"]] + l["grid"] + [l["lds"]] for l in c] for c in per_case]
    with open(out_json, "w") as f:
        f.write("{\n \"note\": %s,\n \"table_kernels\": %s,\n \"kernels\": %s,\n \"launches\": [\n" % (json.dumps(NOTE), json.dumps(tables), json.dumps(kernels)))
        f.write(",\n".join("  " + json.dumps(packed[i:i + 8], separators=(",", ":"))[1:-1] for i in range(0, len(packed), 8)))
        f.write("\n ]\n}\n")
    print(json.dumps({"cases": len(per_case), "launches": sum(len(x) for x in per_case), "table_kernels": tables}))


NOTE = ("rocprofv3 --kernel-trace of tools/ntt_launch_trace.py run. launches[i] belongs to cases()[i] of that tool, in stream order: [index into kernels, "
        "workgroup size, grid x, grid y (workgroups), LDS bytes as the trace reports them (it reports 0 for dynamic LDS)]")


def load(path):
    """a reduction -> (cases() with their launches as {kernel, wg, grid, lds}, table kernel counts)"""
    doc = json.load(open(path))
    want = cases()
    assert len(doc["launches"]) == len(want), (len(doc["launches"]), len(want))
    full = [dict(c, launches=[{"kernel": doc["kernels"][k], "wg": wg, "grid": [gx, gy], "lds": lds} for k, wg, gx, gy, lds in ls])
            for c, ls in zip(want, doc["launches"])]
    return full, doc["table_kernels"]


def diff(parent_json, this_json, out_json):
    import hashlib

    (a, ta), (b, tb) = load(parent_json), load(this_json)
    differing = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    sha = {t: hashlib.sha256(json.dumps([c["launches"] for c in red]).encode()).hexdigest()[:16] for t, red in (("parent", a), ("this", b))}
    doc = {"note": "tools/ntt_launch_trace.py under rocprofv3 --kernel-trace on the parent commit's tree and on this tree, one MI355X: per-case "
                   "launch lists (kernel with template arguments, workgroup size, grid, LDS) compared entry by entry. The parent's reduction is "
                   "tests/golden/ntt_launches.json; launches_sha256 is over each tree's per-case lists",
           "cases": len(a), "launches": sum(len(c["launches"]) for c in a), "identical": not differing, "differing_cases": differing,
           "launches_sha256": sha, "table_kernels": {"parent": ta, "this": tb}}
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("cases", "launches", "identical", "differing_cases", "table_kernels")}))
    return 0 if doc["identical"] else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "run"
    if mode == "run":
        run()
    elif mode == "reduce":
        reduce(sys.argv[2], sys.argv[3])
    elif mode == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3], sys.argv[4]))
    else:
        sys.exit(__doc__)
