"""Trace-layout kernels at the reference's segment size (include/bx_layout.h, csrc/trace_layout.hip), one process on the MI355X:

    python tools/layout_bench.py --build-variant build/layout_variant      # where hipcc and the library's objects are: the comparison build
    python tools/layout_bench.py [--variant-lib build/layout_variant/libbx_hip_hal.so] [-o profiles/r30_trace_layout.json]

po2 20, noise_rows 1994, stride 19 (A records of 76 bytes = 79.5 MB, the reference's segment size), 38 fields of 16 bits over 38 columns,
w_data 256.  Median of 20 calls by events on one stream after warm-up, in two interleaved rounds:
  (a) layout_place, and its bytes (payload + 4 w_data N) as a fraction of the 6.3 TB/s DESIGN section 4 uses;
  (b) a torch composition on the same device in the same run — a strided view of the payload, shift, mask and (x << 32) % P in int64 per
      field, plus a zero fill of the rest — after the two outputs were compared word for word on the active rows;
  (c) layout_code for 16 columns (first, last, a table column, 13 columns of control words);
  (d) with --variant-lib: layout_place of a library whose kernel reads the records with plain strided loads instead of the LDS tile
      (-DBX_LAYOUT_PLACE_STRIDED, a throw-away build: not a tunable), compared word for word too."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PO2, NOISE, STRIDE, FIELDS, W_DATA, W_CODE, P = 20, 1994, 19, 38, 256, 16, 2013265921
HBM = 6.3e12


def build_variant(out_dir):
    """the library again with trace_layout.hip compiled under -DBX_LAYOUT_PLACE_STRIDED; every other object is the library's own"""
    from boundless_amd import build as b

    b.build(verbose=False)
    os.makedirs(out_dir, exist_ok=True)
    obj = os.path.join(out_dir, "trace_layout.o")
    src = "trace_layout.hip"
    subprocess.run(["hipcc", "-x", "hip"] + b.FLAGS + ["-DBX_LAYOUT_PLACE_STRIDED=1", b.cuid_flag(src), "-c", os.path.join(b.CSRC, src), "-o", obj], check=True)
    objs = [obj if s == src else os.path.join(b.OBJ, s.rsplit(".", 1)[0] + ".o") for s in b.sources()]
    lib = os.path.join(out_dir, "libbx_hip_hal.so")
    subprocess.run(["hipcc", "-shared", "-fPIC", f"--offload-arch={b.ARCH}", "-fno-gpu-rdc", f"-Wl,--version-script={b.EXPORTS}", "-o", lib] + objs, check=True)
    return lib


def the_layout():
    import trace_layout_ref as ref

    t = ref.Layout(STRIDE, NOISE)
    t.col(ref.FIRST).col(ref.LAST).col(ref.ROW, 1 << 15)
    for _ in range(3, W_CODE):
        t.word(ref.LOOKUP_CODE_SEED)
    for c in range(FIELDS):  # two 16-bit halves of each record word
        t.field(c, c // 2, 16 * (c % 2), 16, c)
    return t


class Variant:
    """the few entry points the comparison needs, on a second copy of the library"""

    def __init__(self, path, layout, stream):
        from boundless_amd.circuit import LayoutCodeCol, LayoutField, TraceLayoutDesc
        from boundless_amd.hal import BxBuf

        self.lib, vp = C.CDLL(path), C.c_void_p
        sigs = {"bx_init": [C.c_int, C.POINTER(vp)], "bx_free": [vp], "bx_set_stream": [vp, vp], "bx_trace_layout_create": [C.POINTER(TraceLayoutDesc), C.POINTER(vp)],
                "bx_trace_layout_load": [vp, vp, C.POINTER(vp)], "bx_trace_layout_unload": [vp],
                "bx_trace_layout_place": [vp, vp, C.c_uint32, BxBuf, C.c_size_t, C.c_uint64, BxBuf, C.c_uint32]}
        for name, args in sigs.items():
            getattr(self.lib, name).argtypes, getattr(self.lib, name).restype = args, C.c_char_p
        self.ctx, self.layout, self.dev = vp(), vp(), vp()
        self._ok(self.lib.bx_init(0, C.byref(self.ctx)))
        self._ok(self.lib.bx_set_stream(self.ctx, stream))
        code = (LayoutCodeCol * len(layout.code))(*[LayoutCodeCol(*c) for c in layout.code])
        fields = (LayoutField * len(layout.fields))(*[LayoutField(*f) for f in layout.fields])
        desc = TraceLayoutDesc(code, len(layout.code), None, 0, fields, len(layout.fields), layout.stride, layout.noise_rows, 0)
        self._ok(self.lib.bx_trace_layout_create(C.byref(desc), C.byref(self.layout)))
        self._ok(self.lib.bx_trace_layout_load(self.ctx, self.layout, C.byref(self.dev)))

    @staticmethod
    def _ok(msg):
        if msg:
            raise RuntimeError(msg.decode())

    def place(self, seg, seg_len, noise, data):
        self._ok(self.lib.bx_trace_layout_place(self.ctx, self.dev, PO2, seg, seg_len, noise, data, W_DATA))

    def close(self):
        self._ok(self.lib.bx_trace_layout_unload(self.dev))
        self.lib.bx_free(self.ctx)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build-variant", metavar="DIR")
    ap.add_argument("--variant-lib")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "r30_trace_layout.json"))
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args(argv)
    if a.build_variant:
        print(build_variant(a.build_variant))
        return 0

    import torch
    import trace_layout_ref as ref

    from boundless_amd import build as b
    from boundless_amd.hal import BxBuf, HipHal

    hal = HipHal(0)
    side = torch.cuda.Stream()  # one stream for the library's launches, torch's and the events
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    hal.set_stream(stream)
    layout = the_layout()
    compiled = ref.compile_ref(layout)
    loaded = compiled.load(hal)
    n, act = 1 << PO2, ref.active_rows(PO2, NOISE)
    recs = np.random.default_rng(20).integers(0, 1 << 32, (act, STRIDE), dtype=np.uint64).astype(np.uint32)
    seg = ref.segment_bytes(PO2, 0xB0D1E55, recs)
    seg_t = torch.from_numpy(np.frombuffer(seg, "<u4").view(np.int32).copy()).cuda()
    out_t = torch.empty(W_DATA * n, dtype=torch.int32, device="cuda")
    twin_t = torch.empty(W_DATA, n, dtype=torch.int32, device="cuda")
    code_t = torch.empty(W_CODE * n, dtype=torch.int32, device="cuda")
    dseg, data, code = hal.wrap(seg_t.data_ptr(), seg_t.numel()), hal.wrap(out_t.data_ptr(), out_t.numel()), hal.wrap(code_t.data_ptr(), code_t.numel())
    noise = 12345

    def place():
        loaded.place(PO2, dseg, len(seg), noise, data, W_DATA)

    def torch_twin():
        pay = seg_t[7:7 + act * STRIDE].view(act, STRIDE)
        twin_t.zero_()
        for col, word, shift, bits, _pad in layout.fields:
            x = pay[:, word].to(torch.int64) & 0xFFFFFFFF
            twin_t[col, :act] = ((((x >> shift) & ((1 << bits) - 1)) << 32) % P).to(torch.int32)

    def code_fill():
        loaded.code(PO2, code)

    runs = {"layout_place": place, "torch_composition": torch_twin, "layout_code": code_fill}
    variant = None
    if a.variant_lib:
        variant = Variant(a.variant_lib, layout, stream)
        var_t = torch.empty(W_DATA * n, dtype=torch.int32, device="cuda")
        vseg, vdata = BxBuf(seg_t.data_ptr(), seg_t.numel()), BxBuf(var_t.data_ptr(), var_t.numel())
        runs["layout_place_strided_loads"] = lambda: variant.place(vseg, len(seg), noise, vdata)

    # the outputs agree before anything is timed
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    got = out_t.view(W_DATA, n)
    assert torch.equal(got[:, :act], twin_t[:, :act]), "layout_place and the torch composition differ on the active rows"
    host = compiled.data_host(PO2, seg, W_DATA, noise)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), host), "layout_place differs from the host fill"
    assert np.array_equal(code_t.cpu().numpy().view(np.uint32).reshape(W_CODE, n), compiled.code_host(PO2)), "layout_code differs from the host fill"
    if variant:
        assert torch.equal(var_t, out_t), "the strided-load build differs from the library's"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for fn in runs.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _round in range(2):  # interleaved: every round times every form
        for k, fn in runs.items():
            times[k] += [timed(fn) for _ in range(a.calls // 2)]
    med = {k: statistics.median(v) for k, v in times.items()}
    place_bytes = len(seg) - 28 + 4 * W_DATA * n
    result = {"tool": "tools/layout_bench.py", "device": hal.device_name(), "device_code_hash": b.device_code_hash(),
              "shape": {"po2": PO2, "noise_rows": NOISE, "stride": STRIDE, "records": act, "fields": FIELDS, "field_bits": 16, "w_data": W_DATA, "w_code": W_CODE,
                        "payload_bytes": len(seg) - 28},
              "calls": a.calls, "rounds": 2,
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
              "layout_place_bytes": place_bytes, "layout_place_fraction_of_6.3TBps": round(place_bytes / (med["layout_place"] * 1e-3) / HBM, 4),
              "layout_code_bytes": 4 * W_CODE * n, "layout_code_fraction_of_6.3TBps": round(4 * W_CODE * n / (med["layout_code"] * 1e-3) / HBM, 4),
              "layout_place_over_torch": round(med["layout_place"] / med["torch_composition"], 4)}
    if variant:
        result["lds_tile_over_strided_loads"] = round(med["layout_place"] / med["layout_place_strided_loads"], 4)
        variant.close()
    loaded.unload()
    hal.close()
    print(json.dumps(result))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
