"""Groth16 proof latency on one GPU (include/bx_groth16.h): synthetic keys at 2^20 and 2^22 constraints, or a real zkey + wtns.

    python tools/groth16_bench.py [--log 20,22] [--steps 10] [--warmup 2] [--key K.zkey --wtns W.wtns]

Synthetic key: n_vars = n_constraints = 2^k - 2 (domain 2^k), n_public = 1 as in the blake3 circuit, two A entries and one B entry
per constraint; its points are a table of a few thousand generated ones tiled (valid curve points, so the key passes the on-curve
check, but NOT a trusted setup: the proofs do not verify, the work and the timing are those of a real key of this shape).  Two
witnesses: uniform values and a circom-like one (45 % zeros, 45 % ones, the rest uniform).  For each: milliseconds per proof
(median of `steps` blocking proofs after `warmup`) and the per-stage split of one more proof from the ctx's profile events
(bx_profile_enable): upload, coefficient evaluation, NTTs (+ the pointwise kernel), each MSM.  Prints one JSON line per case,
stamped with `device_code_sha`.
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _sec(t, data):
    return struct.pack("<IQ", t, len(data)) + data


def synthetic_zkey(log_n, rng, t1=2048, t2=256):
    import bn254_ref as ref

    from boundless_amd import groth16 as g16

    N = 1 << log_n
    ncons = N - 2
    n, npub = ncons, 1
    ks = [int(x) for x in rng.integers(1, 1 << 62, size=t1)]
    g1 = g16.g1_words(ref.fixed_base(1).many(ks)).reshape(t1, 16)
    g2 = g16.g2_words(ref.fixed_base(2).many(ks[:t2])).reshape(t2, 32)
    tile1 = lambda k: np.resize(g1, (k, 16)).tobytes()
    tile2 = lambda k: np.resize(g2, (k, 32)).tobytes()
    hdr = (struct.pack("<I", 32) + ref.Q.to_bytes(32, "little") + struct.pack("<I", 32) + ref.R.to_bytes(32, "little")
           + struct.pack("<III", n, npub, N) + tile1(2) + tile2(1) + tile2(1) + tile1(1) + tile2(1))
    dt = np.dtype([("m", "<u4"), ("c", "<u4"), ("s", "<u4"), ("v", "<u4", 8)])
    m = 3 * ncons + npub + 1
    co = np.zeros(m, dt)
    cons = np.arange(ncons, dtype=np.uint32)
    co["m"][:3 * ncons] = np.concatenate([np.zeros(2 * ncons, np.uint32), np.ones(ncons, np.uint32)])
    co["c"][:3 * ncons] = np.concatenate([cons, cons, cons])
    co["s"][:3 * ncons] = rng.integers(0, n, size=3 * ncons, dtype=np.uint32)
    v = rng.integers(0, 1 << 32, size=(3 * ncons, 8), dtype=np.uint64).astype(np.uint32)
    v[:, 7] &= 0x1FFFFFFF
    co["v"][:3 * ncons] = v
    co["c"][3 * ncons:] = ncons + np.arange(npub + 1, dtype=np.uint32)  # the public signals' A-rows
    co["s"][3 * ncons:] = np.arange(npub + 1, dtype=np.uint32)
    co["v"][3 * ncons:, 0] = 1
    secs = [(1, struct.pack("<I", 1)), (2, hdr), (3, tile1(npub + 1)), (4, struct.pack("<I", m) + co.tobytes()), (5, tile1(n)),
            (6, tile1(n)), (7, tile2(n)), (8, tile1(n - npub - 1)), (9, tile1(N)), (10, b"")]
    return b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(_sec(t, d) for t, d in secs)


def witness(n, rng, skew):
    w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 7] &= 0x1FFFFFFF
    if skew:
        u = rng.random(n)
        w[u < 0.9] = 0
        w[u < 0.45, 0] = 1
    w[0] = 0
    w[0, 0] = 1
    return w.tobytes()


def run(hal, key, wit, steps, warmup, label):
    rs = (12345).to_bytes(32, "little") + (67890).to_bytes(32, "little")
    r, s = int.from_bytes(rs[:32], "little"), int.from_bytes(rs[32:], "little")
    for _ in range(warmup):
        key.prove(wit, r, s)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        key.prove(wit, r, s)
        ts.append(1e3 * (time.perf_counter() - t0))
    hal.profile_reset()
    hal.profile_enable(True)
    key.prove(wit, r, s)
    prof = hal.profile_report()
    hal.profile_enable(False)
    hal.profile_reset()
    stages = {k: {"calls": v["calls"], "ms": round(v["ms"], 3)} for k, v in prof.items()}
    return {"case": label, "ms_per_proof_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
            "steps": steps, "warmup": warmup, "stages": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default="20,22")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--key")
    ap.add_argument("--wtns")
    a = ap.parse_args()
    from boundless_amd import build, groth16 as g16
    from boundless_amd.hal import HipHal

    hal = HipHal(0)
    stamp = build.device_code_hash()
    if a.key:
        key = g16.Groth16Key(hal, a.key)
        wit = g16.witness_bytes(g16.read_wtns(a.wtns))
        print(json.dumps(dict(run(hal, key, wit, a.steps, a.warmup, "real"), info=key.info, device_code_sha=stamp, device=hal.device_name())), flush=True)
        key.free()
        return
    for log_n in map(int, a.log.split(",")):
        rng = np.random.default_rng(log_n)
        t0 = time.perf_counter()
        z = synthetic_zkey(log_n, rng)
        t1 = time.perf_counter()
        key = g16.Groth16Key(hal, z)
        t2 = time.perf_counter()
        n = key.info["n_vars"]
        for skew in (False, True):
            res = run(hal, key, witness(n, rng, skew), a.steps, a.warmup, f"2^{log_n} {'circom-like (90% 0/1)' if skew else 'uniform'} witness")
            res.update(info=key.info, key_build_s=round(t1 - t0, 2), key_load_s=round(t2 - t1, 2), device_code_sha=stamp, device=hal.device_name(),
                       synthetic=True)
            print(json.dumps(res), flush=True)
        key.free()
        del z
    hal.close()


if __name__ == "__main__":
    main()
