"""Groth16 proof latency on one GPU (include/bx_groth16.h): synthetic keys at 2^20 and 2^22 constraints, or a real zkey + wtns.

    python tools/groth16_bench.py [--log 20,22] [--steps 10] [--warmup 2] [--key K.zkey --wtns W.wtns] [--verify]
    python tools/groth16_bench.py --verify-only          # host only, no GPU: the reference's seal through bx_groth16_verify_seal

Synthetic key: n_vars = n_constraints = 2^k - 2 (domain 2^k), n_public = 1 as in the blake3 circuit, two A entries and one B entry
per constraint; its points are a table of a few thousand generated ones tiled (valid curve points, so the key passes the on-curve
check, but NOT a trusted setup: the proofs do not verify, the work and the timing are those of a real key of this shape).  Two
witnesses: uniform values and a circom-like one (45 % zeros, 45 % ones, the rest uniform).  For each: milliseconds per proof
(median of `steps` blocking proofs after `warmup`) and the per-stage split of one more proof from the ctx's profile events
(bx_profile_enable): upload, coefficient evaluation, NTTs (+ the pointwise kernel), each MSM.  Prints one JSON line per case,
stamped with `device_code_sha`.

--verify: each case also times bx_groth16_verify (host C++) on the proof it made, against the key's own vk (bx_groth16_key_vk).  A
synthetic key's proofs do not verify, so the verdict is reported, not asserted; the work is the same up to the final comparison.
--verify-only: the median of 200 bx_groth16_verify_seal calls (after 20 warm-up) on tests/golden/groth16/blake3_groth16_reference.json,
and beside it the time of tests/bn254_ref.py's big-integer Python verifier on the same vector, with the CPU model.  One JSON line.
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


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform

    return platform.processor() or platform.machine()


def time_verify(g16, vk, proof, steps, warmup):
    """ms per bx_groth16_verify call (median, min, max) and the verdict"""
    from boundless_amd.hal import HalError

    verdict, ts = "accepted", []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        try:
            g16.verify(vk, proof)
        except HalError as e:
            verdict = str(e)
        if i >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    return {"verify_ms_median": round(statistics.median(ts), 3), "verify_ms_min": round(min(ts), 3), "verify_ms_max": round(max(ts), 3),
            "verify_calls": steps, "verify_verdict": verdict}


def verify_only(calls=200, warmup=20):
    import bn254_ref as ref

    from boundless_amd import build, groth16 as g16

    build.build(verbose=False)
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "groth16", "blake3_groth16_reference.json")))
    v = {k: int(x) for k, x in d["vk"].items()}
    g1 = lambda p: [str(v[p + "x"]), str(v[p + "y"]), "1"]
    g2 = lambda p: [[str(v[p + "x2"]), str(v[p + "x1"])], [str(v[p + "y2"]), str(v[p + "y1"])], ["1", "0"]]
    vk = g16.VerifyingKey.from_json(json.dumps({"protocol": "groth16", "curve": "bn128", "nPublic": 1, "vk_alpha_1": g1("alpha"),
                                                "vk_beta_2": g2("beta"), "vk_gamma_2": g2("gamma"), "vk_delta_2": g2("delta"),
                                                "IC": [g1("IC0"), g1("IC1")]}))
    seal, digest = bytes.fromhex(d["seal_hex"]), bytes.fromhex(d["claim_digest_hex"])
    ts = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        g16.verify_seal(vk, seal, digest)  # raises if the reference's seal were refused
        if i >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    vk_again = g16.VerifyingKey.from_json(vk.to_json())
    vk_ms = 1e3 * (time.perf_counter() - t0)
    assert vk_again == vk
    proof = g16.Proof.from_seal(seal)
    rts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ok = ref.verify(vk.as_dict(), proof.as_tuple(), [int.from_bytes(digest, "big") % ref.R])
        rts.append(1e3 * (time.perf_counter() - t0))
        assert ok
    print(json.dumps({"case": "bx_groth16_verify_seal on the reference vector", "verify_seal_ms_median": round(statistics.median(ts), 4),
                      "verify_seal_ms_min": round(min(ts), 4), "verify_seal_ms_max": round(max(ts), 4), "calls": calls, "warmup": warmup,
                      "vk_from_json_ms": round(vk_ms, 3), "bn254_ref_verify_ms_median": round(statistics.median(rts), 1), "bn254_ref_calls": 3,
                      "cpu": cpu_model(), "threads": 1}), flush=True)


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
    ap.add_argument("--verify", action="store_true", help="also time bx_groth16_verify on each case's proof")
    ap.add_argument("--verify-only", action="store_true", help="host only: time bx_groth16_verify_seal on the reference vector")
    a = ap.parse_args()
    if a.verify_only:
        return verify_only()
    from boundless_amd import build, groth16 as g16
    from boundless_amd.hal import HipHal

    hal = HipHal(0)
    stamp = build.device_code_hash()
    if a.key:
        key = g16.Groth16Key(hal, a.key)
        wit = g16.witness_bytes(g16.read_wtns(a.wtns))
        res = run(hal, key, wit, a.steps, a.warmup, "real")
        if a.verify:
            res.update(time_verify(g16, key.vk(), key.prove(wit), a.steps, a.warmup), cpu=cpu_model())
        print(json.dumps(dict(res, info=key.info, device_code_sha=stamp, device=hal.device_name())), flush=True)
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
            wit = witness(n, rng, skew)
            res = run(hal, key, wit, a.steps, a.warmup, f"2^{log_n} {'circom-like (90% 0/1)' if skew else 'uniform'} witness")
            if a.verify:
                res.update(time_verify(g16, key.vk(), key.prove(wit), a.steps, a.warmup), cpu=cpu_model())
            res.update(info=key.info, key_build_s=round(t1 - t0, 2), key_load_s=round(t2 - t1, 2), device_code_sha=stamp, device=hal.device_name(),
                       synthetic=True)
            print(json.dumps(res), flush=True)
        key.free()
        del z
    hal.close()


if __name__ == "__main__":
    main()
