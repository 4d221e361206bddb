"""CPU: the independent BN254 / Groth16 restatement (tests/bn254_ref.py) against the reference's real proof, and the library's host-only
zkey inspection (bx_groth16_zkey_inspect) on synthetic keys and corrupted ones."""
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groth16")


def reference_vector():
    d = json.load(open(os.path.join(GOLDEN, "blake3_groth16_reference.json")))
    v = {k: int(x) for k, x in d["vk"].items()}
    g2 = lambda p: ((v[p + "x2"], v[p + "x1"]), (v[p + "y2"], v[p + "y1"]))  # x1 / y1 are the imaginary parts
    vk = {"alpha1": (v["alphax"], v["alphay"]), "beta2": g2("beta"), "gamma2": g2("gamma"), "delta2": g2("delta"),
          "ic": [(v["IC0x"], v["IC0y"]), (v["IC1x"], v["IC1y"])]}
    seal = bytes.fromhex(d["seal_hex"])
    w = [int.from_bytes(seal[4 + 32 * i:36 + 32 * i], "big") for i in range(8)]
    proof = ((w[0], w[1]), ((w[3], w[2]), (w[5], w[4])), (w[6], w[7]))
    return v, vk, proof, int(d["claim_digest_hex"], 16), seal


def test_golden_manifest():
    import hashlib

    man = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    for name, digest in man["sha256"].items():
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == digest, name


def test_reference_constants_are_bn254():
    v, vk, proof, x, _ = reference_vector()
    assert v["q"] == ref.Q and v["r"] == ref.R
    assert x < ref.R
    A, B, C = proof
    assert ref.on_curve(ref.G1F, A) and ref.on_curve(ref.G1F, C) and ref.on_curve(ref.G2F, B)
    assert all(ref.on_curve(ref.G2F, vk[k]) for k in ("beta2", "gamma2", "delta2"))
    # the EIP-197 order matters: read real part first, B is not on the twist
    assert not ref.on_curve(ref.G2F, ((B[0][1], B[0][0]), (B[1][1], B[1][0])))


def test_reference_proof_verifies_and_public_input_is_bound():
    _, vk, proof, x, _ = reference_vector()
    assert ref.verify(vk, proof, [x])
    assert not ref.verify(vk, proof, [x + 1])


def test_reference_proof_rejected_when_tampered():
    _, vk, proof, x, _ = reference_vector()
    A, B, C = proof
    flat = [A[0], A[1], B[0][0], B[0][1], B[1][0], B[1][1], C[0], C[1]]
    for i in range(8):
        f = list(flat)
        f[i] = (f[i] + 1) % ref.Q
        p = ((f[0], f[1]), ((f[2], f[3]), (f[4], f[5])), (f[6], f[7]))
        assert not ref.verify(vk, p, [x]), f"coordinate {i} changed and still accepted"
    swapped = (A, ((B[0][1], B[0][0]), (B[1][1], B[1][0])), C)
    assert not ref.verify(vk, swapped, [x])
    assert not ref.verify(vk, (C, B, A), [x])


def test_definitional_prover_verifies_on_a_synthetic_key():
    rng = random.Random(7)
    w = ref.random_witness(rng, 10)
    r1 = ref.random_r1cs(rng, w, 2, 8)
    assert r1.satisfied(w)
    s = ref.Setup(r1, 11)
    proof = ref.prove(s, w, 123, 456)
    assert proof == ref.prove(s, w, 123, 456, definitional=False)
    assert ref.verify(s.vk(), proof, w[1:3])


def _key(n_vars=9, n_public=1, n_cons=6, seed=3):
    rng = random.Random(seed)
    w = ref.random_witness(rng, n_vars)
    s = ref.Setup(ref.random_r1cs(rng, w, n_public, n_cons), seed)
    return s, s.zkey()


@pytest.fixture(scope="module")
def g16():
    from boundless_amd import build

    build.build(verbose=False)
    from boundless_amd import groth16

    return groth16


def test_inspect_reads_synthetic_keys(g16, tmp_path):
    for n_vars, n_public, n_cons in ((9, 1, 6), (20, 3, 40), (5, 0, 2)):
        s, z = _key(n_vars, n_public, n_cons)
        info = g16.inspect(z)
        assert info == {"n_vars": n_vars, "n_public": n_public, "domain_size": s.N, "n_coefs": len(s.coefs), "bytes": len(z)}
    p = tmp_path / "k.zkey"
    p.write_bytes(z)
    assert g16.inspect(str(p))["n_vars"] == 5


def _sections(z):
    n, at, out = struct.unpack_from("<I", z, 8)[0], 12, []
    for _ in range(n):
        t, size = struct.unpack_from("<IQ", z, at)
        out.append((t, at + 12, size))
        at += 12 + size
    return out


def test_inspect_refuses_corrupted_keys(g16, tmp_path):
    from boundless_amd.hal import HalError

    _, z = _key()
    secs = {t: (off, size) for t, off, size in _sections(z)}
    h = secs[2][0]
    cases = {
        "bad magic": b"zkez" + z[4:],
        "version": z[:4] + struct.pack("<I", 2) + z[8:],
        "protocol": z[:secs[1][0]] + struct.pack("<I", 2) + z[secs[1][0] + 4:],
        "q is not": z[:h + 4] + (ref.Q + 2).to_bytes(32, "little") + z[h + 36:],
        "r is not": z[:h + 40] + (ref.R - 2).to_bytes(32, "little") + z[h + 72:],
        "truncated": z[:-7],
        "above 2\\^27": z[:h + 80] + struct.pack("<I", 1 << 28) + z[h + 84:],
        "power of two": z[:h + 80] + struct.pack("<I", 24) + z[h + 84:],
    }
    # a short section: H one point short, with the section size and the file made consistent
    t9 = next(i for i, (t, _, _) in enumerate(_sections(z)) if t == 9)
    _, off9, size9 = _sections(z)[t9]
    short = bytearray(z[:off9 - 8] + struct.pack("<Q", size9 - 64) + z[off9:off9 + size9 - 64] + z[off9 + size9:])
    cases["section 9 is"] = bytes(short)
    for what, bad in cases.items():
        with pytest.raises(HalError, match=what):
            g16.inspect(bad)
    with pytest.raises(HalError, match="cannot open"):
        g16.inspect(str(tmp_path / "missing.zkey"))


def test_wtns_round_trip(g16):
    w = [1, 5, ref.R - 1, 0, 123456789]
    assert g16.read_wtns(ref.write_wtns(w)) == w


def test_seal_layout_matches_the_reference(g16):
    """Proof.seal writes the reference's byte layout: rebuilding the reference seal from its own numbers gives the same bytes"""
    _, _, (A, B, C), _, seal = reference_vector()

    from boundless_amd.groth16 import Proof, _Proof, _words

    raw = _Proof()
    for i, v in enumerate([A[0], A[1]]):
        raw.a[8 * i:8 * i + 8] = [int(x) for x in _words(v)]
    for i, v in enumerate([B[0][0], B[0][1], B[1][0], B[1][1]]):
        raw.b[8 * i:8 * i + 8] = [int(x) for x in _words(v)]
    for i, v in enumerate([C[0], C[1]]):
        raw.c[8 * i:8 * i + 8] = [int(x) for x in _words(v)]
    p = Proof(raw)
    assert p.seal(seal[:4]) == seal
    j = json.loads(p.to_json())
    assert j["pi_a"] == [str(A[0]), str(A[1]), "1"] and j["pi_b"][0] == [str(B[0][0]), str(B[0][1])]
    assert j["protocol"] == "groth16" and j["curve"] == "bn128"
