"""CPU: the library's host Groth16 verifier (bx_groth16_verify*, bx_groth16_vk*, the seal codec, bx_bn254_pairing_check) against the
reference's own proof (tests/golden/groth16/blake3_groth16_reference.json) and against the independent restatement
tests/bn254_ref.py.  No GPU: everything here is host C++ behind the C ABI."""
import json
import os
import random
import struct
import sys
import threading

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groth16")
Q, R = ref.Q, ref.R


@pytest.fixture(scope="module")
def g16():
    from boundless_amd import build

    build.build(verbose=False)
    from boundless_amd import groth16

    return groth16


@pytest.fixture(scope="module")
def HalError():
    from boundless_amd.hal import HalError as E

    return E


# ---- helpers ----
def vk_json(vk, n_public=None, extra=None):
    """a snarkjs verification_key.json from a dict in the shape of bn254_ref.Setup.vk()"""
    g1 = lambda p: ["0", "1", "0"] if p is None else [str(p[0]), str(p[1]), "1"]
    g2 = lambda p: [[str(p[0][0]), str(p[0][1])], [str(p[1][0]), str(p[1][1])], ["1", "0"]]
    d = {"protocol": "groth16", "curve": "bn128", "nPublic": len(vk["ic"]) - 1 if n_public is None else n_public,
         "vk_alpha_1": g1(vk["alpha1"]), "vk_beta_2": g2(vk["beta2"]), "vk_gamma_2": g2(vk["gamma2"]), "vk_delta_2": g2(vk["delta2"]),
         "IC": [g1(p) for p in vk["ic"]]}
    d.update(extra or {})
    return json.dumps(d)


def reference_vector():
    d = json.load(open(os.path.join(GOLDEN, "blake3_groth16_reference.json")))
    v = {k: int(x) for k, x in d["vk"].items()}
    g2 = lambda p: ((v[p + "x2"], v[p + "x1"]), (v[p + "y2"], v[p + "y1"]))  # x1 / y1 are the imaginary parts
    vk = {"alpha1": (v["alphax"], v["alphay"]), "beta2": g2("beta"), "gamma2": g2("gamma"), "delta2": g2("delta"),
          "ic": [(v["IC0x"], v["IC0y"]), (v["IC1x"], v["IC1y"])]}
    return vk, bytes.fromhex(d["seal_hex"]), bytes.fromhex(d["claim_digest_hex"])


def make_proof(g16, abc, public):
    """a library Proof from integer affine points (A, B, C) and public signals, through the snarkjs JSON reader"""
    A, B, C = abc
    pj = json.dumps({"pi_a": [str(A[0]), str(A[1]), "1"], "pi_b": [[str(B[0][0]), str(B[0][1])], [str(B[1][0]), str(B[1][1])], ["1", "0"]],
                     "pi_c": [str(C[0]), str(C[1]), "1"], "protocol": "groth16", "curve": "bn128"})
    return g16.Proof.from_json(pj, json.dumps([str(x) for x in public]))


def native_verdict(g16, HalError, vk, proof):
    """True / False like bn254_ref.verify; the message of a refusal is returned too"""
    try:
        g16.verify(vk, proof)
        return True, None
    except HalError as e:
        return False, str(e)


def setup_for(n_vars, n_public, n_cons, seed):
    rng = random.Random(seed)
    w = ref.random_witness(rng, n_vars)
    return ref.Setup(ref.random_r1cs(rng, w, n_public, n_cons), seed), w


def f2sqrt(a):
    """a square root in Fq2 (q = 3 mod 4), or None when a is not a square"""
    if a == (0, 0):
        return a
    a1 = ref.f2pow(a, (Q - 3) // 4)
    alpha = ref.f2mul(ref.f2mul(a1, a1), a)
    x0 = ref.f2mul(a1, a)
    if alpha == (Q - 1, 0):
        x = ref.f2mul((0, 1), x0)
    else:
        x = ref.f2mul(ref.f2pow(ref.f2add((1, 0), alpha), (Q - 1) // 2), x0)
    return x if ref.f2mul(x, x) == a else None


def twist_point_outside_subgroup(seed):
    rng = random.Random(seed)
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = f2sqrt(ref.f2add(ref.f2mul(ref.f2mul(x, x), x), ref.B2))
        if y is None:
            continue
        P = (x, y)
        assert ref.on_curve(ref.G2F, P)
        if ref.mul(ref.G2F, P, R) is not None:
            return P


# ---- 1. the reference's own proof ----
@pytest.fixture(scope="module")
def refvec(g16):
    vk, seal, digest = reference_vector()
    return g16.VerifyingKey.from_json(vk_json(vk)), seal, digest


def test_reference_seal_is_accepted_with_and_without_its_selector(g16, refvec):
    vk, seal, digest = refvec
    assert len(seal) == 260 and len(digest) == 32
    assert g16.verify_seal(vk, seal, digest) is None
    assert g16.verify_seal(vk, seal[4:], digest) is None


def _tampered(seal, digest, how):
    w = [int.from_bytes(seal[4 + 32 * i:36 + 32 * i], "big") for i in range(8)]
    if how.startswith("coordinate"):
        i = int(how[-1])
        w[i] = (w[i] + 1) % Q
    elif how == "B parts swapped":
        w[2], w[3], w[4], w[5] = w[3], w[2], w[5], w[4]
    elif how == "A and C exchanged":
        w[0], w[1], w[6], w[7] = w[6], w[7], w[0], w[1]
    elif how == "digest + 1":
        digest = (int.from_bytes(digest, "big") + 1).to_bytes(32, "big")
    return seal[:4] + b"".join(x.to_bytes(32, "big") for x in w), digest


REFUSALS = [f"coordinate {i}" for i in range(8)] + ["B parts swapped", "A and C exchanged", "digest + 1"]


@pytest.mark.parametrize("how", REFUSALS)
def test_reference_seal_is_refused_when_tampered(g16, HalError, refvec, how):
    vk, seal, digest = refvec
    bad_seal, bad_digest = _tampered(seal, digest, how)
    assert (bad_seal, bad_digest) != (seal, digest)
    with pytest.raises(HalError, match="bx_groth16_verify_seal"):
        g16.verify_seal(vk, bad_seal, bad_digest)
    with pytest.raises(HalError):
        g16.verify_seal(vk, bad_seal[4:], bad_digest)


def test_reference_seal_is_refused_at_other_lengths(g16, HalError, refvec):
    vk, seal, digest = refvec
    for bad in (seal[:-1], seal + b"\0", seal[4:-1], seal[:128], b""):
        with pytest.raises(HalError, match="260 bytes"):
            g16.verify_seal(vk, bad, digest)
        with pytest.raises(HalError, match="260 bytes"):
            g16.Proof.from_seal(bad)


def test_verify_seal_reduces_the_digest_mod_r(g16, HalError, refvec):
    """the reference reads the digest with from_be_bytes_mod_order: digest + r is the same public input; bx_groth16_verify is strict"""
    vk, seal, digest = refvec
    x = int.from_bytes(digest, "big")
    assert x + R < 1 << 256
    assert g16.verify_seal(vk, seal, (x + R).to_bytes(32, "big")) is None
    p = g16.Proof.from_seal(seal, [x])
    assert g16.verify(vk, p) is None
    with pytest.raises(HalError, match="public signal 0 is not below r"):
        g16.verify(vk, g16.Proof.from_seal(seal, [x + R]))


# ---- 2. agreement with the independent restatement ----
KEYS = [(8, 0, 6, 101), (9, 1, 6, 102), (12, 3, 10, 103), (14, 5, 12, 104), (10, 1, 9, 105)]


@pytest.fixture(scope="module")
def setups():
    out = []
    for n_vars, n_public, n_cons, seed in KEYS:
        s, w = setup_for(n_vars, n_public, n_cons, seed)
        proof = ref.prove(s, w, 1000 + seed, 2000 + seed)
        other = ref.prove(s, w, 3000 + seed, 4000 + seed)
        out.append((s, w, proof, other))
    return out


def test_zkey_vk_equals_the_setups_vk(g16, setups, tmp_path):
    for s, _, _, _ in setups:
        z = s.zkey()
        vk = g16.VerifyingKey.from_zkey(z)
        assert vk.as_dict() == s.vk()
        assert vk.n_public == s.r1cs.n_public
    p = tmp_path / "k.zkey"
    p.write_bytes(z)
    assert g16.VerifyingKey.from_zkey(str(p)).as_dict() == s.vk()


def test_honest_proofs_are_accepted_and_mutations_judged_like_the_restatement(g16, HalError, setups):
    vks = [g16.VerifyingKey.from_zkey(s.zkey()) for s, _, _, _ in setups]
    verdicts, n_mut = set(), 0
    for ki, (s, w, proof, other) in enumerate(setups):
        npub = s.r1cs.n_public
        pub = w[1:npub + 1]
        vk, vkd = vks[ki], s.vk()
        for pr in (proof, other):
            assert ref.verify(vkd, pr, pub)
            assert native_verdict(g16, HalError, vk, make_proof(g16, pr, pub)) == (True, None)
        A, B, C = proof
        rng = random.Random(7000 + ki)
        k = rng.randrange(2, R)
        nk = (ki + 1) % len(setups)
        swapped = dict(vkd, gamma2=vkd["delta2"], delta2=vkd["gamma2"])
        cases = [
            ("A <- C", vk, vkd, (C, B, C), pub),
            ("C <- A", vk, vkd, (A, B, A), pub),
            ("B <- another proof's B", vk, vkd, (A, other[1], C), pub),
            ("A <- a random point", vk, vkd, (ref.mul(ref.G1F, ref.G1_GEN, rng.randrange(1, R)), B, C), pub),
            ("C <- -C", vk, vkd, (A, B, ref.neg(ref.G1F, C)), pub),
            ("another key's vk", vks[nk], setups[nk][0].vk(), proof, pub),
            ("gamma2 and delta2 exchanged", g16.VerifyingKey.from_json(vk_json(swapped)), swapped, proof, pub),
            # Groth16 proofs are malleable: (kA, B/k, C) is another valid proof
            ("A <- kA, B <- B/k", vk, vkd, (ref.mul(ref.G1F, A, k), ref.mul(ref.G2F, B, ref.inv(k, R)), C), pub),
            ("A <- -A, B <- -B", vk, vkd, (ref.neg(ref.G1F, A), ref.neg(ref.G2F, B), C), pub),
        ]
        for i in range(npub):
            cases.append((f"public signal {i} changed", vk, vkd, proof, pub[:i] + [(pub[i] + 1 + i) % R] + pub[i + 1:]))
        for name, nvk, rvk, pr, pb in cases:
            want = ref.verify(rvk, pr, pb)
            got, msg = native_verdict(g16, HalError, nvk, make_proof(g16, pr, pb))
            assert got == want, f"key {ki}, {name}: native {got} ({msg}), restatement {want}"
            verdicts.add(got)
            n_mut += 1
    assert n_mut >= 40
    assert verdicts == {True, False}


# ---- 3. where native is stricter than the restatement ----
def test_strict_input_checks_name_the_failed_check(g16, HalError, setups):
    s, w, proof, _ = setups[1]
    vk = g16.VerifyingKey.from_zkey(s.zkey())
    A, B, C = proof
    pub = w[1:2]
    P = twist_point_outside_subgroup(1)
    assert ref.mul(ref.G2F, P, R) is not None
    with pytest.raises(HalError, match="B is not in the subgroup"):
        g16.verify(vk, make_proof(g16, (A, P, C), pub))
    with pytest.raises(HalError, match="A has a coordinate not below q"):
        g16.verify(vk, make_proof(g16, ((Q, A[1]), B, C), pub))
    with pytest.raises(HalError, match="B has a coordinate not below q"):
        g16.verify(vk, make_proof(g16, (A, ((B[0][0], Q), B[1]), C), pub))
    with pytest.raises(HalError, match="C has a coordinate not below q"):
        g16.verify(vk, make_proof(g16, (A, B, (C[0], Q + 5)), pub))
    with pytest.raises(HalError, match="public signal 0 is not below r"):
        g16.verify(vk, make_proof(g16, proof, [R]))
    with pytest.raises(HalError, match="A is the point at infinity"):
        g16.verify(vk, make_proof(g16, ((0, 0), B, C), pub))
    with pytest.raises(HalError, match="B is the point at infinity"):
        g16.verify(vk, make_proof(g16, (A, ((0, 0), (0, 0)), C), pub))
    with pytest.raises(HalError, match="C is the point at infinity"):
        g16.verify(vk, make_proof(g16, (A, B, (0, 0)), pub))
    with pytest.raises(HalError, match="A is not on the curve"):
        g16.verify(vk, make_proof(g16, ((A[0], (A[1] + 1) % Q), B, C), pub))
    with pytest.raises(HalError, match="B is not on the curve"):
        g16.verify(vk, make_proof(g16, (A, (B[0], (B[1][1], B[1][0])), C), pub))
    with pytest.raises(HalError, match="C is not on the curve"):
        g16.verify(vk, make_proof(g16, (A, B, (C[1], C[0])), pub))
    with pytest.raises(HalError, match="n_public mismatch"):
        g16.verify(vk, make_proof(g16, proof, pub + [1]))
    with pytest.raises(HalError, match="n_public mismatch"):
        g16.verify(vk, make_proof(g16, proof, []))
    with pytest.raises(HalError, match="pairing check failed"):
        g16.verify(vk, make_proof(g16, proof, [(pub[0] + 1) % R]))
    assert g16.verify(vk, make_proof(g16, proof, pub)) is None


# ---- 4. bx_bn254_pairing_check ----
def test_pairing_check_is_bilinear(g16, HalError):
    rng = random.Random(404)
    G1, G2 = ref.G1_GEN, ref.G2_GEN
    for _ in range(3):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        P, Qp = ref.mul(ref.G1F, G1, a), ref.mul(ref.G2F, G2, b)
        assert g16.pairing_check([P, ref.mul(ref.G1F, G1, (-a * b) % R)], [Qp, G2])
        assert not g16.pairing_check([P, ref.mul(ref.G1F, G1, (-a * b + 1) % R)], [Qp, G2])
        assert not g16.pairing_check([P], [Qp])
        # e(aG, bH) e(-G, abH) = 1 as well: bilinear in the second argument
        assert g16.pairing_check([P, ref.neg(ref.G1F, G1)], [Qp, ref.mul(ref.G2F, G2, a * b % R)])
    assert g16.pairing_check([], [])
    assert g16.pairing_check([None], [G2]) and g16.pairing_check([G1], [None]) and g16.pairing_check([None, G1], [None, None])
    assert g16.pairing_check([P, None, ref.neg(ref.G1F, P), G1], [Qp, G2, Qp, None])
    assert not g16.pairing_check([P, None], [Qp, G2])
    # 40 pairs: more than one chunk of the multi-Miller loop
    ps = [ref.mul(ref.G1F, G1, i + 2) for i in range(20)]
    assert g16.pairing_check(ps + [ref.neg(ref.G1F, p) for p in ps], [G2] * 40)
    assert not g16.pairing_check(ps + [ref.neg(ref.G1F, p) for p in ps[:-1]] + [ps[0]], [G2] * 40)
    with pytest.raises(HalError, match="G2 point 0 is not in the subgroup"):
        g16.pairing_check([G1], [twist_point_outside_subgroup(2)])
    with pytest.raises(HalError, match="G1 point 1 is not on the curve"):
        g16.pairing_check([G1, (1, 3)], [G2, G2])
    with pytest.raises(HalError, match="not below q"):
        g16.pairing_check([(1 + Q, 2)], [G2])


def test_pairing_agrees_with_the_restatement_on_random_products(g16):
    """three-pair products that are 1 by construction, and the same with one scalar off, against bn254_ref's own pairing"""
    rng = random.Random(405)
    for _ in range(2):
        a, b, c, d = (rng.randrange(1, R) for _ in range(4))
        e = (-(a * b + c * d)) % R
        g1 = [ref.mul(ref.G1F, ref.G1_GEN, k) for k in (a, c, e)]
        g2 = [ref.mul(ref.G2F, ref.G2_GEN, k) for k in (b, d, 1)]
        assert ref.pairing_product_is_one(list(zip(g1, g2))) and g16.pairing_check(g1, g2)
        g1[2] = ref.mul(ref.G1F, ref.G1_GEN, (e + 1) % R)
        assert not g16.pairing_check(g1, g2)


# ---- 5. round trips ----
def test_round_trips(g16, setups, refvec):
    for s, w, proof, _ in setups:
        vk = g16.VerifyingKey.from_zkey(s.zkey())
        text = vk.to_json()
        d = json.loads(text)
        assert d["protocol"] == "groth16" and d["curve"] == "bn128" and d["nPublic"] == s.r1cs.n_public
        assert len(d["IC"]) == s.r1cs.n_public + 1 and d["vk_alpha_1"][2] == "1" and d["vk_beta_2"][2] == ["1", "0"]
        assert d["vk_gamma_2"][0] == [str(s.gamma2[0][0]), str(s.gamma2[0][1])] and "vk_alphabeta_12" not in d
        again = g16.VerifyingKey.from_json(text)
        assert again == vk and again.as_dict() == s.vk() and again.to_json() == text
        # unknown keys and vk_alphabeta_12 are ignored
        d["vk_alphabeta_12"] = [[["1", "2"]]]
        d["comment"] = {"nested": [1, 2.5, True, None, 'x"y']}
        assert g16.VerifyingKey.from_json(json.dumps(d, indent=1)) == vk
        pub = w[1:s.r1cs.n_public + 1]
        p = make_proof(g16, proof, pub)
        assert p.as_tuple() == proof and p.public == pub
        p2 = g16.Proof.from_json(p.to_json(), p.public_json())
        assert p2.as_tuple() == proof and p2.public == pub and p2.to_json() == p.to_json()
        seal = p.seal(b"\x01\x02\x03\x04")
        assert len(seal) == 260 and seal[:4] == b"\x01\x02\x03\x04"
        p3 = g16.Proof.from_seal(seal, pub)
        assert p3.as_tuple() == proof and p3.public == pub and p3.seal(b"\x01\x02\x03\x04") == seal
        assert g16.Proof.from_seal(seal[4:]).as_tuple() == proof and g16.Proof.from_seal(seal).public == []
    _, seal, digest = refvec
    p = g16.Proof.from_seal(seal)
    assert p.seal(seal[:4]) == seal  # the reference's seal, byte for byte
    w = [int.from_bytes(seal[4 + 32 * i:36 + 32 * i], "big") for i in range(8)]
    assert p.as_tuple() == ((w[0], w[1]), ((w[3], w[2]), (w[5], w[4])), (w[6], w[7]))


def test_json_buffers_too_small_are_refused(g16, HalError, setups):
    import ctypes as C

    vk = g16.VerifyingKey.from_zkey(setups[0][0].zkey())
    buf = C.create_string_buffer(64)
    msg = g16._lib().bx_groth16_vk_json(C.byref(vk._raw), buf, len(buf))
    assert msg and b"too small" in msg


# ---- 6. refusals of bad keys ----
def test_bad_verifying_keys_are_refused(g16, HalError, setups):
    s = setups[2][0]
    good = s.vk()
    assert g16.VerifyingKey.from_json(vk_json(good)).as_dict() == good
    x, y = good["ic"][1]
    with pytest.raises(HalError, match=r"IC\[1\] is not on the curve"):
        g16.VerifyingKey.from_json(vk_json(dict(good, ic=[good["ic"][0], (x, (y + 1) % Q)] + good["ic"][2:])))
    P = twist_point_outside_subgroup(3)
    with pytest.raises(HalError, match="gamma2 is not in the subgroup"):
        g16.VerifyingKey.from_json(vk_json(dict(good, gamma2=P)))
    with pytest.raises(HalError, match="delta2 is not on the curve"):
        g16.VerifyingKey.from_json(vk_json(dict(good, delta2=(good["delta2"][1], good["delta2"][0]))))
    with pytest.raises(HalError, match="beta2 is the point at infinity"):
        g16.VerifyingKey.from_json(vk_json(dict(good, beta2=((0, 0), (0, 0)))))
    with pytest.raises(HalError, match="alpha1 has a coordinate not below q"):
        g16.VerifyingKey.from_json(vk_json(dict(good, alpha1=(good["alpha1"][0] + Q, good["alpha1"][1]))))
    with pytest.raises(HalError, match="nPublic is 2"):
        g16.VerifyingKey.from_json(vk_json(good, n_public=2))
    ic66 = [ref.mul(ref.G1F, ref.G1_GEN, i + 1) for i in range(66)]
    with pytest.raises(HalError, match="65 public signals, more than BX_GROTH16_MAX_PUBLIC"):
        g16.VerifyingKey.from_json(vk_json(dict(good, ic=ic66)))
    assert g16.VerifyingKey.from_json(vk_json(dict(good, ic=ic66[:65]))).n_public == 64  # the largest key
    for bad in ("", "[1, 2]", vk_json(good)[:-1], vk_json(good) + "x", vk_json(good).replace('"groth16"', '"plonk"')):
        with pytest.raises(HalError, match="bx_groth16_vk_from_json"):
            g16.VerifyingKey.from_json(bad)
    with pytest.raises(HalError, match="not a decimal number"):
        g16.VerifyingKey.from_json(vk_json(good).replace(str(good["alpha1"][0]), "0x12"))


def _sections(z):
    n, at, out = struct.unpack_from("<I", z, 8)[0], 12, {}
    for _ in range(n):
        t, size = struct.unpack_from("<IQ", z, at)
        out[t] = (at + 12, size)
        at += 12 + size
    return out


def test_bad_zkeys_are_refused(g16, HalError, setups, tmp_path):
    s = setups[2][0]
    z = s.zkey()
    off3, size3 = _sections(z)[3]
    with pytest.raises(HalError, match="truncated"):
        g16.VerifyingKey.from_zkey(z[:off3 + size3 // 2])
    with pytest.raises(HalError, match="bad magic"):
        g16.VerifyingKey.from_zkey(b"zkez" + z[4:])
    with pytest.raises(HalError, match="cannot open"):
        g16.VerifyingKey.from_zkey(str(tmp_path / "missing.zkey"))
    # an IC point off its curve, gamma2 replaced by a twist point outside the subgroup (Montgomery form, as the file holds them)
    y = int.from_bytes(z[off3 + 96:off3 + 128], "little")
    with pytest.raises(HalError, match=r"IC\[1\] is not on the curve"):
        g16.VerifyingKey.from_zkey(z[:off3 + 96] + ((y + 1) % Q).to_bytes(32, "little") + z[off3 + 128:])
    off2, _ = _sections(z)[2]
    with pytest.raises(HalError, match="gamma2 is not in the subgroup"):
        g16.VerifyingKey.from_zkey(z[:off2 + 340] + ref.g2_bytes(twist_point_outside_subgroup(4)) + z[off2 + 468:])
    with pytest.raises(HalError, match="alpha1 has a coordinate not below q"):
        g16.VerifyingKey.from_zkey(z[:off2 + 84] + Q.to_bytes(32, "little") + z[off2 + 116:])
    # a damaged point section does not matter: only sections 2 and 3 are read
    off7, _ = _sections(z)[7]
    assert g16.VerifyingKey.from_zkey(z[:off7] + bytes(64) + z[off7 + 64:]).as_dict() == s.vk()


# ---- 7. threads ----
def test_eight_threads_verify_concurrently(g16, HalError, refvec):
    vk, seal, digest = refvec
    tampered = [_tampered(seal, digest, how) for how in ("digest + 1", "coordinate 1", "coordinate 3", "A and C exchanged")]
    expect = ["pairing check failed", "A is not on the curve", "B is not on the curve", "pairing check failed"]
    errors = []

    def worker(t):
        bad_seal, bad_digest = tampered[t % 4]
        try:
            for _ in range(50):
                assert g16.verify_seal(vk, seal, digest) is None
                try:
                    g16.verify_seal(vk, bad_seal, bad_digest)
                    errors.append((t, "a tampered seal was accepted"))
                except HalError as e:
                    if expect[t % 4] not in str(e):
                        errors.append((t, str(e)))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]
