"""GPU: proofs made by the device prover (bx_groth16_prove) checked by the library's own host verifier (bx_groth16_verify), with the
verifying key taken from the loaded key (bx_groth16_key_vk), from the zkey bytes and from the setup."""
import glob
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402

from boundless_amd import groth16 as g16  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402

pytestmark = pytest.mark.gpu
R = ref.R
UPSTREAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groth16", "upstream")


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def setup_for(n_vars, n_public, n_cons, kind, seed):
    rng = random.Random(seed)
    w = ref.random_witness(rng, n_vars, kind)
    return ref.Setup(ref.random_r1cs(rng, w, n_public, n_cons), seed), w


# the key shapes of tests/test_groth16_gpu.py: n_public 0 / 1 / 3, domains 2^4 ... 2^12
SHAPES = [
    (8, 0, 10, "random"),    # N = 16
    (12, 1, 28, "small"),    # N = 32
    (10, 3, 20, "edge"),     # N = 32
    (20, 3, 100, "repeat"),  # N = 128
    (40, 1, 1000, "random"),  # N = 1024
    (64, 1, 3000, "small"),  # N = 4096
]


@pytest.mark.parametrize("n_vars,n_public,n_cons,kind", SHAPES)
def test_device_proofs_are_accepted_by_the_native_verifier(hal, n_vars, n_public, n_cons, kind):
    s, w = setup_for(n_vars, n_public, n_cons, kind, seed=n_cons)
    z = s.zkey()
    key = g16.Groth16Key(hal, z)
    vk = key.vk()
    assert vk == g16.VerifyingKey.from_zkey(z)
    assert vk.as_dict() == s.vk() and vk.n_public == n_public
    proof = key.prove(w)  # r and s from OS randomness
    assert proof.public == w[1:n_public + 1]
    assert g16.verify(vk, proof) is None
    # the same proof under another key's vk, and with one public signal changed
    s2, _ = setup_for(n_vars, n_public, n_cons, kind, seed=n_cons + 1)
    with pytest.raises(HalError, match="pairing check failed"):
        g16.verify(g16.VerifyingKey.from_zkey(s2.zkey()), proof)
    if n_public:
        i = n_cons % n_public
        pub = list(proof.public)
        pub[i] = (pub[i] + 1) % R
        with pytest.raises(HalError, match="pairing check failed"):
            g16.verify(vk, proof.with_public(pub))
    assert g16.verify(vk, proof) is None
    key.free()


def test_seal_path_end_to_end(hal):
    s, w = setup_for(12, 1, 28, "random", seed=61)
    key = g16.Groth16Key(hal, s.zkey())
    vk = key.vk()
    proof = key.prove(w)
    selector = b"\x62\xf0\x49\xf6"
    seal = proof.seal(selector)
    assert len(seal) == 260 and seal[:4] == selector
    back = g16.Proof.from_seal(seal)
    assert back.as_tuple() == proof.as_tuple() and back.public == []
    with pytest.raises(HalError, match="n_public mismatch"):
        g16.verify(vk, back)
    assert g16.verify(vk, back.with_public(w[1:2])) is None
    assert g16.verify(vk, g16.Proof.from_seal(seal[4:], w[1:2])) is None
    # bx_groth16_verify_seal takes the one public input as a 32-byte big-endian digest
    assert g16.verify_seal(vk, seal, w[1].to_bytes(32, "big")) is None
    with pytest.raises(HalError, match="pairing check failed"):
        g16.verify_seal(vk, seal, ((w[1] + 1) % R).to_bytes(32, "big"))
    # and through the snarkjs JSON
    assert g16.verify(g16.VerifyingKey.from_json(vk.to_json()), g16.Proof.from_json(proof.to_json(), proof.public_json())) is None
    key.free()


def test_two_keys_one_ctx_and_a_sha256_ctx_each_verify_under_their_own_vk(hal):
    s1, w1 = setup_for(9, 1, 6, "random", seed=31)
    s2, w2 = setup_for(9, 1, 6, "small", seed=32)
    k1, k2 = g16.Groth16Key(hal, s1.zkey()), g16.Groth16Key(hal, s2.zkey())
    v1, v2 = k1.vk(), k2.vk()
    assert v1.as_dict() == s1.vk() and v2.as_dict() == s2.vk() and v1 != v2
    p2, p1 = k2.prove(w2), k1.prove(w1)
    assert g16.verify(v1, p1) is None and g16.verify(v2, p2) is None
    for vk, p in ((v1, p2), (v2, p1)):
        with pytest.raises(HalError, match="pairing check failed"):
            g16.verify(vk, p)
    k1.free()
    k2.free()
    sh = HipHal(0, hashfn="sha-256")
    try:
        k = g16.Groth16Key(sh, s1.zkey())
        assert k.vk() == v1
        p = k.prove(w1)
        assert g16.verify(v1, p) is None
        with pytest.raises(HalError, match="pairing check failed"):
            g16.verify(v2, p)
        k.free()
    finally:
        sh.close()


def test_upstream_key_proves_and_verifies_natively(hal):
    zkeys, wtns = sorted(glob.glob(os.path.join(UPSTREAM, "*.zkey"))), sorted(glob.glob(os.path.join(UPSTREAM, "*.wtns")))
    if not zkeys or not wtns:
        pytest.skip("no zkey + wtns under tests/golden/groth16/upstream/")
    key = g16.Groth16Key(hal, zkeys[0])
    vk = key.vk()
    assert vk == g16.VerifyingKey.from_zkey(zkeys[0])
    proof = key.prove(g16.read_wtns(wtns[0]))
    assert g16.verify(vk, proof) is None
    key.free()
