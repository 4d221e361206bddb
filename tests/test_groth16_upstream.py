"""GPU: a real snarkjs key and witness, when placed under tests/golden/groth16/upstream/ (circuit.zkey + circuit.wtns; see the README
there).  The proof is made on the GPU and checked with the verifying key read from the zkey itself (IC, alpha1, beta2, gamma2,
delta2), which pins the recalled zkey conventions of DESIGN.md §11.  Skips when the files are absent."""
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
UP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groth16", "upstream")
ZKEY, WTNS = os.path.join(UP, "circuit.zkey"), os.path.join(UP, "circuit.wtns")


def _fq(b):
    return int.from_bytes(b, "little") * pow(ref.MONT, -1, ref.Q) % ref.Q


def _g1(b):
    x, y = _fq(b[:32]), _fq(b[32:64])
    return None if x == 0 and y == 0 else (x, y)


def _g2(b):
    c = [_fq(b[32 * i:32 * i + 32]) for i in range(4)]
    return None if not any(c) else ((c[0], c[1]), (c[2], c[3]))


def vk_from_zkey(path):
    z = open(path, "rb").read()
    n, at, secs = struct.unpack_from("<I", z, 8)[0], 12, {}
    for _ in range(n):
        t, size = struct.unpack_from("<IQ", z, at)
        secs[t] = z[at + 12:at + 12 + size]
        at += 12 + size
    h = secs[2]
    npub = struct.unpack_from("<I", h, 76)[0]
    return {"alpha1": _g1(h[84:148]), "beta2": _g2(h[212:340]), "gamma2": _g2(h[340:468]), "delta2": _g2(h[532:660]),
            "ic": [_g1(secs[3][64 * i:64 * i + 64]) for i in range(npub + 1)]}


@pytest.mark.skipif(not (os.path.exists(ZKEY) and os.path.exists(WTNS)), reason="no real zkey / wtns under tests/golden/groth16/upstream/")
def test_real_key_and_witness():
    from boundless_amd import groth16 as g16
    from boundless_amd.hal import HipHal

    hal = HipHal(0)
    try:
        w = g16.read_wtns(WTNS)
        key = g16.Groth16Key(hal, ZKEY)
        proof = key.prove(w)
        vk = vk_from_zkey(ZKEY)
        assert ref.verify(vk, proof.as_tuple(), w[1:key.info["n_public"] + 1])
        key.free()
    finally:
        hal.close()
