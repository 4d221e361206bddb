"""GPU: the BN254 Groth16 prover (include/bx_groth16.h) and its MSMs against the independent restatement tests/bn254_ref.py —
exact parity with fixed r and s, pairing verification with random r and s, the MSM edge cases, the MSM at 2^20 and 2^22 by
linearity (uniform and circom-like skewed scalars), refusals, and keys and memory."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402
import bn254_tiled as tiled  # noqa: E402

from boundless_amd import groth16 as g16  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402

pytestmark = pytest.mark.gpu
R = ref.R


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


def setup_for(n_vars, n_public, n_cons, kind, seed):
    rng = random.Random(seed)
    w = ref.random_witness(rng, n_vars, kind)
    r1 = ref.random_r1cs(rng, w, n_public, n_cons)
    return ref.Setup(r1, seed), w


# n_public 0 / 1 / 3; domains 2^4 ... 2^12; witnesses with zeros, ones, r - 1, repeated and random values
PARITY = [
    (8, 0, 10, "random", True),    # N = 16
    (12, 1, 28, "small", True),    # N = 32
    (10, 3, 20, "edge", True),     # N = 32
    (20, 3, 100, "repeat", False),  # N = 128
    (40, 1, 1000, "random", False),  # N = 1024
    (64, 1, 3000, "small", False),  # N = 4096
]


@pytest.mark.parametrize("n_vars,n_public,n_cons,kind,definitional", PARITY)
def test_parity_with_fixed_r_s(hal, n_vars, n_public, n_cons, kind, definitional):
    s, w = setup_for(n_vars, n_public, n_cons, kind, seed=n_cons)
    key = g16.Groth16Key(hal, s.zkey())
    assert key.info["domain_size"] == s.N and key.info["n_vars"] == n_vars
    r, sk = 0x1234567 + n_cons, R - 5 - n_cons
    got = key.prove(w, r, sk)
    want = ref.prove(s, w, r, sk, definitional=definitional)
    assert got.as_tuple() == want
    assert got.public == w[1:n_public + 1]
    key.free()


def test_random_proofs_verify_and_differ(hal):
    s, w = setup_for(14, 2, 40, "random", seed=5)
    key = g16.Groth16Key(hal, s.zkey())
    p1, p2 = key.prove(w), key.prove(w)
    assert p1.as_tuple() != p2.as_tuple()
    assert ref.verify(s.vk(), p1.as_tuple(), w[1:3])
    assert ref.verify(s.vk(), p2.as_tuple(), w[1:3])
    import json

    j = json.loads(p1.to_json())
    assert j["pi_a"][:2] == [str(p1.a[0]), str(p1.a[1])] and j["pi_b"][2] == ["1", "0"] and j["curve"] == "bn128"
    assert json.loads(p1.public_json()) == [str(x) for x in w[1:3]]
    assert len(p1.seal(b"\x62\xf0\x49\xf6")) == 260
    key.free()


# ---- MSM against Python, by discrete logs ----
T = 1024


@pytest.fixture(scope="module")
def tables():
    k1, p1, k2, p2 = tiled.tables()
    assert len(k1) == T
    return k1, p1, g16.g1_words(p1), k2, p2, g16.g2_words(p2)


def _expect(F, gen, ks, scalars):
    return ref.mul(F, gen, sum(k * s for k, s in zip(ks, scalars)) % R)


def _cases(rng, n_tab):
    """(point indices into the table, or None for infinity; scalars)"""
    idx = [rng.randrange(n_tab) for _ in range(700)]
    out = {
        "zero_one_rminus1": (idx[:300], [rng.choice([0, 1, R - 1]) for _ in range(300)]),
        "all_equal": (idx[:333], [123456789 * 10 ** 40 % R] * 333),
        "duplicated": ([5] * 100 + [6] * 50, [rng.randrange(R) for _ in range(150)]),
        "n1": ([3], [rng.randrange(R)]),
        "not_pow2": (idx[:677], [rng.randrange(R) for _ in range(677)]),
        "with_infinity": (idx[:40] + [None] * 10, [rng.randrange(R) for _ in range(50)]),
    }
    return out


@pytest.mark.parametrize("group", [1, 2])
def test_msm_edge_cases(hal, tables, group):
    k1, p1, _, k2, p2, _ = tables
    ks, pts = (k1, p1) if group == 1 else (k2, p2)
    F, gen, msm = (ref.G1F, ref.G1_GEN, g16.msm_g1) if group == 1 else (ref.G2F, ref.G2_GEN, g16.msm_g2)
    rng = random.Random(group)
    for name, (idx, sc) in _cases(rng, len(ks)).items():
        P = [None if i is None else pts[i] for i in idx]
        K = [0 if i is None else ks[i] for i in idx]
        assert msm(hal, P, sc) == _expect(F, gen, K, sc), name
    # P with -P: sum P_i - P_i = infinity, and P + P + (-P) = P
    a = pts[7]
    assert msm(hal, [a, ref.neg(F, a)], [5, 5]) is None
    assert msm(hal, [a, a, ref.neg(F, a)], [1, 1, 1]) == a
    assert msm(hal, [a], [0]) is None
    # n up to about 2^12: the table tiled four times
    n = 4 * len(ks) + 3
    idx = [i % len(ks) for i in range(n)]
    sc = [rng.randrange(R) for _ in range(n)]
    assert msm(hal, [pts[i] for i in idx], sc) == _expect(F, gen, [ks[i] for i in idx], sc)


def _big_scalars(rng, n, skew):
    w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 7] &= 0x1FFFFFFF  # below 2^253 < r
    if skew:
        m = rng.random(n)
        w[m < 0.9] = 0
        w[m < 0.45, 0] = 1
    return w


@pytest.mark.parametrize("log_n,skew", [(20, False), (20, True), (22, False), (22, True)])
def test_msm_g1_large_by_linearity(hal, tables, log_n, skew):
    k1, _, w1, _, _, _ = tables
    n = 1 << log_n
    rng = np.random.default_rng(log_n + skew)
    sc = _big_scalars(rng, n, skew)
    pts = hal.copy_from(np.tile(w1, n // T))
    scb = hal.copy_from(sc.ravel())
    got = g16.msm_g1(hal, pts, scb, n)
    # sum_i s_i k_(i mod T) mod r
    assert got == ref.mul(ref.G1F, ref.G1_GEN, tiled.tiled_total(k1, sc))
    pts.free()
    scb.free()


# ---- refusals ----
def test_prove_refusals(hal):
    s, w = setup_for(9, 1, 6, "random", seed=21)
    key = g16.Groth16Key(hal, s.zkey())
    with pytest.raises(HalError, match="witness length"):
        key.prove(w[:-1], 1, 2)
    with pytest.raises(HalError, match="not below r"):
        key.prove(w[:3] + [R] + w[4:], 1, 2)
    with pytest.raises(HalError, match=r"witness\[0\] must be 1"):
        key.prove([2] + w[1:], 1, 2)
    with pytest.raises(HalError, match="r or s"):
        key.prove(w, R, 2)
    assert key.prove(w, 1, 2).as_tuple() == ref.prove(s, w, 1, 2)  # still usable
    key.free()


def test_key_with_off_curve_point_refused(hal):
    import struct

    s, _ = setup_for(9, 1, 6, "random", seed=22)
    z = bytearray(s.zkey())
    n, at = struct.unpack_from("<I", z, 8)[0], 12
    for _ in range(n):
        t, size = struct.unpack_from("<IQ", z, at)
        if t == 7:  # B2: bump y.c0 of the first finite point
            i = next(i for i, P in enumerate(s.B2) if P is not None)
            off = at + 12 + 128 * i + 64
            y = int.from_bytes(z[off:off + 32], "little")
            z[off:off + 32] = ((y + 1) % ref.Q).to_bytes(32, "little")
        at += 12 + size
    with pytest.raises(HalError, match="not on its curve"):
        g16.Groth16Key(hal, bytes(z))


# ---- keys and memory ----
def test_two_keys_one_ctx_and_a_sha256_ctx(hal):
    s1, w1 = setup_for(9, 1, 6, "random", seed=31)
    s2, w2 = setup_for(16, 2, 30, "small", seed=32)
    k1, k2 = g16.Groth16Key(hal, s1.zkey()), g16.Groth16Key(hal, s2.zkey())
    assert k2.prove(w2, 3, 4).as_tuple() == ref.prove(s2, w2, 3, 4)
    assert k1.prove(w1, 3, 4).as_tuple() == ref.prove(s1, w1, 3, 4)
    k1.free()
    k2.free()
    sh = HipHal(0, hashfn="sha-256")
    try:
        k = g16.Groth16Key(sh, s1.zkey())
        assert k.prove(w1, 5, 6).as_tuple() == ref.prove(s1, w1, 5, 6)
        with pytest.raises(HalError, match="another ctx"):
            hal._check(g16._lib().bx_groth16_key_free(hal.ctx, k.key))
        k.free()
    finally:
        sh.close()


def test_twenty_proofs_and_memory_returns(hal, tmp_path):
    import torch

    s, w = setup_for(64, 1, 3000, "random", seed=41)
    path = tmp_path / "k.zkey"
    path.write_bytes(s.zkey())
    want = ref.prove(s, w, 11, 12, definitional=False)
    key = g16.Groth16Key(hal, str(path))
    for _ in range(20):
        assert key.prove(w, 11, 12).as_tuple() == want
    key.free()
    hal.sync()
    base = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        k = g16.Groth16Key(hal, str(path))
        k.prove(w, 11, 12)
        k.free()
    hal.sync()
    assert abs(torch.cuda.mem_get_info()[0] - base) <= 4 << 20


def test_msm_g2_wide_window_reduction(hal, tables):
    """2^17 G2 points: window width 13, so each window's weighted reduction is split over several workgroups"""
    _, _, _, k2, _, w2 = tables
    n, t = 1 << 17, len(k2)
    rng = np.random.default_rng(17)
    sc = _big_scalars(rng, n, skew=False)
    sc[::5] = 0
    sc[1::5] = 0
    sc[1::5, 0] = 1
    pts = hal.copy_from(np.tile(w2, n // t))
    scb = hal.copy_from(sc.ravel())
    got = g16.msm_g2(hal, pts, scb, n)
    assert got == ref.mul(ref.G2F, ref.G2_GEN, tiled.tiled_total(k2, sc))
    pts.free()
    scb.free()


@pytest.mark.parametrize("which", ["ic", "gamma2"])
def test_key_with_off_curve_verifying_point_refused(hal, which):
    """IC and gamma2 take no part in proving, but a key holding an off-curve one is refused as well"""
    import struct

    s, _ = setup_for(9, 1, 6, "random", seed=23)
    z = bytearray(s.zkey())
    n, at = struct.unpack_from("<I", z, 8)[0], 12
    for _ in range(n):
        t, size = struct.unpack_from("<IQ", z, at)
        if which == "ic" and t == 3:
            off = at + 12 + 64 + 32  # IC1.y
        elif which == "gamma2" and t == 2:
            off = at + 12 + 340 + 64  # gamma2 y.c0
        else:
            at += 12 + size
            continue
        y = int.from_bytes(z[off:off + 32], "little")
        z[off:off + 32] = ((y + 1) % ref.Q).to_bytes(32, "little")
        at += 12 + size
    with pytest.raises(HalError, match="not on its curve"):
        g16.Groth16Key(hal, bytes(z))


def test_closing_the_ctx_releases_its_keys():
    """bx_free releases the keys still loaded on its ctx: a key outliving its HipHal leaks nothing, and freeing it later is a no-op"""
    import torch

    s, w = setup_for(40, 1, 1000, "random", seed=51)
    z = s.zkey()
    h = HipHal(0)
    k = g16.Groth16Key(h, z)
    k.prove(w, 1, 2)
    h.close()
    k.free()
    torch.cuda.synchronize()
    base = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        h = HipHal(0)
        k = g16.Groth16Key(h, z)
        assert k.prove(w, 1, 2).as_tuple() == ref.prove(s, w, 1, 2, definitional=False)
        h.close()  # the key is still loaded
        k.free()
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - base) <= 8 << 20
