"""GPU: the BN254 edge operands of tests/bn254_edge.py on gfx950.

* the op table of tests/bn254_edge_ops.hpp built for the device (one launch per op family): equal to the Python reference and
  byte-identical to the host program's result file;
* edge COORDINATES through the library's own MSM kernels (msm_bucket, msm_level0, msm_level, msm_window_reduce with its
  xyzz_mul_small, the host Horner and affine conversion): bx_bn254_msm_g1/g2 do not check on-curve, and any (x, y) is a point of
  y^2 = x^3 + b' with b' = y^2 - x^3, so the affine chord-and-tangent law is the reference;
* edge SCALARS, reduced and not: the kernels read all 256 bits, so the result is (k mod r) P (include/bx_groth16.h says so);
* bx_groth16_key_load refuses a key with a coordinate not below q, in every section, by message.

Every comparison is exact equality."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_edge as edge  # noqa: E402
import bn254_ref as ref  # noqa: E402
import bn254_tiled as tiled  # noqa: E402

from boundless_amd import groth16 as g16  # noqa: E402
from boundless_amd.hal import HalError, HipHal  # noqa: E402

pytestmark = pytest.mark.gpu
Q, R = ref.Q, ref.R
FAMILIES = [edge.FIELD_Q, edge.FIELD_R, edge.FQ2, edge.CURVE_Q, edge.CURVE_Q2]


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


# ---- the header through the op table ----
@pytest.mark.parametrize("family", FAMILIES, ids=[edge.FAMILY_NAMES[f] for f in FAMILIES])
def test_device_build_matches_python_integers_and_the_host_program(tmp_path, family):
    rec, exp, ops = edge.cases(family)
    got = edge.run_dev(family, rec)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(rec)} rows differ; first: row {bad[0]} op {ops[bad[0]]}\nin  {rec[bad[0]]}\ngot {got[bad[0]]}\nexp {exp[bad[0]]}"
    _, raw = edge.run_host(family, rec, tmp_path)
    assert got.astype("<u4").tobytes() == raw


@pytest.mark.parametrize("family", [edge.FIELD_Q, edge.FIELD_R], ids=["q", "r"])
def test_mul_outside_its_domain_on_the_device(tmp_path, family):
    rec, exp = edge.raw_mul_cases(edge.Q if family == edge.FIELD_Q else edge.FR)
    got = edge.run_dev(family, rec)
    assert np.array_equal(got, exp)
    assert got.astype("<u4").tobytes() == edge.run_host(family, rec, tmp_path)[1]


@pytest.mark.parametrize("family", [edge.CURVE_Q, edge.CURVE_Q2], ids=["g1", "g2"])
def test_on_curve_of_coordinates_not_below_q_device_equals_host(tmp_path, family):
    """no reference says what on_curve answers outside its domain; the two builds of one text must still agree"""
    rec = edge.on_curve_records(family, edge.noncanonical_points(family))
    host, raw = edge.run_host(family, rec, tmp_path)
    assert edge.run_dev(family, rec).astype("<u4").tobytes() == raw
    assert host[:, -1].sum() == (72 if family == edge.CURVE_Q else 52)  # tests/test_bn254_edge_cpu.py says where these come from
    rec, _ = edge.noncanonical_doubling(family)  # and the sums that miss the doubling branch are the same wrong sums
    assert edge.run_dev(family, rec).astype("<u4").tobytes() == edge.run_host(family, rec, tmp_path)[1]


# ---- edge coordinates through the MSM ----
MSM_SCALARS = (1, 2, 3, 5, 15, (1 << 32) - 1)
N_MSM_PAIRS = 56  # 9 MSM calls per pair: 504 per group


def _point_words(F, pts):
    """stored (x, y) pairs -> the MSM's point layout"""
    return np.hstack([F.w([p[0] for p in pts]), F.w([p[1] for p in pts])]).ravel()


@pytest.mark.parametrize("family", [edge.CURVE_Q, edge.CURVE_Q2], ids=["g1", "g2"])
def test_msm_of_points_with_edge_coordinates(hal, family):
    F = edge.FIELD_OF[family]
    msm = g16.msm_g1 if family == edge.CURVE_Q else g16.msm_g2
    one = {k: hal.copy_from(g16.scalar_words([k])) for k in MSM_SCALARS}
    two = hal.copy_from(g16.scalar_words([1, 1]))
    wrong, finite = [], 0
    try:
        for xs, ys in edge.curve_pairs(family)[:N_MSM_PAIRS]:
            P = None if (xs, ys) == (F.zero, F.zero) else (F.val(xs), F.val(ys))
            twice = hal.copy_from(_point_words(F, [(xs, ys), (xs, ys)]))
            inverse = hal.copy_from(_point_words(F, [(xs, ys), (xs, F.sub(F.zero, ys))]))
            beside_inf = hal.copy_from(_point_words(F, [(F.zero, F.zero), (xs, ys)]))
            try:
                for k in MSM_SCALARS:  # n = 1: the window reduction's k * B_k and the Horner doublings
                    want = edge.aff_mul(F, P, k)
                    finite += want is not None
                    if msm(hal, twice, one[k], 1) != want:
                        wrong.append((xs, ys, k))
                if msm(hal, twice, two, 2) != edge.aff_mul(F, P, 2):  # level 0 meets the same point twice: the doubling branch
                    wrong.append((xs, ys, "P + P"))
                if msm(hal, inverse, two, 2) is not None:  # and the inverse branch
                    wrong.append((xs, ys, "P - P"))
                if msm(hal, beside_inf, two, 2) != P:  # (0, 0) is infinity: it adds nothing
                    wrong.append((xs, ys, "P + (0, 0)"))
            finally:
                twice.free()
                inverse.free()
                beside_inf.free()
    finally:
        two.free()
        for b in one.values():
            b.free()
    assert not wrong, f"{len(wrong)} wrong sums; first (stored x, stored y, case): {wrong[0]}"
    assert finite >= (N_MSM_PAIRS - 8) * len(MSM_SCALARS)  # the expected sums are points, not one long list of infinities


# ---- scalar edges ----
EDGE_SCALARS = ([R - 1, R - 2, 1 << 253] + [1 << (32 * j) for j in range(1, 8)] + [(1 << (32 * j)) - 1 for j in range(1, 8)]
                + [R, R + 1, 1 << 255, (1 << 256) - 1])  # the last four are not reduced: the result is (k mod r) P


def _group(group):
    k1, p1, k2, p2 = tiled.tables()
    return (k1, g16.g1_words(p1), 16, ref.G1F, ref.G1_GEN, g16.msm_g1) if group == 1 else (k2, g16.g2_words(p2), 32, ref.G2F, ref.G2_GEN, g16.msm_g2)


@pytest.mark.parametrize("group", [1, 2])
def test_msm_scalar_edges_one_point(hal, group):
    ks, words, per, F, gen, msm = _group(group)
    pts = hal.copy_from(tiled.tile_words(words, per, 1))
    try:
        for k in EDGE_SCALARS:
            sc = hal.copy_from(g16.scalar_words([k]))
            try:
                assert msm(hal, pts, sc, 1) == ref.mul(F, gen, (k % R) * ks[0] % R), hex(k)
            finally:
                sc.free()
    finally:
        pts.free()


@pytest.mark.parametrize("pattern", ["cycled", "all_2^256-1"])
@pytest.mark.parametrize("n", [300, 600], ids=["n300-c4", "n600-c5"])
@pytest.mark.parametrize("group", [1, 2])
def test_msm_scalar_edges_many_points(hal, group, n, pattern):
    """c = 4 divides 256; at c = 5 the top window holds one bit.  In 2^256 - 1 every digit of every window is maximal."""
    assert tiled.window_shape(n)[0] == (4 if n == 300 else 5)
    ks, words, per, F, gen, msm = _group(group)
    scalars = [EDGE_SCALARS[i % len(EDGE_SCALARS)] for i in range(n)] if pattern == "cycled" else [(1 << 256) - 1] * n
    sc = g16.scalar_words(scalars).reshape(n, 8)
    pts, scb = hal.copy_from(tiled.tile_words(words, per, n)), hal.copy_from(sc.ravel())
    try:
        got = msm(hal, pts, scb, n)
    finally:
        pts.free()
        scb.free()
    want = sum((k % R) * ks[i % len(ks)] for i, k in enumerate(scalars)) % R
    assert want == tiled.tiled_total(ks, sc)
    assert got == ref.mul(F, gen, want)


# ---- the loader refuses coordinates not below q ----
def _sections(z):
    out, at = {}, 12
    for _ in range(struct.unpack_from("<I", z, 8)[0]):
        t, size = struct.unpack_from("<IQ", z, at)
        out[t] = (at + 12, size)
        at += 12 + size
    return out


def test_key_with_a_coordinate_not_below_q_is_refused(hal, tmp_path):
    import random

    rng = random.Random(21)
    w = ref.random_witness(rng, 9, "random")
    s = ref.Setup(ref.random_r1cs(rng, w, 1, 6), 21)
    z = s.zkey()
    sec = _sections(z)
    h = sec[2][0]
    # (what the message must name, offset of the first point, points, coordinates per point)
    lists = [("section 2 (alpha1)", h + 84, 1, 2), ("section 2 (beta1)", h + 148, 1, 2), ("section 2 (beta2)", h + 212, 1, 4),
             ("section 2 (gamma2)", h + 340, 1, 4), ("section 2 (delta1)", h + 468, 1, 2), ("section 2 (delta2)", h + 532, 1, 4),
             ("section 3 (IC)", sec[3][0], 2, 2), ("section 5 (A)", sec[5][0], 9, 2), ("section 6 (B1)", sec[6][0], 9, 2),
             ("section 7 (B2)", sec[7][0], 9, 4), ("section 8 (C)", sec[8][0], 7, 2), ("section 9 (H)", sec[9][0], s.N, 2)]
    muts = []  # (what, point index, byte offset of the coordinate, new value, the mutated point's coordinates)
    for what, at, count, coords in lists:
        for i in range(count):
            c = [int.from_bytes(z[at + 32 * (coords * i + j):at + 32 * (coords * i + j + 1)], "little") for j in range(coords)]
            if not any(c):
                continue  # infinity
            for j in range(coords):
                for mult in (1, 2, 3):
                    d = list(c)
                    d[j] += mult * Q
                    assert d[j] < 1 << 256
                    muts.append((what, i, at + 32 * (coords * i + j), d[j], tuple(d)))
    # what on_curve alone says about each mutated point (the host build of the same header)
    accepted = {}
    for family, coords in ((edge.CURVE_Q, 2), (edge.CURVE_Q2, 4)):
        idx = [n for n, m in enumerate(muts) if len(m[4]) == coords]
        pts = [muts[n][4] if coords == 2 else (muts[n][4][:2], muts[n][4][2:]) for n in idx]
        flags = edge.run_host(family, edge.on_curve_records(family, pts), tmp_path)[0][:, -1]
        accepted.update(zip(idx, flags))
        assert flags.any(), "no mutation of this point type passes on_curve: the test would not see a loader without the range check"
    for what in {m[0] for m in muts}:
        assert any(accepted[n] for n, m in enumerate(muts) if m[0] == what) or what.startswith("section 2"), what
    for n, (what, i, off, value, _) in enumerate(muts):
        bad = bytearray(z)
        bad[off:off + 32] = value.to_bytes(32, "little")
        with pytest.raises(HalError, match="not below q") as e:
            g16.Groth16Key(hal, bytes(bad))
        assert f"{what}: point {i} " in str(e.value), (str(e.value), bool(accepted[n]))
    key = g16.Groth16Key(hal, z)  # the unmutated key still loads, proves and verifies
    try:
        proof = key.prove(w, 1, 2)
        assert proof.as_tuple() == ref.prove(s, w, 1, 2)
        g16.verify(key.vk(), proof)
    finally:
        key.free()
