"""GPU: the size-dependent shapes of the BN254 Groth16 prover against tests/bn254_ref.py, over tiled points (tests/bn254_tiled.py,
validated on the CPU by tests/test_bn254_tiled_cpu.py).

* every MSM window width c = 4 .. 16 on G1 and G2, so every (W, G, seg) of the Pippenger pipeline: uniform, sparse, single-digit,
  all-in-one-bucket and circom-like scalars (G2 with sparse buckets at seg > 1 is `g2-...-c13-sparse` / `-c16-sparse`);
* bucket lists whose lengths sit on the chunk boundaries of the level kernels;
* proof parity on NTT domains of 1, 2, 4 and 8 points (LDS workgroups of 1, 2 and 4 lanes) and of 2^11, 2^13 and 2^14 (one, three
  and four global stages), with CSR rows that are empty ranges.

Every comparison is exact equality of affine coordinates (None = infinity)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402
import bn254_tiled as tiled  # noqa: E402

from boundless_amd import groth16 as g16  # noqa: E402
from boundless_amd.hal import HipHal  # noqa: E402

pytestmark = pytest.mark.gpu
R = ref.R


@pytest.fixture(scope="module")
def hal():
    h = HipHal(0)
    yield h
    h.close()


class _Points:
    """one device copy of the tiled points at a time: kept while consecutive cases share (group, n), freed when they change"""

    def __init__(self, hal):
        self.hal, self.key, self.buf = hal, None, None
        _, p1, _, p2 = tiled.tables()
        self.words = {1: (g16.g1_words(p1), 16), 2: (g16.g2_words(p2), 32)}

    def get(self, group, n):
        if self.key != (group, n):
            self.free()
            words, per = self.words[group]
            self.buf, self.key = self.hal.copy_from(tiled.tile_words(words, per, n)), (group, n)
        return self.buf

    def free(self):
        if self.buf is not None:
            self.buf.free()
        self.key = self.buf = None


@pytest.fixture(scope="module")
def points(hal):
    p = _Points(hal)
    yield p
    p.free()


def _group(group):
    k1, _, k2, _ = tiled.tables()
    return (k1, ref.G1F, ref.G1_GEN, g16.msm_g1) if group == 1 else (k2, ref.G2F, ref.G2_GEN, g16.msm_g2)


# (group, n, pattern), ordered so that the cases of one (group, n) follow each other.  The circom-like skew on G1 at 2^20 is
# test_groth16_gpu.py's.
SWEEP = [(g, n, p) for g in (1, 2) for n in tiled.sweep_sizes() for p in tiled.PATTERNS if (g, n, p) != (1, 1 << 20, "skewed")]


def _sweep_id(case):
    g, n, p = case
    return f"g{g}-n{n}-c{tiled.window_shape(n)[0]}-{p}"


@pytest.mark.parametrize("case", SWEEP, ids=_sweep_id)
def test_msm_width_sweep(hal, points, case):
    group, n, name = case
    ks, F, gen, msm = _group(group)
    sc = tiled.pattern(name, seed=1000 * group + tiled.PATTERNS.index(name), n=n)
    scb = hal.copy_from(sc.ravel())
    try:
        got = msm(hal, points.get(group, n), scb, n)
    finally:
        scb.free()
    assert got == ref.mul(F, gen, tiled.tiled_total(ks, sc))


@pytest.mark.parametrize("group", [1, 2])
def test_msm_bucket_lists_on_chunk_boundaries(hal, points, group):
    """distinct buckets of one MSM (c = 9) hold 1, 15, 16, 17, 255, 256, 257, 4095, 4096 and 4097 points; one scalar is zero and
    one point, whose scalar names the 16-entry bucket, is the point at infinity"""
    ks, F, gen, msm = _group(group)
    sc, dead, _ = tiled.chunk_boundary_case(seed=group)
    n = len(sc)
    points.free()
    words, per = points.words[group]
    pw = tiled.tile_words(words, per, n).reshape(n, per).copy()
    pw[dead] = 0
    pts, scb = hal.copy_from(pw.ravel()), hal.copy_from(sc.ravel())
    try:
        got = msm(hal, pts, scb, n)
    finally:
        pts.free()
        scb.free()
    assert got == ref.mul(F, gen, tiled.tiled_total(ks, sc, dead))


# ---- proof parity across NTT shapes ----
PROOFS = tiled.PROOF_SHAPES


def _proof_id(case):
    n_vars, n_public, n_cons = case[:3]
    N = tiled.proof_domain(case)
    return f"N{N}-vars{n_vars}-pub{n_public}-{case[3]}" + ("-emptyA" if case[4] is not None else "") + ("-emptyB" if case[5] is not None else "")


@pytest.mark.parametrize("case", PROOFS, ids=_proof_id)
def test_parity_across_ntt_shapes(hal, points, case):
    n_vars, n_public, n_cons, kind, ea, eb = case
    points.free()
    key, w = tiled.tiled_key(n_vars, n_public, n_cons, kind, seed=n_cons + n_vars, empty_a_from=ea, empty_b_from=eb)
    z = key.zkey()
    assert g16.inspect(z)["domain_size"] == key.N
    dev = g16.Groth16Key(hal, z)
    try:
        assert dev.info["domain_size"] == key.N and dev.info["n_vars"] == n_vars
        r, s = 0x1234567 + n_cons, R - 5 - n_cons
        got = dev.prove(w, r, s)
    finally:
        dev.free()
    assert got.as_tuple() == ref.prove(key, w, r, s, definitional=False)
    assert got.public == w[1:n_public + 1]
