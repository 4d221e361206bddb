"""CPU: the tiled-point helpers of tests/bn254_tiled.py against the definitional code of tests/bn254_ref.py — the evidence that
the expected values of tests/test_groth16_shapes_gpu.py are right independently of any kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_ref as ref  # noqa: E402
import bn254_tiled as tiled  # noqa: E402

R = ref.R


def _digits(k, c):
    """{window: digit} of the non-zero c-bit digits of k"""
    out, w = {}, 0
    while k:
        if k & ((1 << c) - 1):
            out[w] = k & ((1 << c) - 1)
        k >>= c
        w += 1
    return out


@pytest.mark.parametrize("group,t,n", [(1, 48, 300), (2, 24, 77)])
def test_tiled_total_equals_the_definitional_msm(group, t, n):
    """n is no multiple of the table size t; the scalars mix every pattern, and one point is the point at infinity"""
    k1, p1, k2, p2 = tiled.tables()
    ks, pts = (k1[:t], p1[:t]) if group == 1 else (k2[:t], p2[:t])
    F, gen = (ref.G1F, ref.G1_GEN) if group == 1 else (ref.G2F, ref.G2_GEN)
    rng = np.random.default_rng(group)
    q = n // 5
    sc = np.concatenate([tiled.uniform(rng, q), tiled.single_digit(rng, q, 9, 2), tiled.single_digit(rng, q, 16, 8), tiled.skewed(rng, q),
                         tiled.all_ones_253(n - 4 * q)])
    assert len(sc) == n and n % t
    dead = [q + 3]
    P = [None if i in dead else pts[i % t] for i in range(n)]
    want = ref.msm(F, P, tiled.scalar_ints(sc))
    assert want is not None
    assert ref.mul(F, gen, tiled.tiled_total(ks, sc, dead)) == want
    # the dead row matters: counting it gives another point
    assert ref.mul(F, gen, tiled.tiled_total(ks, sc)) != want
    # and the device layout of the tiled points is the table repeated and cut at n
    words = np.arange(t * 4, dtype=np.uint32)
    assert tiled.tile_words(words, 4, n).reshape(n, 4)[t + 1].tolist() == [4, 5, 6, 7]
    assert tiled.tile_words(words, 4, n).size == 4 * n


@pytest.mark.parametrize("c", range(4, 17))
def test_patterns_are_canonical_and_land_in_their_buckets(c):
    n = 1 << (c + 4)
    assert tiled.window_shape(n)[0] == c
    seg = tiled.window_shape(n)[3]
    rng = np.random.default_rng(c)
    allowed = set(tiled.digit_set(c, seg))
    wtop, dmax = tiled.top_window(c), tiled.top_digit_max(c)
    assert dmax >= 1 and (dmax << (c * wtop)) < R <= ((dmax + 1) << (c * wtop))
    seen_w, seen_d = set(), set()
    for k in tiled.scalar_ints(tiled.single_digit(rng, 600, c, seg)):
        assert 0 < k < R
        (w, d), = _digits(k, c).items()
        assert d in allowed or (w == wtop and d == dmax)
        seen_w.add(w)
        seen_d.add(d)
    assert seen_w == set(range(wtop + 1)) and allowed <= seen_d
    uni = tiled.scalar_ints(tiled.uniform(rng, 500))
    assert uni[:3] == [R - 1, 0, 1] and all(k < R for k in uni) and max(uni[3:]).bit_length() == 254
    sp = tiled.scalar_ints(tiled.sparse(rng, 4096, c, seg))
    assert all(k < R for k in sp) and 20 <= sum(1 for k in sp if k) <= 120
    if c >= 9:
        assert all(len(_digits(k, c)) == 1 for k in sp if k)
    ones = tiled.scalar_ints(tiled.all_ones_253(3))
    assert ones == [(1 << 253) - 1] * 3 and all(d == (1 << c) - 1 for w, d in _digits(ones[0], c).items() if w < 253 // c)
    assert all(k < R for k in tiled.scalar_ints(tiled.skewed(rng, 300)))


def test_sweep_reaches_every_width_and_reduction_shape():
    ns = tiled.sweep_sizes()
    shapes = {n: tiled.window_shape(n) for n in ns}
    for n, (c, W, G, seg) in shapes.items():
        print(f"n = {n}: c = {c}, W = {W}, G = {G}, seg = {seg}")
    assert {s[0] for s in shapes.values()} == set(range(4, 17))
    assert {s[2] for s in shapes.values()} == {1, 2, 4, 8, 16, 32}
    assert {s[3] for s in shapes.values()} == {1, 2, 4, 8}
    assert 1 << 20 in ns and min(ns) < 256 and max(ns) < (1 << 20) + 16
    for c in range(4, 17):  # one n in [2^(c+4), 2^(c+5)) that is no power of two
        assert any((1 << (c + 4)) < n < (1 << (c + 5)) and n & (n - 1) for n in ns), c
    assert shapes[1 << 20] == (16, 16, 32, 8) and shapes[200][0] == 4


def test_proof_cases_cover_the_ntt_shapes_and_spread_the_msm_widths():
    shapes = []
    for case in tiled.PROOF_SHAPES:
        n_vars, n_public, N = case[0], case[1], tiled.proof_domain(case)
        shapes.append((N, tiled.window_shape(n_vars + 2)[0], tiled.window_shape(n_vars - n_public - 1 + N + 3)[0]))
        print(f"N = {N}: c = {shapes[-1][1]} for A / B1 / B2, c = {shapes[-1][2]} for C")
    assert {N for N, _, _ in shapes} == {1, 2, 4, 8, 1 << 11, 1 << 13, 1 << 14}
    assert all(ca != cc for N, ca, cc in shapes if N >= 1 << 11)
    assert {c for _, ca, cc in shapes for c in (ca, cc)} >= {4, 7, 8, 9, 10, 11}
    assert {case[1] for case in tiled.PROOF_SHAPES} == {0, 1}
    assert any(case[4] is not None for case in tiled.PROOF_SHAPES) and any(case[5] is not None for case in tiled.PROOF_SHAPES)


def test_chunk_boundary_case_fills_its_buckets_exactly():
    sc, dead, buckets = tiled.chunk_boundary_case(1)
    n = len(sc)
    c = tiled.window_shape(n)[0]
    assert c == 9 and n == sum(tiled.CHUNK_LENGTHS) + 2
    hist, zeros = {}, 0
    for i, k in enumerate(tiled.scalar_ints(sc)):
        assert k < R
        if i in dead:
            assert _digits(k, c) == {buckets[tiled.CHUNK_LENGTHS.index(16)][0]: buckets[tiled.CHUNK_LENGTHS.index(16)][1]}
        elif k == 0:
            zeros += 1
        else:
            (b,) = _digits(k, c).items()
            hist[b] = hist.get(b, 0) + 1
    assert zeros == 1 and [hist[b] for b in buckets] == list(tiled.CHUNK_LENGTHS)
    # shuffled: the longest list is not one contiguous run of rows
    rows = [i for i, k in enumerate(tiled.scalar_ints(sc)) if _digits(k, c) == {buckets[-1][0]: buckets[-1][1]}]
    assert rows[-1] - rows[0] > len(rows)


def test_tiled_key_definitional_and_trapdoor_provers_agree():
    """N = 16: the proof through the tiled logs is the proof by plain MSMs over the key's points"""
    key, w = tiled.tiled_key(9, 1, 11, "random", seed=16)
    assert key.N == 16
    r, s = 0x1234567, R - 5
    want = ref.prove(key, w, r, s, definitional=True)
    assert all(P is not None for P in want)
    assert ref.prove(key, w, r, s, definitional=False) == want
    # rows emptied past an index change the proof, and the two provers still agree
    key2, w2 = tiled.tiled_key(9, 1, 11, "random", seed=16, empty_a_from=4)
    assert w2 == w and ref.prove(key2, w, r, s, definitional=False) == ref.prove(key2, w, r, s, definitional=True) != want


@pytest.fixture(scope="module")
def g16():
    from boundless_amd import build

    build.build(verbose=False)
    from boundless_amd import groth16

    return groth16


@pytest.mark.parametrize("n_vars,n_public,n_cons,N", [(5, 0, 0, 1), (5, 0, 1, 2), (6, 1, 2, 4), (7, 1, 5, 8), (9, 1, 11, 16)])
def test_tiled_zkeys_are_accepted_by_inspect(g16, n_vars, n_public, n_cons, N):
    """the library's host-side parser reads a tiled key like any other, down to a domain of one point"""
    key, _ = tiled.tiled_key(n_vars, n_public, n_cons, "small", seed=N)
    z = key.zkey()
    assert g16.inspect(z) == {"n_vars": n_vars, "n_public": n_public, "domain_size": N, "n_coefs": len(key.coefs), "bytes": len(z)}
