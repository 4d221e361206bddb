"""CPU: the BN254 field and curve code (boundless_amd/csrc/bn254_arith.hpp) compiled for the host, on chosen edge operands,
against plain Python integers (tests/bn254_edge.py) — word for word, in a plain build and under AddressSanitizer / UBSan.

Every point the other suites feed this code is k G for a pseudo-random k, so a wrong carry or a `<` for `<=` in the CIOS
product, the conditional subtractions or the limb compares behind the doubling and inverse branches shows about once in 2^32
operands there.  Here the operands are chosen: limb patterns of zeros and ones, neighbours of 0, m, 2^k and R, products forced
onto 0, 1, m - 1, m - 2 and 2^224 - 1, and curve points with such coordinates (on y^2 = x^3 + b', b' = y^2 - x^3)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_edge as edge  # noqa: E402

FAMILIES = [edge.FIELD_Q, edge.FIELD_R, edge.FQ2, edge.CURVE_Q, edge.CURVE_Q2]
N_EDGE = 1835  # what the rule of edge_categories gives for q and for r


@pytest.mark.parametrize("m", [edge.Q, edge.FR], ids=["q", "r"])
def test_operand_set_size_and_categories(m):
    cats = edge.edge_categories(m)
    assert {k: len(v) for k, v in cats.items()} == {"small": 9, "montgomery": 4, "powers": 6 * 254, "below_m": 8, "limb_masks": 320}
    vals = edge.edge_residues(m)
    assert len(vals) == N_EDGE == len(set(vals)) and all(0 <= v < m for v in vals)
    edge.edge_residues.cache_clear()
    assert edge.edge_residues(m) == vals  # the same on two calls
    for must in (0, 1, m - 1, (m - 1) // 2, edge.RR % m, pow(edge.RR, -1, m), (1 << 253) + 1, m - (1 << 224), (1 << 224) - 1,
                 (m >> 224) << 224):
        assert must in vals
    pairs, kinds = edge.operand_pairs(m)
    assert len(pairs) == N_EDGE * (1 + edge.PARTNERS) + 5 * edge.FORCED_PER_TARGET == 76235
    assert kinds.count("self") == N_EDGE and kinds.count("partner") == N_EDGE * edge.PARTNERS and kinds.count("forced") == 1000
    edge.operand_pairs.cache_clear()
    assert edge.operand_pairs(m)[0] == pairs
    assert any(a + b == m for a, b in pairs), "no pair sums to the modulus"
    assert any(a == b for (a, b), k in zip(pairs, kinds) if k == "partner" or k == "self")
    assert any(b > a for a, b in pairs) and any(b < a for a, b in pairs)
    rinv = pow(edge.RR, -1, m)
    products = {a * b * rinv % m for (a, b), k in zip(pairs, kinds) if k == "forced"}
    assert products == set(edge.FORCED_TARGETS(m))


@pytest.mark.parametrize("family", FAMILIES, ids=[edge.FAMILY_NAMES[f] for f in FAMILIES])
def test_reference_is_not_mostly_zeros(family):
    """a stub op table that writes zeros cannot pass: most reference rows are non-zero, for every op of the family"""
    _, exp, ops = edge.cases(family)
    nz = exp.any(axis=1)
    assert nz.mean() > 0.6
    for op in np.unique(ops):
        assert nz[ops == op].any(), f"every expected row of op {op} is zero"
    if family in edge.FIELD_OF:
        E = edge.FIELD_OF[family].E
        law = ops != edge.C_ON_CURVE
        inf = exp[law, 2 * E] == 1
        assert 0.05 < inf.mean() < 0.5  # infinity results (inverse branch, y = 0, k = 0) are there, and are the minority
        assert not exp[law][inf, :2 * E].any()


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("family", FAMILIES, ids=[edge.FAMILY_NAMES[f] for f in FAMILIES])
def test_host_build_matches_python_integers(tmp_path, family, sanitized):
    rec, exp, ops = edge.cases(family)
    got, _ = edge.run_host(family, rec, tmp_path, sanitized=sanitized)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(rec)} rows differ; first: row {bad[0]} op {ops[bad[0]]}\nin  {rec[bad[0]]}\ngot {got[bad[0]]}\nexp {exp[bad[0]]}"
    # the header's "fully reduced" claim, on the output itself
    if family in (edge.FIELD_Q, edge.FIELD_R):
        assert edge.below(got[:, :8], edge.Q if family == edge.FIELD_Q else edge.FR).all()
    else:
        for at in range(0, got.shape[1] - got.shape[1] % 8, 8):
            assert edge.below(got[:, at:at + 8], edge.Q).all()


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("family", [edge.FIELD_Q, edge.FIELD_R], ids=["q", "r"])
def test_mul_outside_its_domain_is_one_reduction_with_one_subtraction(tmp_path, family, sanitized):
    """operands up to 2^256 - 1: the only ones that reach the two carry words of the CIOS product (edge.raw_mul_cases)"""
    rec, exp = edge.raw_mul_cases(edge.Q if family == edge.FIELD_Q else edge.FR)
    assert exp.any(axis=1).mean() > 0.9
    got, _ = edge.run_host(family, rec, tmp_path, sanitized=sanitized)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(rec)} rows differ; first: row {bad[0]}\nin  {rec[bad[0]]}\ngot {got[bad[0]]}\nexp {exp[bad[0]]}"


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_on_curve_accepts_some_coordinates_not_below_q(tmp_path, sanitized):
    """on_curve alone does not refuse an encoding x + i q of a coordinate (the limb compares assume reduced inputs): why
    bx_groth16_key_load checks ranges first.
    The counts are recorded results of this code, not a reference: 72 of 120 G1 encodings accepted, and for 12 of those the sum of
    k G and the encoding is not 2 k G (the figures of the probe that led to the range check); 52 of 96 and 8 on G2.  Every wrong
    sum is fully reduced, so nothing downstream could tell."""
    for family, n, accepted, wrong_doublings in ((edge.CURVE_Q, 120, 72, 12), (edge.CURVE_Q2, 96, 52, 8)):
        pts = edge.noncanonical_points(family)
        assert len(pts) == n
        got, _ = edge.run_host(family, edge.on_curve_records(family, pts), tmp_path, sanitized=sanitized)
        flags = got[:, -1]
        assert set(np.unique(flags)) <= {0, 1} and not got[:, :-1].any()
        assert flags.sum() == accepted
        rec, exp = edge.noncanonical_doubling(family)
        got, _ = edge.run_host(family, rec, tmp_path, sanitized=sanitized)
        wrong = (got != exp).any(axis=1)
        assert (wrong & (flags == 1)).sum() == wrong_doublings
        for at in range(0, got.shape[1] - 1, 8):
            assert edge.below(got[:, at:at + 8], edge.Q).all()
