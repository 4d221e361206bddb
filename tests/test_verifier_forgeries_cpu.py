"""CPU: forged seals that only the verifier's DEEP and FRI checks can refuse.

After the constraint identity, two compares of csrc/verify.cpp are not hash compares, and they are what ties the committed trace to
ONE polynomial of low degree: "FRI layer value does not match the value carried from the previous layer" (in round 0 it binds FRI's
first layer to the DEEP quotient of the opened rows, later it is the fold chain) and "final polynomial does not match the last FRI
fold".  Word flips never reach them: a flip in front of the queries moves the query positions and a flip inside a query breaks its
hash path, so the Merkle compare answers first.  The seals here come from a prover that proves a TRUE statement, lies in exactly
one place and is otherwise self-consistent (oracle/bx_oracle.h: bxo_set_prover_fault) — it commits what it computed from the lie,
draws its challenges from that transcript and opens honestly from what it committed.

For every forgery:
  * the verdict is the expected one, by its full text, on 1 and on 8 verification threads and through an explicit VerifierContext
    that holds the honest control ID;
  * the forged seal is word for word the honest seal of the same shape and seed up to the first word the lie can influence (an
    offset computed from the shape), so every check in front of it saw honest data;
  * the transcript is replayed here with the oracle's hashes and every Merkle opening of the forged seal is recomputed: except
    for the one opening OPEN_NEIGHBOUR moves, all of them match their committed top layer — no hash compare refuses the seal, the
    named arithmetic check does;
  * the honest seal of the same shape and seed verifies.

Shapes: (9, 2/3/2) and (10, 4/8/4) have one FRI round (final sizes 32 and 64); (13, 2/9/6) is the smallest size with a second
round (N / 16 > 256), where the fold chain between two committed layers exists.
"""
import functools

import numpy as np
import pytest

from boundless_amd.hal import HalError
from boundless_amd.prover import VerifierContext, set_verify_threads, verify_seal
from oracle import oracle_lib as ol

QUERIES, FRI_FOLD, FRI_MIN_DEGREE, CHECK_SIZE, MAX_TOP_LAYER = 50, 16, 256, 16, 5

PREFIX = "bx_verify_segment: "
MERKLE = "Merkle opening does not match the committed top layer"
IDENTITY = "constraint identity fails at Z"
LAYER = "FRI layer value does not match the value carried from the previous layer"
FINAL = "final polynomial does not match the last FRI fold"

SHAPES = [(9, (2, 3, 2), 11), (10, (4, 8, 4), 1234), (13, (2, 9, 6), 5)]  # (po2, widths, seed)
SHAPE_IDS = [f"po2_{po2}" for po2, _, _ in SHAPES]
ONE = int(ol.encode([1])[0])


class Layout:
    """Where the words of a synthetic-circuit seal stand, from the shape alone (include/bx_prover.h; as `_regions` in
    test_verifier_cpu.py, for any shape)."""

    def __init__(self, po2, widths):
        wc, wd, wa = widths
        self.po2, self.N, self.D = po2, 1 << po2, 4 << po2
        self.widths = [wc, wd, wa, CHECK_SIZE]
        accs = wa // 4
        taps = [[1] * wc, [2 if c % 8 == 0 else 3 if c % 8 == 4 else 1 for c in range(wd)],
                [2 if c < 4 * accs else 1 for c in range(wa)], [1] * CHECK_SIZE]
        self.n_globals = 2 if wc >= 2 else 1
        self.check_tap_first = sum(sum(t) for t in taps[:3])  # first check column's ext element of coeff_u
        self.total_taps = self.check_tap_first + CHECK_SIZE
        self.sizes = []
        size = self.N
        while size > FRI_MIN_DEGREE:
            self.sizes.append(size)
            size //= FRI_FOLD
        self.final_size = size
        self.trees = [(self.D, w) for w in self.widths] + [(4 * s // FRI_FOLD, 4 * FRI_FOLD) for s in self.sizes]  # (rows, cols)
        at = 6 + self.n_globals
        self.top_at = []
        for t, (rows, _) in enumerate(self.trees):
            if t == 4:
                self.coeff_u_at = at
                at += 4 * self.total_taps
            self.top_at.append(at)
            at += 8 * self.top_size(rows)
        self.final_at = at
        self.queries_at = at + 4 * self.final_size
        self.query_off = [0]
        for rows, cols in self.trees:
            self.query_off.append(self.query_off[-1] + cols + 8 * (rows.bit_length() - 1 - self.top_layer(rows)))
        self.per_query = self.query_off[-1]
        self.seal_words = self.queries_at + QUERIES * self.per_query

    @staticmethod
    def top_layer(rows):
        return min(rows.bit_length() - 2, MAX_TOP_LAYER)  # the deepest layer with at most 50 nodes, below the leaves

    def top_size(self, rows):
        return 1 << self.top_layer(rows)

    def opening(self, q, t):
        """(first word, one past the last word) of query q's opening of tree t"""
        at = self.queries_at + q * self.per_query
        return at + self.query_off[t], at + self.query_off[t + 1]


def replay(seal, lay):
    """The verifier's transcript with the oracle's own sponge and generator: the 50 query positions, and the (query, tree) of
    every opening whose recomputed path does not end in the committed top layer."""
    L = ol.lib()
    seal = np.ascontiguousarray(seal, np.uint32)
    state = np.zeros(25, np.uint32)

    def commit_elems(words):
        nonlocal state
        dg = np.zeros(8, np.uint32)
        w = np.ascontiguousarray(words, np.uint32)
        L.bxo_hash_elem_slice(dg, w, w.size, 1)
        state, _ = ol.transcript_step(state, dg, 0)

    def draw_ext():
        nonlocal state
        state, _ = ol.transcript_step(state, np.zeros(0, np.uint32), 4)

    def commit_tree(t):
        nonlocal state
        ts = lay.top_size(lay.trees[t][0])
        top = seal[lay.top_at[t]:lay.top_at[t] + 8 * ts].reshape(ts, 8).copy()
        layer = top
        while layer.shape[0] > 1:
            nxt = np.zeros((layer.shape[0] // 2, 8), np.uint32)
            for i in range(nxt.shape[0]):
                L.bxo_hash_pair(nxt[i], layer[2 * i].copy(), layer[2 * i + 1].copy())
            layer = nxt
        state, _ = ol.transcript_step(state, layer[0], 0)
        return top

    commit_elems(ol.encode(seal[:6]))
    commit_elems(seal[6:6 + lay.n_globals])
    tops = [commit_tree(0), commit_tree(1)]
    draw_ext()  # the accumulators' mix
    tops.append(commit_tree(2))
    draw_ext()  # poly_mix
    tops.append(commit_tree(3))
    draw_ext()  # Z
    commit_elems(seal[lay.coeff_u_at:lay.coeff_u_at + 4 * lay.total_taps])
    draw_ext()  # the DEEP mix
    for t in range(4, len(lay.trees)):
        tops.append(commit_tree(t))
        draw_ext()  # the round's fold mix
    commit_elems(seal[lay.final_at:lay.final_at + 4 * lay.final_size])
    positions = [int(L.bxo_rng_random_bits(state, lay.D.bit_length() - 1)) % lay.D for _ in range(QUERIES)]
    bad = []
    for q, pos in enumerate(positions):
        for t, (rows, cols) in enumerate(lay.trees):
            first, _ = lay.opening(q, t)
            idx = pos % rows
            cur, nxt = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
            L.bxo_hash_elem_slice(cur, seal[first:first + cols].copy(), cols, 1)
            node, at = idx + rows, first + cols
            while node >= 2 * lay.top_size(rows):
                sib = seal[at:at + 8].copy()
                at += 8
                if node & 1:
                    L.bxo_hash_pair(nxt, sib, cur)
                else:
                    L.bxo_hash_pair(nxt, cur, sib)
                cur, nxt = nxt, cur
                node >>= 1
            if not np.array_equal(cur, tops[t][node - lay.top_size(rows)]):
                bad.append((q, t))
    return positions, bad


@functools.lru_cache(maxsize=None)
def honest(po2, widths, seed):
    seal, roots = ol.prove_segment(po2, *widths, seed)
    seal.setflags(write=False)
    return seal, roots


def forge(kind, a, b, po2, widths, seed):
    seal, roots = ol.prove_segment_with_fault(kind, a, b, po2, *widths, seed)
    return seal


def verdict(seal, ctx=None):
    try:
        verify_seal(seal, ctx=ctx)
    except HalError as e:
        return str(e)
    return "DID NOT RAISE"


def check_forgery(forged, shape, expected, first_word, moved_openings=()):
    """The asserts every forgery shares (module docstring); returns (honest seal, layout, replayed positions)."""
    po2, widths, seed = shape
    good, roots = honest(*shape)
    lay = Layout(po2, widths)
    assert good.size == forged.size == lay.seal_words
    # the lie is where it should be: honest data in front of it, and something else from there on
    assert np.array_equal(forged[:first_word], good[:first_word])
    assert not np.array_equal(forged[first_word:], good[first_word:])
    # the prover stayed self-consistent: every opening but the ones the lie moved ends in the top layer it committed
    positions, bad = replay(forged, lay)
    assert bad == list(moved_openings)
    want = PREFIX + expected
    try:
        for threads in (1, 8):
            set_verify_threads(threads)
            assert verdict(forged) == want, threads
    finally:
        set_verify_threads(0)
    assert verdict(forged, ctx=VerifierContext().add_control_id(po2, roots[0])) == want
    verify_seal(good)
    return good, lay, positions


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_with_the_hook_off_the_seal_is_the_honest_one_and_the_layout_here_is_the_seals(shape):
    po2, widths, seed = shape
    good, roots = honest(*shape)
    lay = Layout(po2, widths)
    assert good.size == lay.seal_words
    L = ol.lib()
    L.bxo_set_prover_fault(ol.FAULT_FINAL, 0, 0)
    L.bxo_set_prover_fault(ol.FAULT_NONE, 0, 0)  # switched on and off again: nothing stays behind
    again, roots_again = ol.prove_segment(po2, *widths, seed)
    assert again.tobytes() == good.tobytes() and np.array_equal(roots, roots_again)
    positions, bad = replay(good, lay)  # the replay used below is the verifier's: on an honest seal every opening checks
    assert bad == [] and len(set(positions)) > 40
    verify_seal(good)
    verify_seal(good, ctx=VerifierContext().add_control_id(po2, roots[0]))


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_false_tap_claim_that_keeps_the_constraint_identity_is_refused_by_the_deep_quotient(shape, k):
    """Check column 4k is claimed to be Z^2 more, column 4k+1 one less, at Z^4/3: the verifier's 1 * g_4k + Z^2 * g_4k+1 does not
    move, so the constraint identity holds for values the committed columns do not take.  Only the DEEP quotient recomputed from
    the opened rows, compared with FRI's first layer, can tell."""
    forged = forge(ol.FAULT_TAP_PAIR, k, 1, *shape)
    lay = Layout(shape[0], shape[1])
    at = lay.coeff_u_at + 4 * (lay.check_tap_first + 4 * k)
    good, lay, _ = check_forgery(forged, shape, LAYER, at)
    u = slice(lay.coeff_u_at, lay.coeff_u_at + 4 * lay.total_taps)
    differ = np.flatnonzero((forged[u] != good[u]).reshape(-1, 4).any(axis=1))
    assert differ.tolist() == [lay.check_tap_first + 4 * k, lay.check_tap_first + 4 * k + 1]  # exactly two ext elements
    minus_one = (good[at + 4:at + 8].astype(np.int64) - [ONE, 0, 0, 0]) % ol.P
    assert np.array_equal(forged[at + 4:at + 8], minus_one)


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_same_false_tap_claim_without_its_compensation_fails_the_constraint_identity(shape, k):
    """The control of the test above: with only the first half of the lie the identity is the check that answers."""
    forged = forge(ol.FAULT_TAP_PAIR, k, 0, *shape)
    lay = Layout(shape[0], shape[1])
    at = lay.coeff_u_at + 4 * (lay.check_tap_first + 4 * k)
    good, lay, _ = check_forgery(forged, shape, IDENTITY, at)
    u = slice(lay.coeff_u_at, lay.coeff_u_at + 4 * lay.total_taps)
    differ = np.flatnonzero((forged[u] != good[u]).reshape(-1, 4).any(axis=1))
    assert differ.tolist() == [lay.check_tap_first + 4 * k]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_low_degree_fri_that_is_not_the_quotient_of_the_trace_is_refused_in_round_0(shape):
    """One added to the constant coefficient of the DEEP sum: FRI's layers, folds and final polynomial are all consistent and of
    low degree, every tap claim is true; the first layer just is not what the opened rows give."""
    forged = forge(ol.FAULT_LAYER0_SHIFT, 0, 0, *shape)
    lay = Layout(shape[0], shape[1])
    check_forgery(forged, shape, LAYER, lay.top_at[4])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_last_round_folded_with_another_mix_is_refused_by_the_final_polynomial(shape):
    lay = Layout(shape[0], shape[1])
    forged = forge(ol.FAULT_FOLD_MIX, len(lay.sizes) - 1, 0, *shape)
    check_forgery(forged, shape, FINAL, lay.final_at)


def test_a_first_round_folded_with_another_mix_is_refused_by_the_fold_chain_in_round_1():
    """po2 13: round 0's layer is the honest DEEP quotient, so the compare passes in round 0; round 1 commits the wrong fold of it
    and is itself folded honestly into the final polynomial, so only the compare in round 1 can answer."""
    shape = SHAPES[2]
    lay = Layout(shape[0], shape[1])
    assert len(lay.sizes) == 2
    forged = forge(ol.FAULT_FOLD_MIX, 0, 0, *shape)
    check_forgery(forged, shape, LAYER, lay.top_at[5])


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_final_polynomial_with_one_coefficient_off_is_refused(shape, which):
    lay = Layout(shape[0], shape[1])
    j = 0 if which == "first" else lay.final_size - 1
    forged = forge(ol.FAULT_FINAL, j, 0, *shape)
    good, lay, _ = check_forgery(forged, shape, FINAL, lay.final_at + j)
    fin = slice(lay.final_at, lay.final_at + 4 * lay.final_size)
    assert np.flatnonzero(forged[fin] != good[fin]).tolist() == [j]
    assert int(forged[lay.final_at + j]) == (int(good[lay.final_at + j]) + ONE) % ol.P


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_committed_last_layer_that_is_no_polynomial_is_refused_where_a_query_meets_it(shape):
    """Every second row of the last round's evaluation matrix is off by one in every word, and committed so.  A query that opens
    such a row carries another value into it; one that opens none of them passes, which is FRI's soundness error: here 2^-50,
    and the replayed positions show that this seed is not that case."""
    lay = Layout(shape[0], shape[1])
    r = len(lay.sizes) - 1
    forged = forge(ol.FAULT_ROWS, r, 2, *shape)
    _, lay, positions = check_forgery(forged, shape, LAYER, lay.top_at[4 + r])
    rows = lay.trees[4 + r][0]
    assert any((pos % rows) % 2 == 0 for pos in positions)


# trees 1 and 3 are the data and the check group, 4 is FRI round 0; po2 13 alone has a tree 5, its second round
NEIGHBOURS = [(shape, q, t) for shape in SHAPES for q in (0, 49) for t in (1, 3, 4, 5) if t < 4 + len(Layout(shape[0], shape[1]).sizes)]


@pytest.mark.parametrize("shape,q,t", NEIGHBOURS, ids=[f"po2_{s[0]}-query_{q}-tree_{t}" for s, q, t in NEIGHBOURS])
def test_an_authentic_row_opened_beside_the_drawn_position_is_refused(shape, q, t):
    """The row and its path are the committed tree's, for the leaf next to the one the transcript drew: the path must be hashed at
    the drawn position.  Nothing else of the seal changes (the queries commit nothing), and with q = 49 the 49 queries in front
    pass on every thread count."""
    lay = Layout(shape[0], shape[1])
    forged = forge(ol.FAULT_OPEN_NEIGHBOUR, q, t, *shape)
    first, end = lay.opening(q, t)
    good, lay, _ = check_forgery(forged, shape, MERKLE, first, moved_openings=[(q, t)])
    assert np.array_equal(forged[end:], good[end:])
    assert not np.array_equal(forged[first:first + lay.trees[t][1]], good[first:first + lay.trees[t][1]])  # another row


@pytest.mark.parametrize("t", [1, 4])
def test_an_honest_row_under_the_path_of_another_query_is_refused_by_the_hash_compare_alone(t):
    """The counterpart: every value the arithmetic reads is honest, and the last query's row stands under the siblings of query
    0's opening of the same tree — authentic digests, in the wrong place.  No DEEP or FRI compare can see it; a neighbour's row, above,
    would still be refused by them."""
    shape = SHAPES[1]
    good, _ = honest(*shape)
    lay = Layout(shape[0], shape[1])
    cols = lay.trees[t][1]
    (first0, end0), (first49, end49) = lay.opening(0, t), lay.opening(49, t)
    forged = good.copy()
    forged[first49 + cols:end49] = good[first0 + cols:end0]
    moved = first49 + cols + int(np.flatnonzero(forged[first49 + cols:end49] != good[first49 + cols:end49])[0])
    check_forgery(forged, shape, MERKLE, moved, moved_openings=[(49, t)])
