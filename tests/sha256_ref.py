"""Test helper (not collected): the `sha-256` hash suite written from FIPS 180-4 and the suite's conventions alone, sharing no code
with boundless_amd/csrc (transcript.hpp, sha256_suite.hpp).

* a pure-Python SHA-256 compression (checked against hashlib by tests/test_sha256_suite_cpu.py) and a numpy one for many lanes;
* the element hash (hashlib over canonical values as little-endian bytes), the pair hash (one compression over a || b), Sha256Rng;
* a seal replay: parses a `sha-256` seal as the verifier does, re-derives every challenge and the 50 query positions with its own
  RNG, and checks every Merkle opening against the committed top layer.  That is the hash-dependent half of verification; the
  algebraic half (constraint identity, DEEP, FRI arithmetic) is shared with the Poseidon2 path and checked there.
"""
import hashlib

import numpy as np

P = 2013265921
R = (1 << 32) % P
R_INV = pow(R, P - 2, P)
M32 = 0xFFFFFFFF
K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(state, block):
    """One SHA-256 compression: state = 8 ints, block = 64 bytes.  Returns the new state."""
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t]) & M32
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        h, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    return [(x + y) & M32 for x, y in zip(state, [a, b, c, d, e, f, g, h])]


def sha256(msg):
    """Full SHA-256 from `compress` (padding included): 32 bytes."""
    msg = bytes(msg)
    padded = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")
    st = list(IV)
    for i in range(0, len(padded), 64):
        st = compress(st, padded[i:i + 64])
    return b"".join(x.to_bytes(4, "big") for x in st)


def words_of(digest_bytes):
    return np.frombuffer(digest_bytes, dtype="<u4").copy()


def decode(mont):
    return (np.asarray(mont, dtype=np.uint64) * R_INV % P).astype(np.uint32)


def encode(canon):
    return (np.asarray(canon, dtype=np.uint64) % P * R % P).astype(np.uint32)


def elem_hash(mont_words):
    """Convention 1 + 2: SHA-256 of the canonical values as little-endian u32 bytes, read back as 8 little-endian words."""
    return words_of(hashlib.sha256(decode(mont_words).astype("<u4").tobytes()).digest())


def pair_hash(a, b):
    """Convention 3: one compression from the initial state over the 64 bytes a || b, no padding."""
    block = np.asarray(a, np.uint32).astype("<u4").tobytes() + np.asarray(b, np.uint32).astype("<u4").tobytes()
    st = compress(IV, block)
    return words_of(b"".join(x.to_bytes(4, "big") for x in st))


def rows_hash(matrix_cols):
    """Leaves of a column-major (cols, rows) matrix of Montgomery words: one elem_hash per row."""
    m = np.asarray(matrix_cols, np.uint32)
    cols, rows = m.shape
    canon = decode(m.T.reshape(-1)).reshape(rows, cols).astype("<u4")
    out = np.empty((rows, 8), np.uint32)
    for r in range(rows):
        out[r] = words_of(hashlib.sha256(canon[r].tobytes()).digest())
    return out


# ---- many pair hashes at once (numpy lanes): for whole trees ----
def _np_rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def pair_hash_np(a, b):
    """pair_hash over lanes: a, b = (n, 8) digest words -> (n, 8)."""
    a = np.asarray(a, np.uint32)
    b = np.asarray(b, np.uint32)
    w = [x.byteswap() for x in np.concatenate([a, b], axis=1).T]
    for t in range(16, 64):
        s0 = _np_rotr(w[t - 15], 7) ^ _np_rotr(w[t - 15], 18) ^ (w[t - 15] >> np.uint32(3))
        s1 = _np_rotr(w[t - 2], 17) ^ _np_rotr(w[t - 2], 19) ^ (w[t - 2] >> np.uint32(10))
        w.append(w[t - 16] + s0 + w[t - 7] + s1)
    n = a.shape[0]
    st = [np.full(n, v, np.uint32) for v in IV]
    va, vb, vc, vd, ve, vf, vg, vh = st
    for t in range(64):
        t1 = vh + (_np_rotr(ve, 6) ^ _np_rotr(ve, 11) ^ _np_rotr(ve, 25)) + ((ve & vf) ^ (~ve & vg)) + np.uint32(K[t]) + w[t]
        t2 = (_np_rotr(va, 2) ^ _np_rotr(va, 13) ^ _np_rotr(va, 22)) + ((va & vb) ^ (va & vc) ^ (vb & vc))
        vh, vg, vf, ve, vd, vc, vb, va = vg, vf, ve, vd + t1, vc, vb, va, t1 + t2
    out = [s + v for s, v in zip(st, [va, vb, vc, vd, ve, vf, vg, vh])]
    return np.stack(out, axis=1).byteswap()


def merkle_nodes(leaves):
    """The library's node array (2 * rows digests; node 1 = root, leaves at [rows, 2 rows)) from (rows, 8) leaves."""
    leaves = np.asarray(leaves, np.uint32)
    rows = leaves.shape[0]
    nodes = np.zeros((2 * rows, 8), np.uint32)
    nodes[rows:] = leaves
    size = rows
    while size > 1:
        kids = nodes[size:2 * size]
        nodes[size // 2:size] = pair_hash_np(kids[0::2], kids[1::2])
        size //= 2
    return nodes


class Sha256Rng:
    """Convention 4."""

    def __init__(self):
        self.pool0 = words_of(hashlib.sha256(b"Hello").digest())
        self.pool1 = words_of(hashlib.sha256(b"World").digest())
        self.used = 0

    def step(self):
        self.pool0 = pair_hash(self.pool0, self.pool1)
        self.pool1 = pair_hash(self.pool0, self.pool1)
        self.used = 0

    def mix(self, digest):
        self.pool0 = self.pool0 ^ np.asarray(digest, np.uint32)
        self.step()

    def next_u32(self):
        if self.used == 8:
            self.step()
        v = int(self.pool1[self.used])
        self.used += 1
        return v

    def random_bits(self, bits):
        return self.next_u32() & ((1 << bits) - 1)

    def random_elem(self):
        v = 0
        for _ in range(6):
            v = ((v << 32) + self.next_u32()) % P
        return int(encode([v])[0])

    def random_ext(self):
        return [self.random_elem() for _ in range(4)]


QUERIES, FRI_FOLD, FRI_MIN_DEGREE, CHECK_SIZE = 50, 16, 256, 16


def _top_layer(layers):
    top = 0
    for i in range(1, layers):
        if (1 << i) > QUERIES:
            break
        top = i
    return top


class ReplayError(AssertionError):
    pass


def replay_seal(seal):
    """Re-derive the transcript of a `sha-256` seal and check every Merkle opening against its committed top layer with this
    module's hashes.  Returns (challenges, positions).  Raises ReplayError on any mismatch."""
    seal = np.asarray(seal, np.uint32)
    pos = 0

    def take(k):
        nonlocal pos
        if pos + k > seal.size:
            raise ReplayError("seal truncated")
        out = seal[pos:pos + k]
        pos += k
        return out

    rng = Sha256Rng()
    hdr = take(6)
    po2, widths = int(hdr[0]), [int(hdr[1]), int(hdr[2]), int(hdr[3]), CHECK_SIZE]
    rng.mix(elem_hash(encode(hdr)))
    n_globals = 2 if widths[0] >= 2 else 1  # the built-in circuit's public words (csrc/circuit.hpp)
    rng.mix(elem_hash(take(n_globals)))
    N = 1 << po2
    D = 4 * N

    trees = []

    def tree(rows, cols):
        layers = rows.bit_length() - 1
        top = _top_layer(layers)
        ts = 1 << top
        top_nodes = take(8 * ts).reshape(ts, 8).copy()
        layer = top_nodes
        while layer.shape[0] > 1:
            layer = np.stack([pair_hash(layer[2 * i], layer[2 * i + 1]) for i in range(layer.shape[0] // 2)])
        rng.mix(layer[0])
        trees.append(dict(rows=rows, cols=cols, layers=layers, top=top, nodes=top_nodes))

    chal = {}
    tree(D, widths[0])
    tree(D, widths[1])
    chal["beta"] = rng.random_ext()
    tree(D, widths[2])
    chal["poly_mix"] = rng.random_ext()
    tree(D, widths[3])
    chal["Z"] = rng.random_ext()
    # the FRI rounds, the final polynomial and the queries have lengths fixed by the shape: what is left is coeff_u
    sizes, size = [], N
    while size > FRI_MIN_DEGREE:
        sizes.append(size)
        size //= FRI_FOLD
    final_size = size
    fri_shapes = [(4 * s // FRI_FOLD, 4 * FRI_FOLD) for s in sizes]
    all_shapes = [(D, w) for w in widths] + fri_shapes
    tops = sum(8 << _top_layer(r.bit_length() - 1) for r, _ in fri_shapes)
    per_query = sum(c + 8 * ((r.bit_length() - 1) - _top_layer(r.bit_length() - 1)) for r, c in all_shapes)
    n_coeff_u = seal.size - pos - tops - 4 * final_size - QUERIES * per_query
    if n_coeff_u <= 0 or n_coeff_u % 4:
        raise ReplayError("seal length does not fit the shape")
    rng.mix(elem_hash(take(n_coeff_u)))
    chal["mix"] = rng.random_ext()
    chal["fold_mix"] = []
    for rows, cols in fri_shapes:
        tree(rows, cols)
        chal["fold_mix"].append(rng.random_ext())
    rng.mix(elem_hash(take(4 * final_size)))
    bits = D.bit_length() - 1
    positions = [rng.random_bits(bits) % D for _ in range(QUERIES)]
    for q in range(QUERIES):
        p = positions[q]
        for t, tr in enumerate(trees):
            if t >= 4:
                p %= tr["rows"]
            vals = take(tr["cols"])
            cur = elem_hash(vals)
            node = p + tr["rows"]
            while node >= 2 * (1 << tr["top"]):
                sib = take(8)
                cur = pair_hash(sib, cur) if node & 1 else pair_hash(cur, sib)
                node >>= 1
            if not np.array_equal(cur, tr["nodes"][node - (1 << tr["top"])]):
                raise ReplayError(f"query {q}, tree {t}: Merkle opening does not match the committed top layer")
    if pos != seal.size:
        raise ReplayError("trailing words")
    return chal, positions


# ---- the built-in circuit's code group (include/bx_prover.h), for control IDs ----
CODE_SEED = 0x434F4E54524F4C21
MONT_ONE = 268435454


def _splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def code_columns(po2, w_code):
    """(w_code, N) cells of the code group: first, last, then word(cseed, c, r)."""
    n = 1 << po2
    active = n - min(1994, n // 4)
    cols = np.zeros((w_code, n), np.uint32)
    r = np.arange(n, dtype=np.uint64)
    cols[0, 0] = MONT_ONE
    if w_code > 1:
        cols[1, active - 1] = MONT_ONE
    for c in range(2, w_code):
        v = (_splitmix64(np.uint64(CODE_SEED) ^ ((np.uint64(c) << np.uint64(32)) | r)) >> np.uint64(33)).astype(np.uint64)
        cols[c] = np.where(v >= P, v - P, v).astype(np.uint32)
    return cols
