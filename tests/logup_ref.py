"""Big-integer restatement of what the LogUp helpers of include/bx_hal.h compute (bx_batch_invert_ext, bx_batch_invert_elem,
bx_prefix_sums, bx_batch_prefix_sums, bx_logup_accumulate), written from the definitions and sharing no code with the library or
with oracle/:

    Fp   = Z / P,  P = 15 * 2^27 + 1 = 2013265921 (BabyBear)
    Fp4  = Fp[X] / (X^4 + 11)
    a word on the ABI is the Montgomery form  x * 2^32 mod P  of the value x, always the canonical representative in [0, P)

Inverses: Fermat in Fp (x^(P-2)); in Fp4 through the norm map — for a = a0 + a1 X + a2 X^2 + a3 X^3 the product a(X) a(-X) has only
even powers, b0 + b2 X^2, and (b0 + b2 Y)(b0 - b2 Y) = b0^2 + 11 b2^2 with Y = X^2, Y^2 = -11, lies in Fp.  Zero has no inverse; every
function here maps it to zero, which is the library's convention.

Everything works on Python ints (lists of 4 for Fp4).  The array helpers at the bottom convert to and from the uint32 Montgomery words
of the ABI and are what the tests call.
"""
import numpy as np

P = 2013265921
R = (1 << 32) % P
R_INV = pow(R, P - 2, P)
W = 11  # X^4 = -W


def encode(x):
    """value -> Montgomery word"""
    return x % P * R % P


def decode(w):
    """Montgomery word -> value"""
    return w * R_INV % P


# ---- Fp ----
def fp_inv(x):
    return pow(x, P - 2, P)  # 0 -> 0


# ---- Fp4: lists [a0, a1, a2, a3] of values ----
def f4_add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def f4_mul(a, b):
    prod = [0] * 7
    for i in range(4):
        for j in range(4):
            prod[i + j] += a[i] * b[j]
    return [(prod[k] - W * (prod[k + 4] if k < 3 else 0)) % P for k in range(4)]


def f4_scale(a, s):
    return [x * s % P for x in a]


def f4_inv(a):
    a0, a1, a2, a3 = a
    if not (a0 or a1 or a2 or a3):
        return [0, 0, 0, 0]
    # a(X) a(-X) = b0 + b2 X^2
    # (X^4 = -W: the X^4 terms a2^2 - 2 a1 a3 and the X^6 term -a3^2 come back with their signs flipped)
    b0 = (a0 * a0 + W * (2 * a1 * a3 - a2 * a2)) % P
    b2 = (2 * a0 * a2 - a1 * a1 + W * a3 * a3) % P
    norm = (b0 * b0 + W * b2 * b2) % P  # (b0 + b2 Y)(b0 - b2 Y), Y^2 = -W
    ni = fp_inv(norm)
    conj = [a0, -a1 % P, a2, -a3 % P]  # a(-X)
    return f4_mul(conj, [b0 * ni % P, 0, -b2 * ni % P, 0])


# ---- arrays of Montgomery words (what crosses the ABI) ----
def _vals(words):
    return [decode(int(w)) for w in np.asarray(words, dtype=np.uint32).ravel()]


def _words(vals):
    return np.array([encode(v) for v in vals], dtype=np.uint32)


def _ext(words):
    v = _vals(words)
    assert len(v) % 4 == 0
    return [v[i:i + 4] for i in range(0, len(v), 4)]


def _ext_words(elems):
    return _words([x for e in elems for x in e])


def batch_invert_elem(words):
    return _words([fp_inv(v) for v in _vals(words)])


def batch_invert_ext(words):
    return _ext_words([f4_inv(e) for e in _ext(words)])


def ext_mul(a_words, b_words):
    """element-wise Fp4 product of two arrays of AoS ext words"""
    return _ext_words([f4_mul(a, b) for a, b in zip(_ext(a_words), _ext(b_words))])


def elem_mul(a_words, b_words):
    return _words([a * b % P for a, b in zip(_vals(a_words), _vals(b_words))])


def scale_ext(ext_words, mult_words):
    """element-wise: ext element i times base-field element i"""
    return _ext_words([f4_scale(e, m) for e, m in zip(_ext(ext_words), _vals(mult_words))])


def batch_prefix_sums(words, count=1):
    """`count` sequences back to back, each replaced by its inclusive running sum.  Addition commutes with the Montgomery map, so this
    one works on the words directly (numpy, exact in uint64) and stays usable at 2^22 elements."""
    w = np.asarray(words, dtype=np.uint64).reshape(count, -1, 4)
    # a running sum of up to 2^27 words < 2^31 fits 2^58
    assert w.shape[1] <= 1 << 27
    return (np.cumsum(w, axis=1) % P).astype(np.uint32).ravel()


def prefix_sums(words):
    return batch_prefix_sums(words, 1)


def batch_prefix_products(words, count=1):
    e = _ext(words)
    n = len(e) // count
    out = []
    for s in range(count):
        acc = [1, 0, 0, 0]
        for x in e[s * n:(s + 1) * n]:
            acc = f4_mul(acc, x)
            out.append(acc)
    return _ext_words(out)


def logup_accumulate(denom_words, mult_words, count=1):
    """out[s][i] = sum_{j <= i} mults[s][j] / denoms[s][j], the definition, term by term"""
    d = _ext(denom_words)
    m = _vals(mult_words)
    n = len(d) // count
    out = []
    for s in range(count):
        acc = [0, 0, 0, 0]
        for j in range(s * n, (s + 1) * n):
            acc = f4_add(acc, f4_scale(f4_inv(d[j]), m[j]))
            out.append(acc)
    return _ext_words(out)


# ---- the same definitions vectorised for the large cases: uint64 numpy, every product of two values < P reduced before it is added
# to anything (P^2 < 2^62, so one product fits and a sum of two does not) ----
def _m(a, b):
    return a * b % P


def _pow_arr(x, e):
    r = np.ones_like(x)
    while e:
        if e & 1:
            r = _m(r, x)
        x = _m(x, x)
        e >>= 1
    return r


def _decode_arr(words):
    return _m(np.asarray(words, dtype=np.uint64), np.uint64(R_INV))


def _encode_arr(vals):
    return _m(vals, np.uint64(R)).astype(np.uint32)


def _neg(a):
    return (P - a) % P


def batch_invert_elem_big(words):
    return _encode_arr(_pow_arr(_decode_arr(words), P - 2))


def batch_invert_ext_big(words):
    v = _decode_arr(words).reshape(-1, 4)
    a0, a1, a2, a3 = (np.ascontiguousarray(v[:, k]) for k in range(4))
    w = np.uint64(W)
    # b0 = a0^2 + W (2 a1 a3 - a2^2),  b2 = 2 a0 a2 - a1^2 + W a3^2
    t = (2 * _m(a1, a3) % P + _neg(_m(a2, a2))) % P
    b0 = (_m(a0, a0) + _m(w, t)) % P
    b2 = (2 * _m(a0, a2) % P + _neg(_m(a1, a1)) + _m(w, _m(a3, a3))) % P
    ni = _pow_arr((_m(b0, b0) + _m(w, _m(b2, b2))) % P, P - 2)  # a zero element has norm 0 -> 0 -> result 0
    d0, d2 = _m(b0, ni), _neg(_m(b2, ni))
    c0, c1, c2, c3 = a0, _neg(a1), a2, _neg(a3)  # a(-X)
    # (c0 + c1 X + c2 X^2 + c3 X^3)(d0 + d2 X^2), X^4 = -W
    r0 = (_m(c0, d0) + _neg(_m(w, _m(c2, d2)))) % P
    r1 = (_m(c1, d0) + _neg(_m(w, _m(c3, d2)))) % P
    r2 = (_m(c2, d0) + _m(c0, d2)) % P
    r3 = (_m(c3, d0) + _m(c1, d2)) % P
    return _encode_arr(np.stack([r0, r1, r2, r3], axis=1).ravel())


def scale_ext_big(ext_words, mult_words):
    v = _decode_arr(ext_words).reshape(-1, 4)
    m = _decode_arr(mult_words).reshape(-1, 1)
    return _encode_arr(_m(v, m).ravel())


def logup_accumulate_big(denom_words, mult_words, count=1):
    return batch_prefix_sums(scale_ext_big(batch_invert_ext_big(denom_words), mult_words), count)
