"""Big-integer restatement of bx_batch_ratio_products (include/bx_hal.h), written from its definition and sharing no code with the
library:

    out[s][i] = prod_{j <= i} nums[s][j] * denoms[s][j]^-1      in Fp4 = Fp[X] / (X^4 + 11), the inverse sending 0 to 0

over `count` sequences back to back.  A zero denominator therefore contributes the factor 0: the product is 0 from that row on.
Field arithmetic and the word conversions are those of tests/logup_ref.py.

ratio_products is the definition, term by term on Python ints.  ratio_products_big is the same on uint64 numpy arrays for the large
cases: the vectorised inverse of logup_ref, an element-wise product, and the running product as a log-step scan (every element
multiplied by the one 1, 2, 4, .. places before it), which is the definition regrouped by associativity.  by_parts is the call spelt
as the three HAL calls it must agree with (invert, multiply, prefix products); tests/test_ratio_products_cpu.py holds the three
against each other.
"""
import numpy as np

import logup_ref as lr

P = lr.P
W = lr.W


def ratio_products(num_words, denom_words, count=1):
    """the definition: a running product of num * den^-1 per sequence"""
    a, d = lr._ext(num_words), lr._ext(denom_words)
    assert len(a) == len(d) and len(a) % count == 0
    n = len(a) // count
    out = []
    for s in range(count):
        acc = [1, 0, 0, 0]
        for j in range(s * n, (s + 1) * n):
            acc = lr.f4_mul(acc, lr.f4_mul(a[j], lr.f4_inv(d[j])))
            out.append(acc)
    return lr._ext_words(out)


def by_parts(num_words, denom_words, count=1):
    """bx_batch_invert_ext on a copy of the denominators, an element-wise Fp4 product, bx_batch_prefix_products"""
    return lr.batch_prefix_products(lr.ext_mul(num_words, lr.batch_invert_ext(denom_words)), count)


# ---- vectorised: (n, 4) uint64 arrays of plain values ----
def _mul_arr(a, b):
    out = np.zeros_like(a)
    w = np.uint64(W)
    for i in range(4):
        for j in range(4):
            t = a[..., i] * b[..., j] % P
            if i + j >= 4:
                out[..., i + j - 4] = (out[..., i + j - 4] + (P - t * w % P)) % P
            else:
                out[..., i + j] = (out[..., i + j] + t) % P
    return out


def _scan_products(v):
    """(count, n, 4) -> inclusive running products along axis 1, by doubling"""
    v = v.copy()
    n, d = v.shape[1], 1
    while d < n:
        v[:, d:] = _mul_arr(v[:, d:], v[:, :-d])  # the right side is evaluated in full before the assignment
        d *= 2
    return v


def ratio_products_big(num_words, denom_words, count=1):
    inv = lr._decode_arr(lr.batch_invert_ext_big(denom_words)).reshape(count, -1, 4)
    num = lr._decode_arr(num_words).reshape(count, -1, 4)
    return lr._encode_arr(_scan_products(_mul_arr(num, inv)).ravel())
