// sha256_suite.hpp — FIPS 180-4 SHA-256 and the conventions of the `sha-256` hash suite (host and device).
//
// One place for everything the `sha-256` suite fixes: the compression function (also what the device kernels of sha256.hip run),
// the streaming hash (image_host.cpp's SystemState digest), and how the suite turns field elements and digests into bytes.
// Header-only: verify.cpp / control_id.cpp / image_host.cpp also build with plain g++.
//
// Conventions [EXT: risc0-zkp 3.0.3 core/hash/sha, recalled, not vendored; re-verify against an upstream vector]:
//   1. Element hash (hash_elem_slice: Merkle leaves = rows, and everything the transcript hashes): standard SHA-256 with padding
//      over the byte string formed by each element's CANONICAL value (decoded from Montgomery, < P) as 4 little-endian bytes.
//      Zero elements hash the empty string.  Alternative, if upstream hashes the raw Montgomery words: SHA_ELEM_CANONICAL = false.
//   2. Digest words: the 32 output bytes of SHA-256 read as 8 little-endian u32.  They are NOT field elements: any value occurs.
//   3. Pair hash (hash_pair: Merkle interior nodes, hash_fold): ONE compression from the initial state over the 64-byte block
//      a || b, no padding block; the result serialised as in 2.
//   4. Sha256Rng (Fiat-Shamir): pool0 = SHA-256("Hello"), pool1 = SHA-256("World"), used = 0.
//      mix(d): pool0 ^= d word-wise, step().  step(): pool0 = pair(pool0, pool1); pool1 = pair(pool0, pool1) (the new pool0);
//      used = 0.  next_u32(): if used == 8 step(); return pool1[used++].  random_bits(b) = next_u32() & (2^b - 1).
//      random_elem: v = 0; six times v = ((v << 32) + next_u32()) mod P; Montgomery-encode v.  random_ext = four random_elem.
//      Committing a root is mix(root); the header, globals, coeff_u and the final coefficients are element-hashed, then mixed.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fp.hpp"

namespace bx {

// the element hash reads canonical values (true) or raw Montgomery words (false): convention 1's one switch
constexpr bool SHA_ELEM_CANONICAL = true;

BX_HD constexpr uint32_t sha256_k(int t) {
    constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    return K[t];
}
BX_HD constexpr uint32_t sha256_iv(int i) {
    constexpr uint32_t H0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    return H0[i];
}

BX_HD uint32_t sha_rotr(uint32_t x, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, n);  // v_alignbit_b32
#else
    return (x >> n) | (x << (32 - n));
#endif
}
// Three-input bit functions as one v_bitop3_b32 each (gfx950 has no v_xor3_b32; left to itself the compiler keeps the Sigma
// functions as pairs of two-input xors and Maj as three instructions).  The immediate is the truth table over (a, b, c) =
// (0xF0, 0xCC, 0xAA).
#if defined(__HIP_DEVICE_COMPILE__)
#define BX_SHA_BITOP3(TABLE, EXPR)                                                                  \
    uint32_t r;                                                                                     \
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:" #TABLE : "=v"(r) : "v"(a), "v"(b), "v"(c));         \
    return r;
#else
#define BX_SHA_BITOP3(TABLE, EXPR) return (EXPR);
#endif
BX_HD uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { BX_SHA_BITOP3(0x96, a ^ b ^ c) }
BX_HD uint32_t sha_ch(uint32_t a, uint32_t b, uint32_t c) { BX_SHA_BITOP3(0xCA, (a & b) | (~a & c)) }
BX_HD uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { BX_SHA_BITOP3(0xE8, (a & b) | (a & c) | (b & c)) }
#undef BX_SHA_BITOP3
BX_HD uint32_t sha_bswap(uint32_t x) { return __builtin_bswap32(x); }  // v_perm_b32 on the device
// the byte of an element that goes into the message, as a big-endian message word (convention 1)
BX_HD uint32_t sha_elem_word(uint32_t mont) { return sha_bswap(SHA_ELEM_CANONICAL ? fp_decode(mont) : mont); }

// One compression: st = st + F(st, w), w = 16 big-endian message words (consumed: the schedule rolls through it in place).
// Written so that gfx950 gets v_alignbit_b32 rotates, one v_bitop3_b32 for each of Ch, Maj and the three-input xors, v_add3_u32 sums.
BX_HD void sha256_compress(uint32_t* st, uint32_t* w) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < 64; ++t) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint32_t s0 = sha_xor3(sha_rotr(w15, 7), sha_rotr(w15, 18), w15 >> 3);
            const uint32_t s1 = sha_xor3(sha_rotr(w2, 17), sha_rotr(w2, 19), w2 >> 10);
            w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t S1 = sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25));
        const uint32_t t1 = h + S1 + sha_ch(e, f, g) + sha256_k(t) + w[t & 15];
        const uint32_t S0 = sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22));
        const uint32_t maj = sha_maj(a, b, c);
        h = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + S0 + maj;
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}

// ---- host side ----

// FIPS 180-4 over a byte stream (also the SystemState digest of image_host.cpp)
struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t buf[64];
    size_t fill = 0;
    uint64_t total = 0;
    void block(const uint8_t* p) {
        uint32_t w[16];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        sha256_compress(h, w);
    }
    void update(const uint8_t* p, size_t n) {
        total += n;
        while (n) {
            size_t take = 64 - fill < n ? 64 - fill : n;
            memcpy(buf + fill, p, take);
            fill += take, p += take, n -= take;
            if (fill == 64) block(buf), fill = 0;
        }
    }
    void finish(uint8_t out[32]) {
        const uint64_t bits = total * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while (fill != 56) update(&zero, 1);
        uint8_t lenb[8];
        for (int k = 0; k < 8; ++k) lenb[k] = (uint8_t)(bits >> (8 * (7 - k)));
        update(lenb, 8);
        for (int k = 0; k < 8; ++k) out[4 * k] = h[k] >> 24, out[4 * k + 1] = h[k] >> 16, out[4 * k + 2] = h[k] >> 8, out[4 * k + 3] = h[k];
    }
};

// convention 1 + 2: element hash of n Montgomery words -> 8 digest words
inline void sha256_hash_elems(uint32_t out[8], const uint32_t* elems, size_t n) {
    uint32_t st[8], w[16];
    for (int i = 0; i < 8; ++i) st[i] = sha256_iv(i);
    size_t i = 0;
    for (; i + 16 <= n; i += 16) {
        for (int k = 0; k < 16; ++k) w[k] = sha_elem_word(elems[i + k]);
        sha256_compress(st, w);
    }
    // the tail, the 0x80 byte and the 64-bit bit length: one block if at most 13 words are left, else two
    const size_t r = n - i;
    const uint64_t bits = (uint64_t)n * 32;
    for (int blk = 0; blk < (r <= 13 ? 1 : 2); ++blk) {
        for (int k = 0; k < 16; ++k) {
            const size_t idx = 16 * (size_t)blk + k;
            w[k] = idx < r ? sha_elem_word(elems[i + idx]) : idx == r ? 0x80000000u : 0u;
        }
        if (blk == (r <= 13 ? 0 : 1)) w[14] = (uint32_t)(bits >> 32), w[15] = (uint32_t)bits;
        sha256_compress(st, w);
    }
    for (int k = 0; k < 8; ++k) out[k] = sha_bswap(st[k]);
}
// convention 3: one compression over a || b from the initial state
inline void sha256_hash_pair(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {
    uint32_t st[8], w[16];
    for (int k = 0; k < 8; ++k) st[k] = sha256_iv(k), w[k] = sha_bswap(a[k]), w[8 + k] = sha_bswap(b[k]);
    sha256_compress(st, w);
    for (int k = 0; k < 8; ++k) out[k] = sha_bswap(st[k]);
}
inline void sha256_digest_of_bytes(uint32_t out[8], const char* s) {
    Sha256 h;
    h.update((const uint8_t*)s, strlen(s));
    uint8_t d[32];
    h.finish(d);
    for (int k = 0; k < 8; ++k) out[k] = (uint32_t)d[4 * k] | (uint32_t)d[4 * k + 1] << 8 | (uint32_t)d[4 * k + 2] << 16 | (uint32_t)d[4 * k + 3] << 24;
}

// convention 4
struct Sha256Rng {
    uint32_t pool0[8], pool1[8];
    unsigned used = 0;
    Sha256Rng() { reset(); }
    void reset() {
        sha256_digest_of_bytes(pool0, "Hello");
        sha256_digest_of_bytes(pool1, "World");
        used = 0;
    }
    void step() {
        sha256_hash_pair(pool0, pool0, pool1);
        sha256_hash_pair(pool1, pool0, pool1);
        used = 0;
    }
    void mix(const uint32_t d[8]) {
        for (int k = 0; k < 8; ++k) pool0[k] ^= d[k];
        step();
    }
    uint32_t next_u32() {
        if (used == 8) step();
        return pool1[used++];
    }
    uint32_t random_bits(unsigned bits) {
        const uint32_t v = next_u32();
        return bits >= 32 ? v : (v & ((1u << bits) - 1u));
    }
    uint32_t random_elem() {
        uint64_t v = 0;
        for (int i = 0; i < 6; ++i) v = ((v << 32) + next_u32()) % P;
        return fp_encode((uint32_t)v);
    }
};

}  // namespace bx
