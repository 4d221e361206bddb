// groth16.cpp — host side of the Groth16 prover: zkey parsing and validation (bx_groth16_zkey_inspect*), the snarkjs JSON.
// The layout is stated in groth16.hpp; the device work is in bn254.hip.
#include <stdio.h>
#include <string.h>

#include <string>

#include "groth16.hpp"

namespace {

const uint32_t BN_Q[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
const uint32_t BN_R[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};

thread_local char tl_err[256];

uint32_t rd32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
uint64_t rd64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

bool below(const uint8_t* le32, const uint32_t* m) {
    for (int i = 7; i >= 0; i--) {
        uint32_t w = rd32(le32 + 4 * i);
        if (w != m[i]) return w < m[i];
    }
    return false;
}

// decimal string of an 8-word little-endian number
std::string dec(const uint32_t* w) {
    uint32_t t[8];
    memcpy(t, w, 32);
    std::string s;
    for (;;) {
        bool zero = true;
        uint64_t rem = 0;
        for (int i = 7; i >= 0; i--) {
            uint64_t cur = (rem << 32) | t[i];
            t[i] = (uint32_t)(cur / 10);
            rem = cur % 10;
            zero &= t[i] == 0;
        }
        s.insert(s.begin(), (char)('0' + rem));
        if (zero) break;
    }
    return s;
}

const char* put_json(const std::string& s, char* buf, size_t cap, const char* fn) {
    if (!buf || s.size() + 1 > cap) {
        snprintf(tl_err, sizeof tl_err, "%s: output buffer too small (%zu bytes needed)", fn, s.size() + 1);
        return tl_err;
    }
    memcpy(buf, s.c_str(), s.size() + 1);
    return nullptr;
}

}  // namespace

namespace bx {

const char* zkey_parse(const uint8_t* p, size_t len, ZkeyView* z, char* err, size_t cap) {
#define ZFAIL(...)                            \
    do {                                      \
        snprintf(err, cap, "zkey: " __VA_ARGS__); \
        return err;                           \
    } while (0)
    *z = ZkeyView{};
    if (!p || len < 12) ZFAIL("truncated file (%zu bytes)", len);
    if (memcmp(p, "zkey", 4) != 0) ZFAIL("bad magic (not a zkey file)");
    if (rd32(p + 4) != 1) ZFAIL("unsupported version %u (expected 1)", rd32(p + 4));
    const uint32_t nsec = rd32(p + 8);
    size_t at = 12;
    for (uint32_t i = 0; i < nsec; i++) {
        if (len - at < 12) ZFAIL("truncated file: section table entry %u", i);
        uint32_t type = rd32(p + at);
        uint64_t size = rd64(p + at + 4);
        at += 12;
        if (size > len - at) ZFAIL("truncated file: section %u declares %llu bytes, %zu remain", type, (unsigned long long)size, len - at);
        if (type >= 1 && type <= 10) {
            if (z->sec[type]) ZFAIL("section %u appears twice", type);
            z->sec[type] = p + at;
            z->sec_len[type] = size;
        }
        at += size;
    }
    for (int t = 1; t <= 9; t++)
        if (!z->sec[t]) ZFAIL("section %d missing", t);
    if (z->sec_len[1] != 4 || rd32(z->sec[1]) != 1) ZFAIL("protocol is not Groth16 (section 1 must hold protocol 1)");
    const uint8_t* h = z->sec[2];
    if (z->sec_len[2] != 660) ZFAIL("header section is %llu bytes, expected 660", (unsigned long long)z->sec_len[2]);
    if (rd32(h) != 32 || rd32(h + 36) != 32) ZFAIL("field sizes n8q / n8r are not 32");
    if (memcmp(h + 4, BN_Q, 32) != 0) ZFAIL("q is not BN254's base field prime");
    if (memcmp(h + 40, BN_R, 32) != 0) ZFAIL("r is not BN254's scalar field prime");
    bx_groth16_info& I = z->info;
    I.n_vars = rd32(h + 72);
    I.n_public = rd32(h + 76);
    I.domain_size = rd32(h + 80);
    I.bytes = len;
    const uint64_t n = I.n_vars, npub = I.n_public, N = I.domain_size;
    if (n < 1 || npub + 1 > n) ZFAIL("n_public %u does not fit n_vars %u", I.n_public, I.n_vars);
    if (N == 0 || (N & (N - 1))) ZFAIL("domain size %u is not a power of two", I.domain_size);
    if (N > (1ull << BX_GROTH16_MAX_DOMAIN_LOG)) ZFAIL("domain size %u above 2^%d (the odd coset needs a root of order 2N)", I.domain_size, BX_GROTH16_MAX_DOMAIN_LOG);
    struct {
        int t;
        uint64_t want;
    } sizes[] = {{3, (npub + 1) * 64}, {5, n * 64}, {6, n * 64}, {7, n * 128}, {8, (n - npub - 1) * 64}, {9, N * 64}};
    for (auto& s : sizes)
        if (z->sec_len[s.t] != s.want)
            ZFAIL("section %d is %llu bytes, the header implies %llu", s.t, (unsigned long long)z->sec_len[s.t], (unsigned long long)s.want);
    if (z->sec_len[4] < 4) ZFAIL("section 4 (coefficients) truncated");
    const uint64_t nc = rd32(z->sec[4]);
    if (z->sec_len[4] != 4 + nc * 44) ZFAIL("section 4 is %llu bytes, %llu coefficients need %llu", (unsigned long long)z->sec_len[4], (unsigned long long)nc,
                                            (unsigned long long)(4 + nc * 44));
    I.n_coefs = nc;
    for (uint64_t e = 0; e < nc; e++) {
        const uint8_t* r = z->sec[4] + 4 + e * 44;
        uint32_t m = rd32(r), c = rd32(r + 4), s = rd32(r + 8);
        if (m > 1 || c >= N || s >= n || !below(r + 12, BN_R))
            ZFAIL("coefficient %llu out of range (matrix %u, constraint %u, signal %u)", (unsigned long long)e, m, c, s);
    }
    return nullptr;
#undef ZFAIL
}

}  // namespace bx

extern "C" const char* bx_groth16_zkey_inspect_mem(const void* bytes, size_t len, bx_groth16_info* out) {
    if (!out) return "bx_groth16_zkey_inspect: null output";
    bx::ZkeyView z;
    if (bx::zkey_parse((const uint8_t*)bytes, len, &z, tl_err, sizeof tl_err)) return tl_err;
    *out = z.info;
    return nullptr;
}

extern "C" const char* bx_groth16_zkey_inspect(const char* path, bx_groth16_info* out) try {
    if (!path || !out) return "bx_groth16_zkey_inspect: null argument";
    FILE* f = fopen(path, "rb");
    if (!f) {
        snprintf(tl_err, sizeof tl_err, "bx_groth16_zkey_inspect: cannot open %s", path);
        return tl_err;
    }
    std::string data;
    if (fseek(f, 0, SEEK_END) == 0) {
        long sz = ftell(f);
        if (sz > 0) data.resize((size_t)sz);
        rewind(f);
    }
    size_t got = data.empty() ? 0 : fread(&data[0], 1, data.size(), f);
    fclose(f);
    data.resize(got);
    return bx_groth16_zkey_inspect_mem(data.data(), data.size(), out);
} catch (...) {
    return "bx_groth16_zkey_inspect: out of host memory";
}

extern "C" const char* bx_groth16_proof_json(const bx_groth16_proof* p, char* buf, size_t cap) try {
    if (!p) return "bx_groth16_proof_json: null proof";
    auto q = [](const uint32_t* w) { return "\"" + dec(w) + "\""; };
    std::string s = "{\"pi_a\":[" + q(p->a) + "," + q(p->a + 8) + ",\"1\"],\"pi_b\":[[" + q(p->b) + "," + q(p->b + 8) + "],[" + q(p->b + 16) + "," +
                    q(p->b + 24) + "],[\"1\",\"0\"]],\"pi_c\":[" + q(p->c) + "," + q(p->c + 8) + ",\"1\"],\"protocol\":\"groth16\",\"curve\":\"bn128\"}";
    return put_json(s, buf, cap, "bx_groth16_proof_json");
} catch (...) {
    return "bx_groth16_proof_json: out of host memory";
}

extern "C" const char* bx_groth16_public_json(const bx_groth16_proof* p, char* buf, size_t cap) try {
    if (!p) return "bx_groth16_public_json: null proof";
    if (p->n_public > BX_GROTH16_MAX_PUBLIC) return "bx_groth16_public_json: n_public out of range";
    std::string s = "[";
    for (uint32_t i = 0; i < p->n_public; i++) s += (i ? ",\"" : "\"") + dec(p->public_signals + 8 * i) + "\"";
    s += "]";
    return put_json(s, buf, cap, "bx_groth16_public_json");
} catch (...) {
    return "bx_groth16_public_json: out of host memory";
}
