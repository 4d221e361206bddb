// groth16_verify.cpp — the host-only Groth16 verifier of include/bx_groth16.h: verifying keys (from a zkey, a loaded key or snarkjs
// JSON), the on-chain seal both ways, bx_groth16_verify / _verify_seal and bx_bn254_pairing_check.  The pairing is in
// bn254_pairing.hpp; the zkey section parser is groth16.cpp's.  No ctx, no HIP call, no mutable global state: messages go to a
// thread-local buffer, the pairing's constants are built once behind a std::call_once.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "bn254_pairing.hpp"
#include "groth16.hpp"

namespace {

using namespace bn;

thread_local char tl_err[256];

const char* fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tl_err, sizeof tl_err, fmt, ap);
    va_end(ap);
    return tl_err;
}

// ---- numbers and points ----
bool all_zero(const uint32_t* w, int n) {
    uint32_t o = 0;
    for (int i = 0; i < n; i++) o |= w[i];
    return o == 0;
}
Fq fq_load(const uint32_t* w) {  // canonical words (< q) -> Montgomery
    Fq a;
    memcpy(a.v, w, 32);
    return to_mont(a);
}
Aff<Fq> g1_load(const uint32_t* w) { return {fq_load(w), fq_load(w + 8)}; }
Aff<Fq2> g2_load(const uint32_t* w) { return {{fq_load(w), fq_load(w + 8)}, {fq_load(w + 16), fq_load(w + 24)}}; }

// Range, curve and (G2) subgroup checks of one point given as canonical words; `what` names it in the message.
// may_be_inf: IC points and the points of a pairing check may be the point at infinity (zeros).
const char* g1_check(const char* fn, const char* what, const uint32_t* w, bool may_be_inf, Aff<Fq>* out) {
    if (ge_mod<FqP>(w) || ge_mod<FqP>(w + 8)) return fail("%s: %s has a coordinate not below q", fn, what);
    if (all_zero(w, 16)) {
        if (!may_be_inf) return fail("%s: %s is the point at infinity", fn, what);
    }
    *out = g1_load(w);
    if (!on_curve(*out)) return fail("%s: %s is not on the curve", fn, what);
    return nullptr;
}
const char* g2_check(const char* fn, const char* what, const uint32_t* w, bool may_be_inf, bool subgroup, Aff<Fq2>* out) {
    for (int i = 0; i < 4; i++)
        if (ge_mod<FqP>(w + 8 * i)) return fail("%s: %s has a coordinate not below q", fn, what);
    if (all_zero(w, 32)) {
        if (!may_be_inf) return fail("%s: %s is the point at infinity", fn, what);
    }
    *out = g2_load(w);
    if (!on_curve(*out)) return fail("%s: %s is not on the curve", fn, what);
    if (subgroup && !in_g2_subgroup(*out)) return fail("%s: %s is not in the subgroup of order r", fn, what);
    return nullptr;
}

struct Vk {
    Aff<Fq> alpha1, ic[BX_GROTH16_MAX_PUBLIC + 1];
    Aff<Fq2> beta2, gamma2, delta2;
};
const char* vk_check(const char* fn, const bx_groth16_vk* vk, bool subgroups, Vk* out) {
    if (vk->n_public > BX_GROTH16_MAX_PUBLIC)
        return fail("%s: the key has %u public signals, more than BX_GROTH16_MAX_PUBLIC (%d)", fn, vk->n_public, BX_GROTH16_MAX_PUBLIC);
    const char* m;
    if ((m = g1_check(fn, "alpha1", vk->alpha1, false, &out->alpha1))) return m;
    if ((m = g2_check(fn, "beta2", vk->beta2, false, subgroups, &out->beta2))) return m;
    if ((m = g2_check(fn, "gamma2", vk->gamma2, false, subgroups, &out->gamma2))) return m;
    if ((m = g2_check(fn, "delta2", vk->delta2, false, subgroups, &out->delta2))) return m;
    for (uint32_t i = 0; i <= vk->n_public; i++) {
        char what[16];
        snprintf(what, sizeof what, "IC[%u]", i);
        if ((m = g1_check(fn, what, vk->ic + 16 * i, true, &out->ic[i]))) return m;
    }
    return nullptr;
}

// zkey points are Montgomery little-endian: n coordinates -> canonical words
const char* from_zkey_coords(const char* fn, const char* what, const uint8_t* src, int n, uint32_t* dst) {
    for (int i = 0; i < n; i++) {
        Fq a;
        memcpy(a.v, src + 32 * i, 32);
        if (ge_mod<FqP>(a.v)) return fail("%s: %s has a coordinate not below q", fn, what);
        a = from_mont(a);
        memcpy(dst + 8 * i, a.v, 32);
    }
    return nullptr;
}
// sections 2 (660 bytes) and 3 ((n_public + 1) * 64 bytes), already validated by zkey_parse
const char* vk_from_sections(const char* fn, const uint8_t* s2, const uint8_t* s3, uint32_t n_public, bx_groth16_vk* out) {
    if (n_public > BX_GROTH16_MAX_PUBLIC)
        return fail("%s: the key has %u public signals, more than BX_GROTH16_MAX_PUBLIC (%d)", fn, n_public, BX_GROTH16_MAX_PUBLIC);
    memset(out, 0, sizeof *out);
    out->n_public = n_public;
    const char* m;
    if ((m = from_zkey_coords(fn, "alpha1", s2 + 84, 2, out->alpha1))) return m;
    if ((m = from_zkey_coords(fn, "beta2", s2 + 212, 4, out->beta2))) return m;
    if ((m = from_zkey_coords(fn, "gamma2", s2 + 340, 4, out->gamma2))) return m;
    if ((m = from_zkey_coords(fn, "delta2", s2 + 532, 4, out->delta2))) return m;
    if ((m = from_zkey_coords(fn, "IC", s3, 2 * (int)(n_public + 1), out->ic))) return m;
    Vk v;
    return vk_check(fn, out, true, &v);
}

// ---- decimal strings ----
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
bool parse_dec(const std::string& s, uint32_t* w) {  // digits only, below 2^256
    memset(w, 0, 32);
    if (s.empty() || s.size() > 78) return false;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        uint64_t c = (uint64_t)(ch - '0');
        for (int i = 0; i < 8; i++) {
            c += (uint64_t)w[i] * 10;
            w[i] = (uint32_t)c;
            c >>= 32;
        }
        if (c) return false;
    }
    return true;
}

// ---- a small JSON reader: objects, arrays, strings, and the text of numbers / literals ----
struct JV {
    enum Kind { Null, Str, Num, Arr, Obj, Lit } kind = Null;
    std::string s;  // Str: the unescaped text; Num / Lit: the token
    std::vector<JV> a;
    std::vector<std::pair<std::string, JV>> o;
    const JV* get(const char* key) const {
        for (auto& kv : o)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
};
struct JParser {
    const char* p;
    const char* end;
    void ws() {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
    }
    bool str(std::string* out) {
        if (p >= end || *p != '"') return false;
        p++;
        while (p < end && *p != '"') {
            if (*p == '\\') {
                if (++p >= end) return false;
                if (*p == 'u') {  // kept as '?': no field this library reads needs it
                    if (end - p < 5) return false;
                    p += 4;
                    out->push_back('?');
                } else {
                    out->push_back(*p == 'n' ? '\n' : *p == 't' ? '\t' : *p);
                }
                p++;
            } else {
                out->push_back(*p++);
            }
        }
        if (p >= end) return false;
        p++;
        return true;
    }
    bool value(JV* v, int depth) {
        if (depth > 16) return false;
        ws();
        if (p >= end) return false;
        if (*p == '"') {
            v->kind = JV::Str;
            return str(&v->s);
        }
        if (*p == '[') {
            v->kind = JV::Arr;
            p++;
            ws();
            if (p < end && *p == ']') return p++, true;
            for (;;) {
                v->a.emplace_back();
                if (!value(&v->a.back(), depth + 1)) return false;
                ws();
                if (p < end && *p == ',') {
                    p++;
                    continue;
                }
                if (p < end && *p == ']') return p++, true;
                return false;
            }
        }
        if (*p == '{') {
            v->kind = JV::Obj;
            p++;
            ws();
            if (p < end && *p == '}') return p++, true;
            for (;;) {
                ws();
                std::string k;
                if (!str(&k)) return false;
                ws();
                if (p >= end || *p != ':') return false;
                p++;
                v->o.emplace_back(std::move(k), JV());
                if (!value(&v->o.back().second, depth + 1)) return false;
                ws();
                if (p < end && *p == ',') {
                    p++;
                    continue;
                }
                if (p < end && *p == '}') return p++, true;
                return false;
            }
        }
        const char* b = p;
        while (p < end && ((*p >= '0' && *p <= '9') || (*p >= 'a' && *p <= 'z') || (*p >= 'A' && *p <= 'Z') || *p == '-' || *p == '+' || *p == '.')) p++;
        if (p == b) return false;
        v->s.assign(b, p);
        v->kind = (v->s[0] == '-' || (v->s[0] >= '0' && v->s[0] <= '9')) ? JV::Num : JV::Lit;
        return true;
    }
};
const char* json_parse(const char* fn, const char* text, size_t len, JV* out) {
    if (!text) return fail("%s: null JSON text", fn);
    JParser jp{text, text + len};
    if (!jp.value(out, 0)) return fail("%s: malformed JSON near byte %zu", fn, (size_t)(jp.p - text));
    jp.ws();
    if (jp.p != jp.end && *jp.p != '\0') return fail("%s: text after the JSON value at byte %zu", fn, (size_t)(jp.p - text));
    return nullptr;
}
// a decimal string (or a bare number) -> 8 words
const char* json_num(const char* fn, const char* what, const JV* v, uint32_t* w) {
    if (!v || (v->kind != JV::Str && v->kind != JV::Num) || !parse_dec(v->s, w))
        return fail("%s: %s is not a decimal number below 2^256", fn, what);
    return nullptr;
}
bool json_is_zero(const JV& v) {
    uint32_t w[8];
    return (v.kind == JV::Str || v.kind == JV::Num) && parse_dec(v.s, w) && all_zero(w, 8);
}
// [x, y, "1"]: 16 words; a third coordinate of "0" is snarkjs's point at infinity
const char* json_g1(const char* fn, const char* what, const JV* v, uint32_t* w) {
    if (!v || v->kind != JV::Arr || v->a.size() < 2 || v->a.size() > 3) return fail("%s: %s is not a list [x, y, \"1\"]", fn, what);
    if (v->a.size() == 3 && json_is_zero(v->a[2])) {
        memset(w, 0, 64);
        return nullptr;
    }
    const char* m;
    if ((m = json_num(fn, what, &v->a[0], w))) return m;
    return json_num(fn, what, &v->a[1], w + 8);
}
// [[x.c0, x.c1], [y.c0, y.c1], ["1", "0"]]: 32 words
const char* json_g2(const char* fn, const char* what, const JV* v, uint32_t* w) {
    if (!v || v->kind != JV::Arr || v->a.size() < 2 || v->a.size() > 3) return fail("%s: %s is not a list [[x.c0, x.c1], [y.c0, y.c1], [\"1\", \"0\"]]", fn, what);
    for (auto& c : v->a)
        if (c.kind != JV::Arr || c.a.size() != 2) return fail("%s: %s is not a list [[x.c0, x.c1], [y.c0, y.c1], [\"1\", \"0\"]]", fn, what);
    if (v->a.size() == 3 && json_is_zero(v->a[2].a[0]) && json_is_zero(v->a[2].a[1])) {
        memset(w, 0, 128);
        return nullptr;
    }
    const char* m;
    for (int i = 0; i < 4; i++)
        if ((m = json_num(fn, what, &v->a[i / 2].a[i % 2], w + 8 * i))) return m;
    return nullptr;
}
const char* put_text(const char* fn, const std::string& s, char* buf, size_t cap) {
    if (!buf || s.size() + 1 > cap) return fail("%s: output buffer too small (%zu bytes needed)", fn, s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return nullptr;
}

void be32_to_words(const uint8_t* be, uint32_t* w) {
    for (int i = 0; i < 8; i++) {
        const uint8_t* b = be + 28 - 4 * i;
        w[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    }
}
void words_to_be32(const uint32_t* w, uint8_t* be) {
    for (int i = 0; i < 8; i++) {
        uint8_t* b = be + 28 - 4 * i;
        b[0] = (uint8_t)(w[i] >> 24), b[1] = (uint8_t)(w[i] >> 16), b[2] = (uint8_t)(w[i] >> 8), b[3] = (uint8_t)w[i];
    }
}
// where each 32-byte number of the seal lives in a proof: A.x A.y B.x.c1 B.x.c0 B.y.c1 B.y.c0 C.x C.y
uint32_t* seal_slot(bx_groth16_proof* p, int i) {
    switch (i) {
        case 0: return p->a;
        case 1: return p->a + 8;
        case 2: return p->b + 8;
        case 3: return p->b;
        case 4: return p->b + 24;
        case 5: return p->b + 16;
        case 6: return p->c;
        default: return p->c + 8;
    }
}

const char* read_file(const char* fn, const char* path, std::string* data) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail("%s: cannot open %s", fn, path);
    if (fseek(f, 0, SEEK_END) == 0) {
        long sz = ftell(f);
        if (sz > 0) data->resize((size_t)sz);
        rewind(f);
    }
    size_t got = data->empty() ? 0 : fread(&(*data)[0], 1, data->size(), f);
    fclose(f);
    data->resize(got);
    return nullptr;
}

const char* verify_impl(const char* fn, const bx_groth16_vk* vk, const bx_groth16_proof* proof) {
    if (!vk || !proof) return fail("%s: null argument", fn);
    if (proof->n_public > BX_GROTH16_MAX_PUBLIC)
        return fail("%s: the proof has %u public signals, more than BX_GROTH16_MAX_PUBLIC (%d)", fn, proof->n_public, BX_GROTH16_MAX_PUBLIC);
    Vk k;
    const char* m;
    if ((m = vk_check(fn, vk, false, &k))) return m;
    if (proof->n_public != vk->n_public)
        return fail("%s: n_public mismatch: the proof has %u public signals, the key takes %u", fn, proof->n_public, vk->n_public);
    for (uint32_t i = 0; i < proof->n_public; i++)
        if (ge_mod<FrP>(proof->public_signals + 8 * i)) return fail("%s: public signal %u is not below r", fn, i);
    Aff<Fq> ps[4];
    Aff<Fq2> qs[4];
    if ((m = g1_check(fn, "A", proof->a, false, &ps[0]))) return m;
    if ((m = g2_check(fn, "B", proof->b, false, true, &qs[0]))) return m;
    if ((m = g1_check(fn, "C", proof->c, false, &ps[3]))) return m;
    // IC_0 + sum x_i IC_i
    Xyzz<Fq> acc = from_aff(k.ic[0]);
    acc = xyzz_add(acc, small_msm(k.ic + 1, proof->public_signals, proof->n_public));
    ps[0].y = neg(ps[0].y);
    ps[1] = k.alpha1;
    qs[1] = k.beta2;
    ps[2] = to_affine(acc);
    qs[2] = k.gamma2;
    qs[3] = k.delta2;
    if (!pairing_product_is_one(ps, qs, 4)) return fail("%s: pairing check failed", fn);
    return nullptr;
}

}  // namespace

#define BX_G16_CATCH(fn)                      \
    catch (...) {                             \
        return fn ": out of host memory";     \
    }

extern "C" const char* bx_groth16_zkey_vk_mem(const void* bytes, size_t len, bx_groth16_vk* out) try {
    if (!out) return "bx_groth16_zkey_vk: null output";
    bx::ZkeyView z;
    if (bx::zkey_parse((const uint8_t*)bytes, len, &z, tl_err, sizeof tl_err)) return tl_err;
    return vk_from_sections("bx_groth16_zkey_vk", z.sec[2], z.sec[3], z.info.n_public, out);
}
BX_G16_CATCH("bx_groth16_zkey_vk")

extern "C" const char* bx_groth16_zkey_vk(const char* path, bx_groth16_vk* out) try {
    if (!path || !out) return "bx_groth16_zkey_vk: null argument";
    std::string data;
    if (const char* m = read_file("bx_groth16_zkey_vk", path, &data)) return m;
    return bx_groth16_zkey_vk_mem(data.data(), data.size(), out);
}
BX_G16_CATCH("bx_groth16_zkey_vk")

extern "C" const char* bx_groth16_key_vk(const bx_groth16_key* key, bx_groth16_vk* out) try {
    if (!key || !out) return "bx_groth16_key_vk: null argument";
    if (key->vk_header.size() != 660 || key->vk_ic.size() != ((size_t)key->info.n_public + 1) * 64)
        return "bx_groth16_key_vk: the key holds no verifying key";
    return vk_from_sections("bx_groth16_key_vk", key->vk_header.data(), key->vk_ic.data(), key->info.n_public, out);
}
BX_G16_CATCH("bx_groth16_key_vk")

extern "C" const char* bx_groth16_vk_json(const bx_groth16_vk* vk, char* buf, size_t cap) try {
    const char* fn = "bx_groth16_vk_json";
    if (!vk) return "bx_groth16_vk_json: null key";
    if (vk->n_public > BX_GROTH16_MAX_PUBLIC) return "bx_groth16_vk_json: n_public out of range";
    auto q = [](const uint32_t* w) { return "\"" + dec(w) + "\""; };
    auto g1 = [&](const uint32_t* w) { return "[" + q(w) + "," + q(w + 8) + ",\"1\"]"; };
    auto g2 = [&](const uint32_t* w) { return "[[" + q(w) + "," + q(w + 8) + "],[" + q(w + 16) + "," + q(w + 24) + "],[\"1\",\"0\"]]"; };
    std::string s = "{\"protocol\":\"groth16\",\"curve\":\"bn128\",\"nPublic\":" + std::to_string(vk->n_public) + ",\"vk_alpha_1\":" + g1(vk->alpha1) +
                    ",\"vk_beta_2\":" + g2(vk->beta2) + ",\"vk_gamma_2\":" + g2(vk->gamma2) + ",\"vk_delta_2\":" + g2(vk->delta2) + ",\"IC\":[";
    for (uint32_t i = 0; i <= vk->n_public; i++) s += (i ? "," : "") + g1(vk->ic + 16 * i);
    s += "]}";
    return put_text(fn, s, buf, cap);
}
BX_G16_CATCH("bx_groth16_vk_json")

extern "C" const char* bx_groth16_vk_from_json(const char* json, size_t len, bx_groth16_vk* out) try {
    const char* fn = "bx_groth16_vk_from_json";
    if (!out) return "bx_groth16_vk_from_json: null output";
    JV root;
    const char* m;
    if ((m = json_parse(fn, json, len, &root))) return m;
    if (root.kind != JV::Obj) return fail("%s: the text is not a JSON object", fn);
    if (const JV* p = root.get("protocol"))
        if (p->s != "groth16") return fail("%s: protocol is not groth16", fn);
    if (const JV* c = root.get("curve"))
        if (c->s != "bn128" && c->s != "bn254") return fail("%s: curve is not bn128", fn);
    const JV* ic = root.get("IC");
    if (!ic || ic->kind != JV::Arr || ic->a.empty()) return fail("%s: IC is not a list of at least one point", fn);
    if (ic->a.size() > BX_GROTH16_MAX_PUBLIC + 1)
        return fail("%s: the key has %zu public signals, more than BX_GROTH16_MAX_PUBLIC (%d)", fn, ic->a.size() - 1, BX_GROTH16_MAX_PUBLIC);
    memset(out, 0, sizeof *out);
    out->n_public = (uint32_t)(ic->a.size() - 1);
    if (const JV* np = root.get("nPublic")) {
        uint32_t w[8];
        if ((m = json_num(fn, "nPublic", np, w))) return m;
        if (!all_zero(w + 1, 7) || w[0] != out->n_public) return fail("%s: nPublic is %s but IC holds %zu points (nPublic + 1 expected)", fn, np->s.c_str(), ic->a.size());
    }
    if ((m = json_g1(fn, "vk_alpha_1", root.get("vk_alpha_1"), out->alpha1))) return m;
    if ((m = json_g2(fn, "vk_beta_2", root.get("vk_beta_2"), out->beta2))) return m;
    if ((m = json_g2(fn, "vk_gamma_2", root.get("vk_gamma_2"), out->gamma2))) return m;
    if ((m = json_g2(fn, "vk_delta_2", root.get("vk_delta_2"), out->delta2))) return m;
    for (size_t i = 0; i < ic->a.size(); i++)
        if ((m = json_g1(fn, "IC", &ic->a[i], out->ic + 16 * i))) return m;
    Vk v;
    return vk_check(fn, out, true, &v);
}
BX_G16_CATCH("bx_groth16_vk_from_json")

extern "C" const char* bx_groth16_proof_from_json(const char* proof_json, size_t proof_len, const char* public_json, size_t public_len,
                                                  bx_groth16_proof* out) try {
    const char* fn = "bx_groth16_proof_from_json";
    if (!out) return "bx_groth16_proof_from_json: null output";
    JV root, pub;
    const char* m;
    if ((m = json_parse(fn, proof_json, proof_len, &root))) return m;
    if (root.kind != JV::Obj) return fail("%s: the proof is not a JSON object", fn);
    if (const JV* p = root.get("protocol"))
        if (p->s != "groth16") return fail("%s: protocol is not groth16", fn);
    memset(out, 0, sizeof *out);
    if ((m = json_g1(fn, "pi_a", root.get("pi_a"), out->a))) return m;
    if ((m = json_g2(fn, "pi_b", root.get("pi_b"), out->b))) return m;
    if ((m = json_g1(fn, "pi_c", root.get("pi_c"), out->c))) return m;
    if (public_json) {
        if ((m = json_parse(fn, public_json, public_len, &pub))) return m;
        if (pub.kind != JV::Arr) return fail("%s: the public signals are not a JSON list", fn);
        if (pub.a.size() > BX_GROTH16_MAX_PUBLIC) return fail("%s: %zu public signals, more than BX_GROTH16_MAX_PUBLIC (%d)", fn, pub.a.size(), BX_GROTH16_MAX_PUBLIC);
        for (size_t i = 0; i < pub.a.size(); i++)
            if ((m = json_num(fn, "a public signal", &pub.a[i], out->public_signals + 8 * i))) return m;
        out->n_public = (uint32_t)pub.a.size();
    }
    return nullptr;
}
BX_G16_CATCH("bx_groth16_proof_from_json")

extern "C" const char* bx_groth16_seal_encode(const bx_groth16_proof* proof, const uint8_t selector[4], uint8_t out[260]) {
    if (!proof || !selector || !out) return "bx_groth16_seal_encode: null argument";
    memcpy(out, selector, 4);
    for (int i = 0; i < 8; i++) words_to_be32(seal_slot(const_cast<bx_groth16_proof*>(proof), i), out + 4 + 32 * i);
    return nullptr;
}

extern "C" const char* bx_groth16_seal_decode(const uint8_t* seal, size_t len, bx_groth16_proof* out) {
    if (!seal || !out) return "bx_groth16_seal_decode: null argument";
    if (len != 256 && len != 260) return fail("bx_groth16_seal_decode: a seal is 260 bytes, or 256 without its selector, not %zu", len);
    memset(out, 0, sizeof *out);
    const uint8_t* p = seal + (len - 256);
    for (int i = 0; i < 8; i++) be32_to_words(p + 32 * i, seal_slot(out, i));
    return nullptr;
}

extern "C" const char* bx_groth16_verify(const bx_groth16_vk* vk, const bx_groth16_proof* proof) try {
    return verify_impl("bx_groth16_verify", vk, proof);
}
BX_G16_CATCH("bx_groth16_verify")

extern "C" const char* bx_groth16_verify_seal(const bx_groth16_vk* vk, const uint8_t* seal, size_t len, const uint8_t claim_digest[32]) try {
    const char* fn = "bx_groth16_verify_seal";
    if (!vk || !seal || !claim_digest) return "bx_groth16_verify_seal: null argument";
    if (len != 256 && len != 260) return fail("%s: a seal is 260 bytes, or 256 without its selector, not %zu", fn, len);
    bx_groth16_proof proof;
    if (const char* m = bx_groth16_seal_decode(seal, len, &proof)) return m;
    // the digest as a big-endian number, reduced mod r (2^256 < 6 r)
    uint32_t* x = proof.public_signals;
    be32_to_words(claim_digest, x);
    while (ge_mod<FrP>(x)) {
        int64_t br = 0;
        for (int i = 0; i < 8; i++) {
            br += (int64_t)x[i] - FrP::m(i);
            x[i] = (uint32_t)br;
            br >>= 32;
        }
    }
    proof.n_public = 1;
    return verify_impl(fn, vk, &proof);
}
BX_G16_CATCH("bx_groth16_verify_seal")

extern "C" const char* bx_bn254_pairing_check(const uint32_t* g1, const uint32_t* g2, size_t n) try {
    const char* fn = "bx_bn254_pairing_check";
    if (n && (!g1 || !g2)) return "bx_bn254_pairing_check: null argument";
    Fq12 f = fq12_one();
    constexpr size_t CHUNK = 32;
    Aff<Fq> ps[CHUNK];
    Aff<Fq2> qs[CHUNK];
    for (size_t at = 0; at < n; at += CHUNK) {
        size_t m = n - at < CHUNK ? n - at : CHUNK;
        for (size_t i = 0; i < m; i++) {
            char what[40];
            snprintf(what, sizeof what, "G1 point %zu", at + i);
            if (const char* e = g1_check(fn, what, g1 + 16 * (at + i), true, &ps[i])) return e;
            snprintf(what, sizeof what, "G2 point %zu", at + i);
            if (const char* e = g2_check(fn, what, g2 + 32 * (at + i), true, true, &qs[i])) return e;
        }
        f = mul(f, multi_miller_loop(ps, qs, m));
    }
    if (!is_one(final_exponentiation(f))) return fail("%s: pairing check failed", fn);
    return nullptr;
}
BX_G16_CATCH("bx_bn254_pairing_check")
