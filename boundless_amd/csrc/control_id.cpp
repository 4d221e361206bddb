// control_id.cpp — the verifier's half of the code-group binding (include/bx_circuit.h): VerifierContext, the synthetic
// circuit's check_code, and the definition-level host computation of its control IDs.  Host code only.
//
// Reference: `segment_receipt.verify_integrity_with_context(&agent.verifier_ctx)` (bento/crates/workflow/src/tasks/prove.rs:53-55,
// `verifier_ctx` built at lib.rs:241) ends in risc0_zkp::verify::verify(circuit, suite, seal, check_code) [EXT: risc0-zkp 3.0.3],
// whose `check_code(po2, root)` closure refuses a seal whose code-group Merkle root is not one of the circuit's control IDs
// (risc0-zkvm: `verifier_parameters.control_ids.contains(control_id)`); the generated table one level up is
// contracts/src/blake3-groth16/ControlID.sol:13.  Without that comparison the selectors and control words a seal's constraints
// are evaluated with are the prover's own choice (Weak #2: a code group with `last` == 0 proves any g_1).
//
// The host computation below shares no code with the device path (ntt.hip / poseidon2.hip) nor with the test oracle: plain
// iterative radix-2 transforms in natural order — coefficients by an inverse DFT on <w_N>, the coset shift as a_j * 3^j, the 4N
// evaluations by a zero-padded forward DFT (row i = f(3 * w_4N^i)) — then the row and pair hashes of hash_suite.hpp.
#include <stdio.h>
#include <string.h>

#include <array>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/bx_circuit.h"
#include "circuit.hpp"
#include "lookup.hpp"
#include "trace_layout.hpp"
#include "fp.hpp"
#include "poseidon2_params.hpp"
#include "hash_suite.hpp"

namespace {
using namespace bx;
using Digest = std::array<uint32_t, 8>;

uint32_t root_of_unity(unsigned k) { return fp_pow(fp_encode(137u), (uint64_t)1 << (27 - k)); }  // w_{2^k}, Montgomery

// out[i] = sum_j a[j] * w^(i j), natural order in and out (bit-reversal permutation + decimation-in-time butterflies)
void dft_natural(uint32_t* a, unsigned log_n, uint32_t w) {
    const size_t n = (size_t)1 << log_n;
    for (size_t i = 0; i < n; ++i) {
        const size_t j = log_n ? (size_t)(bit_reverse32((uint32_t)i) >> (32 - log_n)) : 0;
        if (i < j) std::swap(a[i], a[j]);
    }
    std::vector<uint32_t> tw(n / 2 ? n / 2 : 1);
    for (unsigned s = 1; s <= log_n; ++s) {
        const size_t half = (size_t)1 << (s - 1);
        const uint32_t ws = fp_pow(w, (uint64_t)1 << (log_n - s));  // primitive 2^s-th root
        tw[0] = MONT_ONE;
        for (size_t k = 1; k < half; ++k) tw[k] = fp_mul(tw[k - 1], ws);
        for (size_t base = 0; base < n; base += 2 * half)
            for (size_t k = 0; k < half; ++k) {
                const uint32_t u = a[base + k], v = fp_mul(a[base + k + half], tw[k]);
                a[base + k] = fp_add(u, v);
                a[base + k + half] = fp_sub(u, v);
            }
    }
}

unsigned worker_count(size_t items) {
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    if (hw > 16) hw = 16;
    return (unsigned)(items < hw ? (items ? items : 1) : hw);
}
template <class F>
void parallel_ranges(size_t n, F&& body) {  // body(begin, end)
    const unsigned t = worker_count(n / 1024 + 1);
    if (t <= 1) {
        body((size_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t chunk = (n + t - 1) / t;
    for (unsigned i = 0; i < t; ++i) {
        const size_t b = (size_t)i * chunk, e = b + chunk < n ? b + chunk : n;
        if (b < e) th.emplace_back([&body, b, e] { body(b, e); });
    }
    for (auto& x : th) x.join();
}

// Merkle root of the committed code group of a built-in circuit for (po2, w_code) under a hash suite; cell(col, row) is the
// circuit's code cell
// (a functor: the call is inlined into the column loop); `who` holds the entry point's two refusals
struct HostIdErrors {
    const char *range, *too_large;
};
constexpr HostIdErrors SYNTH_ID_ERRORS = {
    "bx_synthetic_control_id_host: shape out of range",
    "bx_synthetic_control_id_host: the code group is too large for the host computation (build a verifier context from bx_prover_control_id instead)"};
constexpr HostIdErrors LOOKUP_ID_ERRORS = {
    "bx_lookup_control_id_host: shape out of range (po2 in [9, 24], w_code >= 3 and below 65536)",
    "bx_lookup_control_id_host: the code group is too large for the host computation (build a verifier context from bx_prover_control_id instead)"};
template <class CodeCell>
const char* host_control_id(uint32_t po2, uint32_t wc, int suite, const CodeCell& cell, const HostIdErrors& who, uint32_t out[8]) {
    if (po2 < 9 || po2 > 24 || wc < 1 || wc >= 65536) return who.range;
    const size_t n = (size_t)1 << po2, dom = 4 * n;
    if ((double)wc * (double)dom * 4.0 > 6.0e9) return who.too_large;
    std::vector<uint32_t> ev((size_t)wc * dom);
    const uint32_t w_n_inv = fp_inv(root_of_unity(po2)), w_dom = root_of_unity(po2 + 2), n_inv = fp_inv(fp_encode((uint32_t)n));
    {
        std::vector<std::thread> th;
        const unsigned t = worker_count(wc);
        for (unsigned k = 0; k < t; ++k)
            th.emplace_back([&, k] {
                for (uint32_t c = k; c < wc; c += t) {
                    uint32_t* col = &ev[(size_t)c * dom];
                    for (size_t r = 0; r < n; ++r) col[r] = cell(c, (uint32_t)r);
                    dft_natural(col, po2, w_n_inv);  // coefficients * N
                    uint32_t shift = n_inv;          // 3^j / N
                    for (size_t j = 0; j < n; ++j) {
                        col[j] = fp_mul(col[j], shift);
                        shift = fp_mul(shift, MONT_THREE);
                    }
                    memset(col + n, 0, (dom - n) * 4);
                    dft_natural(col, po2 + 2, w_dom);  // col[i] = f(3 w_4N^i)
                }
            });
        for (auto& x : th) x.join();
    }
    HostPoseidon2 h2;
    h2.load(POSEIDON2_RC, POSEIDON2_DIAG);
    const HostSuite h{suite, &h2};
    std::vector<uint32_t> layer(8 * dom);
    parallel_ranges(dom, [&](size_t b, size_t e) {
        std::vector<uint32_t> row(wc);
        for (size_t r = b; r < e; ++r) {
            for (uint32_t c = 0; c < wc; ++c) row[c] = ev[(size_t)c * dom + r];
            h.hash_elems(&layer[8 * r], row.data(), wc);
        }
    });
    ev.clear();
    ev.shrink_to_fit();
    h.merkle_root(out, std::move(layer), dom, [](size_t n, auto&& body) { parallel_ranges(n, body); });
    return nullptr;
}

// ---- the generated table (tools/gen_control_ids.py): w_code = 16, po2 9..24 — upstream ships the same thing as control_id.rs ----
struct TableRow {
    uint32_t po2;
    uint32_t id[8];
};
#if !defined(BX_NO_CONTROL_TABLE)
const TableRow SYNTH_CONTROL_IDS_W16[] = {
#include "control_ids_w16.inc"
};
const size_t N_TABLE = sizeof SYNTH_CONTROL_IDS_W16 / sizeof SYNTH_CONTROL_IDS_W16[0];
#else
const TableRow* const SYNTH_CONTROL_IDS_W16 = nullptr;
const size_t N_TABLE = 0;
#endif

std::mutex cache_mu;
enum BuiltIn : uint32_t { BUILTIN_SYNTHETIC = 0, BUILTIN_LOOKUP = 1 };
std::map<std::array<uint32_t, 4>, Digest> cache;  // (circuit, po2, w_code, suite) -> host-computed control ID

constexpr HostIdErrors LAYOUT_ID_ERRORS = {
    "bx_trace_layout_control_id_host: shape out of range (po2 in [9, 24])",
    "bx_trace_layout_control_id_host: the code group is too large for the host computation (build a verifier context from bx_prover_control_id instead)"};

// the cached host computation for one of the built-in circuits
const char* cached_control_id(BuiltIn which, uint32_t po2, uint32_t wc, int suite, uint32_t out[8]) {
    const std::array<uint32_t, 4> key{(uint32_t)which, po2, wc, (uint32_t)suite};
    {
        std::lock_guard<std::mutex> g(cache_mu);
        auto it = cache.find(key);
        if (it != cache.end()) {
            memcpy(out, it->second.data(), 32);
            return nullptr;
        }
    }
    Digest d;
    const char* e;
    if (which == BUILTIN_LOOKUP) {
        if (wc < 3) return LOOKUP_ID_ERRORS.range;
        const Lookup lk(po2, wc, 4, 12);  // only po2 / w_code enter the code group
        e = host_control_id(po2, wc, suite, [&lk](uint32_t c, uint32_t r) { return lookup_code_cell(lk, c, r); }, LOOKUP_ID_ERRORS, d.data());
    } else {
        const Circuit cc(po2, wc, 1, 1, 1, 1);
        e = host_control_id(po2, wc, suite, [&cc](uint32_t c, uint32_t r) { return synth_code_cell(cc, c, r); }, SYNTH_ID_ERRORS, d.data());
    }
    if (e) return e;
    std::lock_guard<std::mutex> g(cache_mu);
    cache[key] = d;
    memcpy(out, d.data(), 32);
    return nullptr;
}

const char* synth_control_id(uint32_t po2, uint32_t wc, int suite, uint32_t out[8], bool use_table) {
    if (use_table && wc == 16 && suite == SUITE_POSEIDON2)  // the generated table holds Poseidon2 IDs
        for (size_t i = 0; i < N_TABLE; ++i)
            if (SYNTH_CONTROL_IDS_W16[i].po2 == po2) {
                memcpy(out, SYNTH_CONTROL_IDS_W16[i].id, 32);
                return nullptr;
            }
    return cached_control_id(BUILTIN_SYNTHETIC, po2, wc, suite, out);
}
}  // namespace

namespace bx {
const char* synth_check_code_suite(const bx_segment_params* s, const uint32_t root[8], int suite) {
    if (!s || !root) return "check_code: null argument";
    uint32_t id[8];
    if (const char* e = synth_control_id(s->po2, s->w_code, suite, id, true)) return e;
    return memcmp(id, root, 32) == 0 ? nullptr : "the code group's root is not this circuit's control ID for the shape (the seal was made with another code group)";
}
const char* synth_check_code(void*, const bx_segment_params* s, const uint32_t root[8]) {
    return synth_check_code_suite(s, root, SUITE_POSEIDON2);  // a table's check_code has no suite parameter: the default one
}
const char* lookup_check_code_suite(const bx_segment_params* s, const uint32_t root[8], int suite) {
    if (!s || !root) return "check_code: null argument";
    uint32_t id[8];
    if (const char* e = cached_control_id(BUILTIN_LOOKUP, s->po2, s->w_code, suite, id)) return e;
    return memcmp(id, root, 32) == 0 ? nullptr : "the code group's root is not the lookup circuit's control ID for the shape (the seal was made with another code group)";
}
const char* lookup_check_code(void*, const bx_segment_params* s, const uint32_t root[8]) {
    return lookup_check_code_suite(s, root, SUITE_POSEIDON2);
}
// a trace layout's code group through the same definition-level path (trace_layout_host.cpp checks the shape and caches the result)
const char* layout_host_control_id(const bx_trace_layout* l, uint32_t po2, int suite, uint32_t out[8]) {
    const uint32_t n = 1u << (po2 & 31u), act = layout_active_rows(po2 & 31u, l->noise_rows);
    const bx_layout_code_col* code = l->code.data();
    const uint32_t* table = l->table.data();
    return host_control_id(po2, (uint32_t)l->code.size(), suite, [=](uint32_t c, uint32_t r) { return layout_code_cell(code[c], table, c, r, n, act); },
                           LAYOUT_ID_ERRORS, out);
}
// the built-in circuits' control IDs follow the hash suite (a table's check_code has no suite parameter): what verify.cpp asks under a
// suite other than the default when it has no context.  Any other table (a plug-in circuit) is refused.
const char* builtin_check_code_suite(const bx_circuit_ops* circ, const bx_segment_params* s, const uint32_t root[8], int suite) {
    if (circ == bx_synthetic_circuit()) return synth_check_code_suite(s, root, suite);
    if (circ && circ->check_code == lookup_check_code) return lookup_check_code_suite(s, root, suite);  // bx_lookup_circuit(), without linking its device half
    return "no control IDs of this suite for the circuit (a plug-in circuit needs a verifier context)";
}
}  // namespace bx

struct bx_verifier_ctx {
    struct Id { int suite; uint32_t po2; Digest digest; };
    std::vector<Id> ids;  // a set, every suite's IDs together
};

namespace bx {
// what verify.cpp asks a context: is `root` one of the IDs registered for po2?
bool verifier_ctx_contains_suite(const bx_verifier_ctx* v, int suite, uint32_t po2, const uint32_t root[8]) {
    for (auto& e : v->ids)
        if (e.suite == suite && e.po2 == po2 && memcmp(e.digest.data(), root, 32) == 0) return true;
    return false;
}
bool verifier_ctx_contains(const bx_verifier_ctx* v, uint32_t po2, const uint32_t root[8]) {
    return verifier_ctx_contains_suite(v, SUITE_POSEIDON2, po2, root);  // the form without a suite means the default one
}
}  // namespace bx

extern "C" {

const char* bx_synthetic_control_id_host(uint32_t po2, uint32_t w_code, uint32_t id_out[8]) {
    return bx_synthetic_control_id_host_hashfn(po2, w_code, "poseidon2", id_out);
}
const char* bx_synthetic_control_id_host_hashfn(uint32_t po2, uint32_t w_code, const char* hashfn, uint32_t id_out[8]) {
    static thread_local char err[256];
    const int suite = parse_hash_suite(hashfn);
    if (suite < 0) return "bx_synthetic_control_id_host: unknown hashfn (\"poseidon2\" or \"sha-256\")";
    if (!id_out) return "bx_synthetic_control_id_host: null output";
    try {
        if (const char* e = synth_control_id(po2, w_code, suite, id_out, false)) {
            snprintf(err, sizeof err, "%s", e);
            return err;
        }
        return nullptr;
    } catch (const std::exception& e) {
        snprintf(err, sizeof err, "bx_synthetic_control_id_host: %s", e.what());
        return err;
    }
}

const char* bx_lookup_control_id_host_hashfn(uint32_t po2, uint32_t w_code, const char* hashfn, uint32_t id_out[8]) {
    static thread_local char err[256];
    const int suite = parse_hash_suite(hashfn);
    if (suite < 0) return "bx_lookup_control_id_host: unknown hashfn (\"poseidon2\" or \"sha-256\")";
    if (!id_out) return "bx_lookup_control_id_host: null output";
    try {
        if (const char* e = cached_control_id(BUILTIN_LOOKUP, po2, w_code, suite, id_out)) {
            snprintf(err, sizeof err, "%s", e);
            return err;
        }
        return nullptr;
    } catch (const std::exception& e) {
        snprintf(err, sizeof err, "bx_lookup_control_id_host: %s", e.what());
        return err;
    }
}

const char* bx_verifier_ctx_create(bx_verifier_ctx** out) {
    if (!out) return "bx_verifier_ctx_create: out is NULL";
    *out = new (std::nothrow) bx_verifier_ctx();
    return *out ? nullptr : "bx_verifier_ctx_create: out of memory";
}
void bx_verifier_ctx_destroy(bx_verifier_ctx* v) { delete v; }
const char* bx_verifier_ctx_add_control_id(bx_verifier_ctx* v, uint32_t po2, const uint32_t id[8]) {
    return bx_verifier_ctx_add_control_id_hashfn(v, po2, id, "poseidon2");  // the ABI without a hashfn means the default suite
}
const char* bx_verifier_ctx_add_control_id_hashfn(bx_verifier_ctx* v, uint32_t po2, const uint32_t id[8], const char* hashfn) {
    const int suite = parse_hash_suite(hashfn);
    if (suite < 0) return "bx_verifier_ctx_add_control_id: unknown hashfn (\"poseidon2\" or \"sha-256\")";
    if (!v || !id) return "bx_verifier_ctx_add_control_id: null argument";
    if (po2 < 9 || po2 > 24) return "bx_verifier_ctx_add_control_id: po2 must be in [9, 24]";
    for (int i = 0; i < 8; ++i)
        if (HostSuite{suite}.digests_are_elems() && id[i] >= bx::P) return "bx_verifier_ctx_add_control_id: a digest word is not a canonical field element";
    try {
        bx_verifier_ctx::Id d{suite, po2, {}};
        memcpy(d.digest.data(), id, 32);
        if (!bx::verifier_ctx_contains_suite(v, suite, po2, id)) v->ids.push_back(d);
        return nullptr;
    } catch (const std::exception&) {
        return "bx_verifier_ctx_add_control_id: out of memory";
    }
}
size_t bx_verifier_ctx_size(const bx_verifier_ctx* v) { return v ? v->ids.size() : 0; }
size_t bx_verifier_ctx_count(const bx_verifier_ctx* v, uint32_t po2) {
    size_t n = 0;
    if (v)
        for (auto& e : v->ids) n += e.po2 == po2;
    return n;
}

}  // extern "C"
