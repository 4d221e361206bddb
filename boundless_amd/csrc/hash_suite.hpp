// hash_suite.hpp — the hash suites a ctx / a prover / a verification runs under (bx_set_hash_suite), host side.
//
// One place for what depends on the suite outside the kernels: its number and name, its host hashes, RNG and Merkle fold
// (HostSuite).  (The top-layer rule of the Merkle trees belongs to the seal's layout: seal_layout.hpp.)  The device half is the
// launcher table of ctx.hpp (HashLaunchers).  Header-only and free of HIP: verify.cpp / control_id.cpp / image_host.cpp also build with plain g++.  A further
// suite is an entry in the enum and the name table, a case in each function of HostSuite, and a launcher table beside its kernels.
#pragma once
#include <stdint.h>
#include <string.h>

#include <variant>
#include <vector>

#include "../../include/bx_hal.h"
#include "poseidon2_host.hpp"
#include "sha256_suite.hpp"

namespace bx {

enum HashSuite : int { SUITE_POSEIDON2 = 0, SUITE_SHA256 = 1, N_SUITES };
constexpr const char* HASH_SUITE_NAMES[N_SUITES] = {"poseidon2", "sha-256"};  // `ProverOpts::hashfn`
inline int parse_hash_suite(const char* name) {  // -1: not a suite this library implements
    for (int s = 0; name && s < N_SUITES; ++s)
        if (strcmp(name, HASH_SUITE_NAMES[s]) == 0) return s;
    return -1;
}
inline const char* hash_suite_name(int s) { return HASH_SUITE_NAMES[s]; }

// The host half of a hash suite: the element hash of Merkle leaves and of what the transcript absorbs, and the pair hash of Merkle
// interior nodes.  Poseidon2's pair hash is its 16-word sponge; SHA-256's is one compression (sha256_suite.hpp, convention 3).
struct HostSuite {
    int suite = SUITE_POSEIDON2;
    const HostPoseidon2* p2 = nullptr;  // the Poseidon2 table (used under SUITE_POSEIDON2 only)
    // Poseidon2 digest words are field elements (canonical only); SHA-256's are any 32-bit value (sha256_suite.hpp, convention 2)
    bool digests_are_elems() const { return suite == SUITE_POSEIDON2; }
    using Rng = std::variant<Poseidon2Rng, Sha256Rng>;
    Rng rng() const { return suite == SUITE_SHA256 ? Rng(Sha256Rng()) : Rng(Poseidon2Rng(p2)); }  // the suite's Fiat-Shamir RNG, seeded
    void hash_elems(uint32_t out[8], const uint32_t* elems, size_t n) const {
        if (suite == SUITE_SHA256) sha256_hash_elems(out, elems, n);
        else p2->hash_elems(out, elems, n);
    }
    void hash_pair(uint32_t out[8], const uint32_t* a, const uint32_t* b) const {
        if (suite == SUITE_SHA256) return sha256_hash_pair(out, a, b);
        uint32_t pair[16];
        memcpy(pair, a, 32);
        memcpy(pair + 8, b, 32);
        p2->hash_elems(out, pair, 16);
    }
    // Merkle root of a layer of `size` digests (a power of two): 2k digests fold to k until one is left.  `ranges(n, body)` runs
    // body(begin, end) over [0, n): in one piece for the verifier's top layers, split over threads by control_id.cpp.
    template <class Ranges>
    void merkle_root(uint32_t root[8], std::vector<uint32_t> layer, size_t size, Ranges&& ranges) const {
        for (size_t sz = size; sz > 1; sz >>= 1) {
            std::vector<uint32_t> next(8 * (sz / 2));
            ranges(sz / 2, [&](size_t b, size_t e) {
                for (size_t i = b; i < e; ++i) hash_pair(&next[8 * i], &layer[16 * i], &layer[16 * i + 8]);
            });
            layer.swap(next);
        }
        memcpy(root, layer.data(), 32);
    }
};

}  // namespace bx
