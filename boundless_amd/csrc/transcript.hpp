// transcript.hpp — host-side Fiat–Shamir transcript of the segment prover (product code, not the oracle).
//
// Restates risc0_zkp::prove::write_iop::WriteIOP (risc0-zkp 3.0.3, reference Cargo.lock:9155) over the suite's RNG: Poseidon2Rng
// (poseidon2_host.hpp) or Sha256Rng (sha256_suite.hpp).  Upstream also runs it on the CPU: a few hundred words per proof.
#pragma once
#include <vector>

#include "hash_suite.hpp"

namespace bx {

// WriteIOP: the seal is the concatenation of everything written; `commit` feeds the suite's RNG, chosen once at construction.
struct Transcript {
    std::vector<uint32_t> seal;
    HostSuite::Rng rng;
    explicit Transcript(const HostSuite& hs) : rng(hs.rng()) {}
    // the one switch over the RNG (two alternatives, hot in the verifier: a branch the compiler inlines through, no visit table)
    template <class F>
    auto with_rng(F&& f) {
        if (Sha256Rng* s = std::get_if<Sha256Rng>(&rng)) return f(*s);
        return f(*std::get_if<Poseidon2Rng>(&rng));
    }
    void reset() { seal.clear(), with_rng([](auto& r) { r.reset(); }); }
    void write(const uint32_t* w, size_t n) { seal.insert(seal.end(), w, w + n); }
    void commit(const uint32_t digest[8]) { with_rng([&](auto& r) { r.mix(digest); }); }
    uint32_t random_elem() { return with_rng([](auto& r) { return r.random_elem(); }); }
    Fp4 random_ext() {
        Fp4 r;
        for (int k = 0; k < 4; ++k) r.c[k] = random_elem();
        return r;
    }
    uint32_t random_bits(unsigned bits) { return with_rng([bits](auto& r) { return r.random_bits(bits); }); }
    // the state prover.hip uploads for the device transcript (a Poseidon2 transcript's only)
    const uint32_t* cells() const { return std::get<Poseidon2Rng>(rng).cells; }
    unsigned pool_used() const { return std::get<Poseidon2Rng>(rng).pool_used; }
};

}  // namespace bx
