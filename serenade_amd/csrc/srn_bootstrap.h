// The bootstrap's weight rule, one statement for the host (srn_bootstrap_weights) and the device (srn_bootstrap.hip):
//   w(seed, b, s) = #{ i : T[i] <= u },  u = mix64( mix64(seed + (b + 1) * 0x9E3779B97F4A7C15) ^ (s * 0xD1B54A32D192ED03 + 1) ) >> 32
// a Poisson(1) count cut at 12, from nothing but (seed, replicate, session index): not from B, the trial, the index or the chunk.
// The click feedback log (srn_feedback.hip) resamples visitors by the same rule: s = fold(key_hi, key_lo).
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRN_BOOT_HD __host__ __device__ __forceinline__
#else
#define SRN_BOOT_HD inline
#endif

namespace srn {

static constexpr uint32_t kBootMaxWeight = 12;

SRN_BOOT_HD uint64_t boot_mix64(uint64_t x) {   // srn_internal.h mix64
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33; return x;
}

// the replicate's half of the hash: once per replicate
SRN_BOOT_HD uint64_t boot_replicate_key(uint64_t seed, uint32_t b) { return boot_mix64(seed + ((uint64_t)b + 1ull) * 0x9E3779B97F4A7C15ull); }

SRN_BOOT_HD uint32_t boot_weight(uint64_t replicate_key, uint64_t s) {
    // T[i] = round(2^32 * P(Poisson(1) <= i)), i = 0..11
    constexpr uint32_t T[kBootMaxWeight] = {1580030169u, 3160060337u, 3950075422u, 4213413783u, 4279248374u, 4292415292u,
                                            4294609778u, 4294923276u, 4294962463u, 4294966817u, 4294967253u, 4294967292u};
    const uint32_t u = (uint32_t)(boot_mix64(replicate_key ^ (s * 0xD1B54A32D192ED03ull + 1ull)) >> 32);
    uint32_t w = 0;
#pragma unroll
    for (uint32_t i = 0; i < kBootMaxWeight; ++i) w += T[i] <= u ? 1u : 0u;
    return w;
}

// the click feedback log's resampling unit: a visitor's 128-bit key folded to the word boot_weight takes.  boot_mix64 is a bijection, so keys that
// differ in one half fold to different words
SRN_BOOT_HD uint64_t boot_fold(uint64_t key_hi, uint64_t key_lo) { return boot_mix64(key_hi ^ 0x9E3779B97F4A7C15ull) ^ key_lo; }

}  // namespace srn
