// The traffic split's assignment rule, one statement for the host (srn_traffic_split_arms) and the device (srn_arms.hip):
//   u = mix64( mix64(seed ^ 0x53524E5F41524D53) ^ (fold(key) * 0xD1B54A32D192ED03 + 1) ) >> 32,   arm = #{ a < A - 1 : T_a <= u },   T_a = floor(2^32 * (w_0 + .. + w_a) / W)
// from nothing but (seed, weights, key).  fold is the click feedback log's (srn_bootstrap.h), the seed's domain is the split's own: a split and a bootstrap that share
// a seed are still independent.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/serenade_hip.h"
#include "srn_bootstrap.h"   // boot_mix64, boot_fold

namespace srn {

constexpr uint64_t kArmDomain = 0x53524E5F41524D53ull;   // "SRN_ARMS"
constexpr uint64_t kArmNever = 1ull << 32;               // a threshold no u reaches: an arm of weight 0 at the end of the list, and the entries behind A - 1

// thr[a] = T_a for a < A - 1, kArmNever behind: the rule compares all SRN_MAX_ARMS - 1 of them
struct ArmRule { uint64_t rkey; uint64_t thr[SRN_MAX_ARMS - 1]; };

SRN_BOOT_HD uint64_t arm_seed_key(uint64_t seed) { return boot_mix64(seed ^ kArmDomain); }
SRN_BOOT_HD uint32_t arm_draw(uint64_t rkey, uint64_t key_hi, uint64_t key_lo) {
    return (uint32_t)(boot_mix64(rkey ^ (boot_fold(key_hi, key_lo) * 0xD1B54A32D192ED03ull + 1ull)) >> 32);
}
SRN_BOOT_HD uint32_t arm_of(const ArmRule& r, uint64_t key_hi, uint64_t key_lo) {
    const uint64_t u = arm_draw(r.rkey, key_hi, key_lo);
    uint32_t arm = 0;
#pragma unroll
    for (uint32_t a = 0; a < SRN_MAX_ARMS - 1; ++a) arm += r.thr[a] <= u ? 1u : 0u;
    return arm;
}

// weights[0 .. A) -> all[a] = T_a for a < A (all[A - 1] = 2^32), 0 behind; false: W = 0 or W >= 2^32.  Every partial sum is below 2^32, so (sum << 32) fits 64 bits
inline bool arm_thresholds(const uint32_t* weights, size_t n_arms, uint64_t* all, int* why) {
    uint64_t W = 0;
    for (size_t a = 0; a < n_arms; ++a) W += weights[a];
    if (W == 0) { *why = SRN_EINVAL; return false; }
    if (W >= (1ull << 32)) { *why = SRN_ERANGE; return false; }
    uint64_t sum = 0;
    for (size_t a = 0; a < SRN_MAX_ARMS; ++a) { if (a < n_arms) sum += weights[a]; all[a] = a < n_arms ? (sum << 32) / W : 0; }
    return true;
}
inline ArmRule arm_rule(uint64_t seed, const uint64_t* all, size_t n_arms) {
    ArmRule r; r.rkey = arm_seed_key(seed);
    for (size_t a = 0; a < SRN_MAX_ARMS - 1; ++a) r.thr[a] = a + 1 < n_arms ? all[a] : kArmNever;
    return r;
}

}  // namespace srn
