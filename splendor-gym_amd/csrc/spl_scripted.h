// spl_scripted.h — the scripted policies over a 45-bit legal mask: the action classes, the uniform
// draw and the k-th-legal-action sampler, and the two scripts/eval_suite.py cascades that the step
// kernels fuse (spl_engine_deal.h policy_action, fed from the table's state) and that k_scripted runs
// beside a network (spl_eval.hip, fed from the observation).  Their random choices are Philox draws
// (sample_uniform over the preferred subset) where the reference calls np.random.choice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_rng.h"

namespace spl {

// the uniform policy's Philox(seed; table, ply) word: independent of the state, so a wave with spare
// time can draw it ahead (the dealer rollout's output wave, two steps ahead of the rules wave)
__device__ __forceinline__ uint32_t uniform_draw(uint64_t seed, uint64_t table, uint64_t ply) {
    return philox4x32(make_uint4((uint32_t)table, (uint32_t)(table >> 32), (uint32_t)ply, (uint32_t)(ply >> 32)),
                      make_uint2((uint32_t)seed, (uint32_t)(seed >> 32))).x;
}
// uniform-random legal action from a drawn word: scaled to the legal count, the k-th legal action
__device__ __forceinline__ int sample_uniform_word(uint64_t m, uint32_t rx) {
    const int n = __popcll(m);
    if (n == 0) return 0;
    int k = (int)(((uint64_t)rx * (uint64_t)n) >> 32);
    // position of the k-th set bit
    uint64_t mm = m;
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const uint64_t low = mm & ((1ull << width) - 1ull);
        const int c = __popcll(low);
        const bool up = k >= c;
        k -= up ? c : 0;
        pos += up ? width : 0;
        mm = up ? (mm >> width) : low;
    }
    return pos;
}
// uniform-random legal action: Philox(seed; table, ply) scaled to the legal count
__device__ __forceinline__ int sample_uniform(uint64_t m, uint64_t seed, uint64_t table, uint64_t ply) {
    return sample_uniform_word(m, uniform_draw(seed, table, ply));
}

// the action classes (engine/encode.py): take-3 0..9, take-2 10..14, buy visible 15..26, reserve 27..41,
// buy reserved 42..44
constexpr uint64_t kVisBuyBits = ((1ull << 12) - 1ull) << 15, kResBuyBits = 7ull << 42;
constexpr uint64_t kBuyBits = kVisBuyBits | kResBuyBits;
constexpr uint64_t kTake2Bits = 0x1Full << 10, kTake3Bits = 0x3FFull, kReserveBits = ((1ull << 15) - 1ull) << 27;
__device__ __forceinline__ int lowest_action(uint64_t m) { return m ? __ffsll((unsigned long long)m) - 1 : 0; }

// take-3 colour sets in itertools.combinations(range(5), 3) order (engine/encode.py:35)
constexpr uint64_t kTake3Masks = (0x07ull) | (0x0Bull << 5) | (0x13ull << 10) | (0x0Dull << 15) |
                                 (0x15ull << 20) | (0x19ull << 25) | (0x0Eull << 30) | (0x16ull << 35) |
                                 (0x1Aull << 40) | (0x1Cull << 45);
__device__ __forceinline__ uint32_t take3_mask(int i) { return (uint32_t)(kTake3Masks >> (5 * i)) & 31u; }

// eval_suite.py:9-29: first legal buy, take-2, take-3, reserve
__device__ __forceinline__ int greedy_v1(uint64_t m) {
    const uint64_t pick = (m & kBuyBits) ? (m & kBuyBits)
                          : (m & kTake2Bits) ? (m & kTake2Bits)
                          : (m & kTake3Bits) ? (m & kTake3Bits)
                          : (m & kReserveBits) ? (m & kReserveBits) : m;
    return lowest_action(pick);
}

// eval_suite.py:32-78; points(k, legal): the points of visible card k (asked for every k; `legal` lets a
// caller that reads memory skip the cards that cannot be bought)
template <class Points>
__device__ __forceinline__ int basic_priority(uint64_t m, Points points, uint64_t seed, uint64_t table, uint64_t ply) {
    const uint64_t vis = m & kVisBuyBits;
    uint64_t pick;
    if (vis) {  // visible buys with the most points
        int best = -1;
        uint64_t best_set = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const bool legal = (vis >> (15 + k)) & 1ull;
            const int pts = points(k, legal);
            const bool better = legal && pts > best, tie = legal && pts == best;
            best_set = better ? (1ull << (15 + k)) : (tie ? (best_set | (1ull << (15 + k))) : best_set);
            best = better ? pts : best;
        }
        pick = best_set;
    } else {
        pick = (m & kResBuyBits) ? (m & kResBuyBits)
               : (m & kTake3Bits) ? (m & kTake3Bits)
               : (m & kTake2Bits) ? (m & kTake2Bits)
               : (m & kReserveBits) ? (m & kReserveBits) : 0ull;
        if (!pick) return lowest_action(m);
    }
    return sample_uniform(pick, seed, table, ply);
}

}  // namespace spl
