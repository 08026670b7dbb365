// spl_search.hip — the pick of a one-ply search (include/splendor_search.h spl_search_pick): per table the legal
// action of greatest q over the [45][n] planes that spl_successors (spl_engine.hip, with the engine's kernels)
// and a value call wrote; spl_search_pick_pairs is the same pick over the compacted planes of spl_successors_pairs.
// No engine layer here: the kernels read planes, not the table state.
#include "../../include/splendor_search.h"
#include "spl_common.h"

namespace spls {

using namespace spl;  // kActions

// One lane per table; plane a of a wave's 64 tables is one coalesced load per input.
__global__ __launch_bounds__(256) void k_pick(int n, spl_pick_args_t p) {
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= n) return;
    float best = -__builtin_inff();
    int act = -1, first = -1;
#pragma unroll 5
    for (int a = 0; a < kActions; ++a) {
        const size_t i = (size_t)a * (size_t)n + t;
        const uint32_t f = p.flags[i];
        const float q = (f & SPL_SUCC_TERMINATED) ? p.reward[i] : p.sign * p.value[i];
        const bool legal = (f & SPL_SUCC_LEGAL) != 0u;
        first = (legal && first < 0) ? a : first;
        const bool better = legal && q > best;  // false for a NaN: it never wins; a tie keeps the lower a
        best = better ? q : best;
        act = better ? a : act;
    }
    p.action[t] = act >= 0 ? act : first;
    if (p.best_q) p.best_q[t] = best;
}

// spl_search_pick_pairs: one wave per 64-table block walks the block's runs in the contract's order.  `run` is the
// index of action a's first pair; a lane whose table allows a reads the pair at run + its rank among those lanes.
__global__ __launch_bounds__(256) void k_pick_pairs(int n, spl_pick_pairs_args_t p) {
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    if ((t & ~63) >= n) return;  // wave-uniform: the whole block is past the tables
    const uint64_t lg = t < n ? p.legal[t] : 0ull;
    int run = p.base[t >> 6];
    float best = -__builtin_inff();
    int act = -1, first = -1;
    for (int a = 0; a < kActions; ++a) {
        const bool bit = ((lg >> a) & 1ull) != 0ull;
        const uint64_t bal = __ballot(bit);
        const int i = run + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        run += __popcll(bal);
        if (bit && i < p.capacity) {  // a pair past the capacity takes no part
            const float q = (p.flags[i] & SPL_SUCC_TERMINATED) ? p.reward[i] : p.sign * p.value[i];
            first = first < 0 ? a : first;
            const bool better = q > best;  // false for a NaN: it never wins; a tie keeps the lower a
            best = better ? q : best;
            act = better ? a : act;
        }
    }
    if (t >= n) return;
    p.action[t] = act >= 0 ? act : first;
    if (p.best_q) p.best_q[t] = best;
}

}  // namespace spls

extern "C" {

int spl_search_pick(int32_t n, const spl_pick_args_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null pick arguments");
    if (!a->flags || !a->reward || !a->value || !a->action) return spl_fail(SPL_E_ARG, "null buffer: flags, reward, value and action are required");
    if (spl_misaligned(a->reward, 4) || spl_misaligned(a->value, 4) || spl_misaligned(a->action, 4) || spl_misaligned(a->best_q, 4))
        return spl_fail(SPL_E_ARG, "reward, value, action and best_q must be 4-byte aligned");
    hipLaunchKernelGGL(spls::k_pick, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_pick");
}

int spl_search_pick_pairs(int32_t n, const spl_pick_pairs_args_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null pick arguments");
    if (!a->legal || !a->base || !a->flags || !a->reward || !a->value || !a->action)
        return spl_fail(SPL_E_ARG, "null buffer: legal, base, flags, reward, value and action are required");
    if (spl_misaligned(a->legal, 8)) return spl_fail(SPL_E_ARG, "legal must be 8-byte aligned");
    if (spl_misaligned(a->base, 4) || spl_misaligned(a->reward, 4) || spl_misaligned(a->value, 4) || spl_misaligned(a->action, 4) ||
        spl_misaligned(a->best_q, 4))
        return spl_fail(SPL_E_ARG, "base, reward, value, action and best_q must be 4-byte aligned");
    if (a->capacity < 1) return spl_fail(SPL_E_ARG, "capacity must be positive");
    hipLaunchKernelGGL(spls::k_pick_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_pick_pairs");
}

}  // extern "C"
