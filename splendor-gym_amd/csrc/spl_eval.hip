// spl_eval.hip — the on-device evaluation league (include/splendor_eval.h): the scripted opponents of
// scripts/eval_suite.py as a kernel over a mask and an observation, the legality check before a dual
// step, the per-table tally after it and the reduction per opponent group.
//
// The step kernel fuses three of the policies (spl_engine_deal.h policy_action, fed from the table's state);
// k_scripted runs the same functions of spl_scripted.h fed from the observation, and adds greedy_v2.
// tests/test_gpu_eval_league.py pins the observation-fed kernel to the state-fed one action by action.
#include "../../include/splendor_eval.h"
#include "spl_common.h"
#include "spl_scripted.h"

namespace sple {

using namespace spl;  // kActions, kObsDim; the mask classes, samplers and cascades of spl_scripted.h

constexpr int kBank = 0;           // obs[0:5]: the bank's coloured tokens (engine/encode.py)
constexpr int kBoard = 32;         // obs[32 + 13k ..]: visible card k; its points at + 2
constexpr int kOppPrestige = 30;   // obs: the other player's prestige
constexpr int kTurnCount = 293;    // obs: turn_count

// one observation value of row t, from whichever form the caller gave (the values read here are < 256)
struct ObsRow {
    const int32_t *o32;
    const uint8_t *o8;
    __device__ __forceinline__ int operator[](int i) const { return o32 ? o32[i] : (int)o8[i]; }
};

// eval_suite.py:89-128 with env_ref.state.bank = obs[0:5]
__device__ __forceinline__ int greedy_v2(uint64_t m, const ObsRow &o) {
    if (m & kVisBuyBits) return lowest_action(m & kVisBuyBits);
    if (m & kResBuyBits) return lowest_action(m & kResBuyBits);
    if (!(m & (kTake2Bits | kTake3Bits))) {
        if (m & kReserveBits) return 63 - __clzll((long long)(m & kReserveBits));  // the highest reserve
        return lowest_action(m);
    }
    int bank[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) bank[c] = o[kBank + c];
    int best = 0, best_key = 0x7fffffff;
    if (m & kTake2Bits) {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const bool better = ((m >> (10 + c)) & 1ull) && bank[c] < best_key;  // strict: the first minimum
            best = better ? 10 + c : best;
            best_key = better ? bank[c] : best_key;
        }
        return best;
    }
#pragma unroll
    for (int a = 0; a < 10; ++a) {
        const uint32_t cs = take3_mask(a);
        int sum = 0;
#pragma unroll
        for (int c = 0; c < 5; ++c) sum += ((cs >> c) & 1u) ? bank[c] : 0;
        const bool better = ((m >> a) & 1ull) && sum < best_key;
        best = better ? a : best;
        best_key = better ? sum : best_key;
    }
    return best;
}

// One wave per 64 tables (k_sample's shape): the wave's 64 x 45 mask bytes are read coalesced, as dwords
// where the block is whole and aligned, into LDS; each lane then packs its table's row into a 45-bit word.
__global__ __launch_bounds__(64) void k_scripted(int n, spl_eval_act_t a) {
    __shared__ uint32_t rows_w[64 * kActions / 4];
    int8_t *rows = reinterpret_cast<int8_t *>(rows_w);
    const int t0 = blockIdx.x * 64, lane = (int)threadIdx.x;
    const int nb = min(64, n - t0) * kActions;
    const int8_t *src = a.mask + (size_t)t0 * kActions;
    if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && nb == 64 * kActions) {  // 720 dwords, 12 per lane
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
        uint32_t v[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = lane + 64 * j < 720 ? s4[lane + 64 * j] : 0u;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (lane + 64 * j < 720) rows_w[lane + 64 * j] = v[j];
    } else {
        for (int i = lane; i < nb; i += 64) rows[i] = src[i];
    }
    __syncthreads();
    const int t = t0 + lane;
    if (t >= n) return;
    const int policy = a.policy_of ? a.policy_of[t] : a.policy;
    if (policy == SPL_EVAL_KEEP) return;
    if (policy < SPL_POLICY_UNIFORM || policy > SPL_POLICY_GREEDY_V2) {
        if (a.errors) atomicAdd(reinterpret_cast<unsigned long long *>(a.errors), 1ull);
        return;
    }
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < kActions; ++i) m |= (uint64_t)(rows[lane * kActions + i] != 0) << i;
    const ObsRow o{a.obs ? a.obs + (size_t)t * kObsDim : nullptr,
                   a.obs ? nullptr : a.obs_u8 + (size_t)t * SPL_EVAL_OBS_U8};
    const uint64_t key = a.table_key ? (uint64_t)a.table_key[t] : (uint64_t)(a.table0 + t);
    const uint64_t ply = a.ply + (a.ply_base ? (uint64_t)*a.ply_base : 0ull);
    int act;
    if (policy == SPL_POLICY_GREEDY_V1) act = greedy_v1(m);
    else if (policy == SPL_POLICY_BASIC_PRIORITY)  // o by value: by reference the registers are allocated otherwise
        act = basic_priority(m, [o](int k, bool legal) { return legal ? o[kBoard + 13 * k + 2] : 0; }, a.seed, key,
                             ply);
    else if (policy == SPL_POLICY_GREEDY_V2) act = greedy_v2(m, o);
    else act = sample_uniform(m, a.seed, key, ply);
    a.action[t] = act;
}

__global__ __launch_bounds__(256) void k_check(int n, spl_eval_check_t c) {
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= n || !c.playing[t]) return;
    const int act = c.action[t];
    const bool legal = act >= 0 && act < kActions && c.mask[(size_t)t * kActions + act] != 0;
    c.checks[t] += 1;
    if (!legal) c.illegal[t] += 1;
}

__global__ __launch_bounds__(256) void k_tally(int n, spl_eval_tally_t y) {
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= n || !y.playing[t] || !y.done[t]) return;
    const float r = y.game_ended_on[t] == 1 ? y.agent_step_reward[t] : -y.opp_reward[t];
    y.result[t] = r > 0.f ? 1 : (r < 0.f ? -1 : 0);
    const int32_t *fo = y.final_obs + (size_t)t * kObsDim;
    y.turns[t] = fo[kTurnCount];
    y.prestige[t] = fo[kOppPrestige];
    y.playing[t] = 0;
}

// workgroup g: the eight sums of group g, lane j over tables j, j + 256, ..., then a tree over the lanes
__global__ __launch_bounds__(256) void k_reduce(int n, spl_eval_reduce_t r) {
    __shared__ long long part[SPL_EVAL_COLS][256];
    const int g = blockIdx.x;
    long long s[SPL_EVAL_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = threadIdx.x; t < n; t += 256) {
        if ((r.group_of ? r.group_of[t] : 0) != g) continue;
        const bool live = r.playing[t] != 0;
        const int res = r.result[t];
        s[0] += !live && res > 0;
        s[1] += !live && res < 0;
        s[2] += !live && res == 0;
        s[3] += live;
        s[4] += r.turns[t];
        s[5] += r.prestige[t];
        s[6] += r.checks[t];
        s[7] += r.illegal[t];
    }
#pragma unroll
    for (int c = 0; c < SPL_EVAL_COLS; ++c) part[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int c = 0; c < SPL_EVAL_COLS; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x < SPL_EVAL_COLS) r.out[(size_t)g * SPL_EVAL_COLS + threadIdx.x] = part[threadIdx.x][0];
}

}  // namespace sple

using namespace sple;

extern "C" {

int spl_eval_abi_version(void) { return SPL_EVAL_ABI; }

int spl_eval_scripted_act(int32_t n, const spl_eval_act_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null scripted-act arguments");
    if (!a->mask || !a->action) return spl_fail(SPL_E_ARG, "null buffer: mask and action are required");
    if (!a->obs == !a->obs_u8) return spl_fail(SPL_E_ARG, "exactly one of obs and obs_u8 must be given");
    if (spl_misaligned(a->obs, 4) || spl_misaligned(a->obs_u8, 4) || spl_misaligned(a->action, 4) || spl_misaligned(a->policy_of, 4))
        return spl_fail(SPL_E_ARG, "obs, obs_u8, action and policy_of must be 4-byte aligned");
    if (spl_misaligned(a->table_key, 8) || spl_misaligned(a->ply_base, 8) || spl_misaligned(a->errors, 8))
        return spl_fail(SPL_E_ARG, "table_key, ply_base and errors must be 8-byte aligned");
    if (!a->policy_of && a->policy != SPL_EVAL_KEEP && (a->policy < SPL_POLICY_UNIFORM || a->policy > SPL_POLICY_GREEDY_V2))
        return spl_fail(SPL_E_ARG, "unknown policy");
    hipLaunchKernelGGL(k_scripted, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_scripted");
}

int spl_eval_check(int32_t n, const spl_eval_check_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null check arguments");
    if (!a->action || !a->mask || !a->playing || !a->checks || !a->illegal) return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->action, 4) || spl_misaligned(a->checks, 4) || spl_misaligned(a->illegal, 4))
        return spl_fail(SPL_E_ARG, "action, checks and illegal must be 4-byte aligned");
    hipLaunchKernelGGL(k_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_check");
}

int spl_eval_tally(int32_t n, const spl_eval_tally_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null tally arguments");
    if (!a->done || !a->game_ended_on || !a->agent_step_reward || !a->opp_reward || !a->final_obs || !a->playing ||
        !a->result || !a->turns || !a->prestige)
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->agent_step_reward, 4) || spl_misaligned(a->opp_reward, 4) || spl_misaligned(a->final_obs, 4) ||
        spl_misaligned(a->turns, 4) || spl_misaligned(a->prestige, 4))
        return spl_fail(SPL_E_ARG, "rewards, final_obs, turns and prestige must be 4-byte aligned");
    hipLaunchKernelGGL(k_tally, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_tally");
}

int spl_eval_reduce(int32_t n, int32_t G, const spl_eval_reduce_t *a, void *stream) {
    if (n < 1) return spl_fail(SPL_E_ARG, "n must be positive");
    if (G < 1) return spl_fail(SPL_E_ARG, "G must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null reduce arguments");
    if (!a->playing || !a->result || !a->turns || !a->prestige || !a->checks || !a->illegal || !a->out)
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->out, 8)) return spl_fail(SPL_E_ARG, "out must be 8-byte aligned");
    if (spl_misaligned(a->group_of, 4) || spl_misaligned(a->turns, 4) || spl_misaligned(a->prestige, 4) || spl_misaligned(a->checks, 4) ||
        spl_misaligned(a->illegal, 4))
        return spl_fail(SPL_E_ARG, "group_of, turns, prestige, checks and illegal must be 4-byte aligned");
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, n, *a);
    return spl_launched("k_reduce");
}

}  // extern "C"
