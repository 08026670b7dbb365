#pragma once
// spl_engine_base.h — the engine's bottom layer, part 2: what every kernel stages into and computes with.
// The MT stream limit, the defaults a context starts with, the workgroup -> table-block map, the row store policy
// of spl_step, the LDS blocks (Consts / WaveBuf / BlockLDS) and the byte and `opaque` helpers.  No rules and no
// kernels here.  (It follows spl_engine_stamps.h in spl_engine.hip: the stamp build's device variables keep the
// order they always had.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_common.h"
#include "spl_rng.h"

namespace spl {

// Outputs a lane takes from the register-only MTStream before a LaneMT continuation takes over
// (MTStream::kMaxOut; lowered only by the test hook spl_debug_set_stream_limit, so the parity tests
// can drive every deal and token return through the continuation path).
__device__ int g_stream_limit = MTStream::kMaxOut;

// Per-lane deal scratch in LDS: an odd number of dwords, so lanes at the same Fisher-Yates
// position (the common case: lanes decrement their index in step) hit 64 different banks.
constexpr int kScratchStride = 116;
// rollout-store delegation period a context starts with (spl_ctx_set_rollout_delegation): off.  Alternating
// A/B on one box, 12 launches per arm of 128 steps at 65 536 tables: 1999 +- 25 us off vs
// 1969 +- 34 us every 6th step, a 1.5 % gain (profiles/r03/deleg_ab_r03a.txt) -- under the 2 %
// that would pay for a cross-XCC hand-off in the headline kernel
constexpr int kDelegEveryDefault = 0;
// partner hand-off of the one-workgroup-per-CU rollout stores (six-wave dealer, quad; spl_ctx_set_partner_lead):
// a team hands a step's rows to its neighbouring-XCC partner when that one is this many steps ahead.
// A context starts with 0 (off) since round 6's sc0 nt sc1 row stores (kRollCpol): the teams then lag far less
// and the polls cost more than the hand-off recovers — quad lead 0 / 4 / 8: 1 873-1 898 / 1 909-1 925 /
// 1 912-1 913 us per launch (another box: lead 0 / 4 1 863-1 873 / 1 892-1 900,
// profiles/r06/quad_lead_ab_r06ad.txt); six-wave dealer (C4) 1 075-1 078 / 1 081-1 100 / 1 083-1 102
// (profiles/r06/c4_lead_ab_r06ag.txt).  With nt-only stores lead 4 had paid 2.4 % (headline,
// profiles/r06/headab_r06d.txt) and ~2 % (C4, profiles/r04/partner_ab_r04u.txt).
constexpr int kPartnerLeadDefault = 0;
// Workgroup -> 64-table block, XCD-contiguous.  The dispatcher hands workgroup b to XCD b % 8, so
// with the identity map every XCD writes every eighth 76 KB chunk of a step's rollout-store block;
// mapped, XCD x's workgroups own tables [x n/8, (x+1) n/8) and each XCD streams one contiguous eighth
// of the block (store-only pattern: 880 -> 844-862 us per 64 steps on one box,
// tools/microbench_hbm_store.hip rows_x).  Only which workgroup steps which tables changes: every
// table's chain is its own, so results are identical.  A grid that is no multiple of 8 keeps the identity.
__device__ __forceinline__ int wg_block_of(uint32_t b) {
    const uint32_t nb = gridDim.x;
    if (nb & 7u) return (int)b;
    return (int)((b & 7u) * (nb >> 3) + (b >> 3));
}
__device__ __forceinline__ int wg_block() { return wg_block_of(blockIdx.x); }
// spl_step's int32 rows leave k_step_ws and k_step_wst as `sc1` buffer stores (16: system scope, temporal).
// k_step_ws (four workgroups per CU): 22.35 -> 20.5 us per step at 65 536 tables against plain stores,
// `sc0 sc1` the same, `sc0` alone as plain (profiles/r06/step_ws_temporal_policy_r06an.txt); non-temporal
// rows cost 22.4 -> 23.8 us there (profiles/r06/step_store_policy_ab_r06x.txt), half the block non-temporal
// 22.2 vs 22.4 (profiles/r06/step_ws_split_policy_r06z.txt), non-temporal rows beside a compact copy neutral
// (profiles/r06/dual_opp_rows_nt_r06aa.txt).
// k_step_wst (at most three workgroups per CU): 15.98 -> 15.07 us at 32 768 tables, 20.0 -> 18.2 at 49 152,
// 12.85 -> 12.82 at 16 384 against sc0 nt sc1 (profiles/r06/step_tail_sc1_ab_r06ap.txt), which itself had
// beaten plain stores 17.1 -> 16.0 us at 32 768 tables (profiles/r06/step_tail_store_ab_r06y.txt).
// k_step_wso keeps plain stores (store_obs_block_mid), and so does every spl_step mask block (sc1 there:
// 20.79 vs 20.62 us at 65 536 tables, equal at 32 768; profiles/r06/step_mask_policy_ab_r06ar.txt).
constexpr int kStepRowCpol = 16;

constexpr int kMaskStreamWords = 64 * 45 / 32;  // 90

// constant tables staged per workgroup: 16-B obs-ready card records and 8-B noble records
struct __align__(16) Consts {
    uint4 cards[90];
    uint2 nobles[10];
};

// one wave's output staging
struct __align__(16) WaveBuf {
    uint64_t mask[64];
    uint32_t mbits[96];  // the wave's 64 x 45 mask bits as one stream (store_mask_block)
    uint8_t rows[64 * kObsDim];   // observation staging; also the deal scratch (64 x 112 B)
    uint8_t frows[64 * kObsDim];  // terminal observations (k_rollout): stored with the step's other outputs
};
struct __align__(16) BlockLDS : Consts, WaveBuf {};

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bget(uint32_t w, int k) { return (w >> (8 * k)) & 0xFFu; }
__device__ __forceinline__ uint32_t bset(uint32_t w, int k, uint32_t v) {
    return (w & ~(0xFFu << (8 * k))) | ((v & 0xFFu) << (8 * k));
}

// Launder a value through an empty asm so that a select chain over struct members stays a
// select of VALUES: otherwise LLVM folds "c ? s.a : s.b" into a load at a selected offset,
// which pins the whole struct in scratch memory.
__device__ __forceinline__ uint32_t opaque(uint32_t x) {
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ int opaque(int x) {
    asm("" : "+v"(x));
    return x;
}

}  // namespace spl
