#pragma once
// spl_engine_ws.h — what every multi-wave kernel shares: the rules / output split and its LDS block (PtShared,
// WsLDS), tab_word / set_tab_word, the reward and episode codes of the packed small outputs (pack_small), ws_sync,
// and the bounded LDS waits' pieces (kSpinLimit, g_spin_limit, signal_fault).
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_step.h"
#include "spl_layout.h"

namespace spl {

// ---- two-wave pipelined rollout -----------------------------------------------------------
// k_rollout as a two-stage pipeline per 64 tables: workgroup = 2 waves, lane l of both = table
// t0 + l.  The RULES wave runs the steps (SplendorEnv.step, autoreset, policy, small outputs,
// fused refill) and hands each step's table state to the OUTPUT wave through LDS; the output
// wave encodes the observation rows (and the terminal rows) and issues the step's block stores
// while the rules wave already computes the next step.  With one wave per table block, a step
// was the rules' dependency chains PLUS the store issue stalls of one instruction stream
// (k_rollout: 12.4 us of the 15 us step with the observation stores compiled out); split over
// two waves on two SIMDs, the step costs the longer of the two stages.
//
// Hand-off per step k (buffers k & 1, so the rules wave refills buffer b only after the output
// wave has passed the next barrier, i.e. finished with it): the state words after the step
// (post-autoreset), the info mask, and the terminal (pre-autoreset) states of the first kTerm
// terminal lanes; the rules wave writes any further terminal rows itself (store_row_direct).
// One s_barrier per step; LDS ordering by lgkmcnt(0) only — a workgroup fence would add
// vmcnt(0) and make each wave wait for its own global stores.
//
// LDS per workgroup must stay <= 40 KB so that four workgroups (a 65 536-table grid) are resident
// per CU.  At 3-4 players the larger state and terminal hand-off would overflow that, so the deal
// scratch shrinks to the 100 bytes a deal uses (stride 25 dwords: odd, conflict-free byte lanes),
// 3 players list at most 8 terminal states per step, and at 4 players the scratch lives inside the
// rules wave's own state slot st[k & 1]: a deal (fused refill or inline autoreset deal) runs
// before that slot is written for step k, and the output wave finished reading it (step k - 2)
// before the hand-off barrier of step k - 1.
// partner hand-off (rollout store kernels): another wave of the team (the dealer, or the rules wave of
// the two-wave kernel) polls the pair's flag words so the output wave never waits on a global load
// behind its own row stores (one in-order vmcnt)
struct PtShared {
    uint32_t pepoch;  // output wave -> poller: this launch's counter
    uint32_t seq[2];  // output wave -> poller: tasks posted (pseq), partner tasks seen (cseq)
    uint64_t in[3];   // poller -> output wave: partner progress; pseq << 32 | my next slot's flag;
                      // cseq << 32 | the partner's next slot's flag
    uint64_t qcons[2];  // quad kernel: in[2] by the parity of the rules step that polled it (the output
                        // wave's step k reads the rules wave's step k - 1, published before the barrier
                        // the output wave has passed: guide row 3's barrier between poll and loads)
};

template <int P>
struct __align__(16) WsLDS : Consts {
    static constexpr int kW = SW_COUNT + 4 * P;  // state words per table
    static constexpr int kWaves = 2;             // rules + output
    PtShared pt;
    static constexpr int kTerm = P == 3 ? 7 : (P == 4 ? 15 : 16);  // terminal states listed per step (3p: 7, room for PtShared)
    static constexpr int kScrStride = P == 2 ? kScratchStride : 100;
    static constexpr bool kScrInSlot = P == 4;
    static_assert(!kScrInSlot || kW * 64 * 4 >= 64 * kScrStride, "scratch must fit the state slot");
    uint32_t st[2][kW][64];
    uint32_t tst[2][kTerm][kW];
    uint32_t small[2][64];  // the step's reward / terminated / flags / winner / episode event (pack_small)
    uint64_t mask[2][64];
    uint64_t fin[2];
    uint32_t mbits[96];
    uint8_t rows[64 * kObsDim];
    uint8_t scr[kScrInSlot ? 16 : 64 * kScrStride];  // the rules wave's deal scratch (P < 4)
    uint32_t mtx[kScrInSlot ? 624 : 0];               // deal continuation (LaneMT) at P = 4 (none below)
    __device__ __forceinline__ uint8_t *scratch(int b, int lane) {
        return kScrInSlot ? reinterpret_cast<uint8_t *>(&st[b][0][0]) + lane * kScrStride : &scr[lane * kScrStride];
    }
    // LDS for a deal's LaneMT continuation: this step's free state slot, unless it holds the scratch
    __device__ __forceinline__ uint32_t *deal_mtx(int b) { return kScrInSlot ? mtx : &st[b][0][0]; }
};
static_assert(sizeof(WsLDS<2>) <= 40960 && sizeof(WsLDS<3>) <= 40960 && sizeof(WsLDS<4>) <= 40960,
              "the two-wave rollout needs four workgroups per CU");

template <int P>
__device__ __forceinline__ uint32_t tab_word(const Tab<P> &T, int w) {
    return w < SW_COUNT ? T.sw[w] : T.pw[(w - SW_COUNT) >> 2][(w - SW_COUNT) & 3];
}
template <int P>
__device__ __forceinline__ void set_tab_word(Tab<P> &T, int w, uint32_t v) {
    if (w < SW_COUNT) T.sw[w] = v;
    else T.pw[(w - SW_COUNT) >> 2][(w - SW_COUNT) & 3] = v;
}

// The rules wave's per-step small outputs, packed for the hand-off: the OUTPUT wave issues every
// global write of a step.  A store the rules wave issued would sit in its vmcnt queue ahead of
// the next step's deck / token-table gathers (gfx9 counts loads and stores in one in-order
// counter), so each step's first use of a gathered value would wait for a write acknowledgement
// from behind the whole chip's observation stream: 12.8 -> 19.6 us per step once that stream
// goes to HBM instead of the Infinity Cache (rollout store, 65 536 tables).
// bits 0-7 flags, 8 terminated, 9 valid, 10-12 winner + 1, 13-15 reward code, 16-17 code of
// player 0's final reward (envs/splendor_env.py:92-115), 18 episode ended (ep_return / ep_count).
__device__ __forceinline__ uint32_t reward_code(float r) {
    return r == 0.0f ? 0u : (r == -0.01f ? 1u : (r == -0.1f ? 2u : (r == 1.0f ? 3u : 4u)));
}
__device__ __forceinline__ float reward_of_code(uint32_t c) {
    return c == 0u ? 0.0f : (c == 1u ? -0.01f : (c == 2u ? -0.1f : (c == 3u ? 1.0f : -1.0f)));
}
// player 0's final reward is one of 0, -1, -0.1, 1 (final_reward_p0)
__device__ __forceinline__ uint32_t ep_code(float r) { return r == 0.0f ? 0u : (r == -1.0f ? 1u : (r == -0.1f ? 2u : 3u)); }
__device__ __forceinline__ float ep_of_code(uint32_t c) {
    return c == 0u ? 0.0f : (c == 1u ? -1.0f : (c == 2u ? -0.1f : 1.0f));
}
__device__ __forceinline__ uint32_t pack_small(bool valid, const StepOut &o, int winner, bool ep, float ep_add) {
    return (o.flags & 0xFFu) | (o.term ? 1u << 8 : 0u) | (valid ? 1u << 9 : 0u) | ((uint32_t)(winner + 1) & 7u) << 10 |
           reward_code(o.reward) << 13 | ep_code(ep_add) << 16 | (ep ? 1u << 18 : 0u);
}

__device__ __forceinline__ void ws_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Bounded LDS waits (the dealer rollout's and the three-wave step's): a wait that runs out faults the
// launch — the serial goes to the context's host-mapped fault word — instead of spinning forever.
constexpr uint32_t kSpinLimit = 1u << 22;
__device__ uint32_t g_spin_limit = kSpinLimit;
__device__ __forceinline__ void signal_fault(const KStep &S) {
    if (S.fault && lane_id() == 0)  // a vector store (system scope: write-through to the host-mapped word)
        __hip_atomic_store(S.fault, S.fault_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace spl
