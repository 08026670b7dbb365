#pragma once
// spl_engine_step.h — one env step of one table, shared by step_ws and the rollouts: the early gathers
// (StepPre, step_prefetch), SplendorEnv.step on the table in registers (StepOut, step_rules), final_reward_p0, the
// autoreset through the pool (flip_to_pool, refill_table, autoreset_table, fresh_deal_mask) and store_final_rows;
// then the launch-side helpers gated_action, store_step_info and RefillSlots / refill_slots.
#include "../../include/splendor_amd.h"
#include "spl_engine_args.h"
#include "spl_engine_stamps.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_deal.h"
#include "spl_layout.h"

namespace spl {

// ---- one env step of one table, shared by step_ws and the rollouts ----------------------------

// Loads a step needs beyond the table state, issued as early as the action is known: the deck
// card the action pops and the token-return table entry it consults (predict_lut_key).
struct StepPre {
    uint32_t top;
    int key;
    uint4 e;
};

template <int P>
__device__ __forceinline__ StepPre step_prefetch(const Tab<P> &T, int action, bool valid, const KArena &A, int t,
                                                 const KTables &Tb) {
    StepPre pre{0xFFu, -1, make_uint4(0u, 0u, 0u, 0u)};
    const bool live_tab = valid && !is_terminal(T.sw);
    const int ptier = pop_tier(action);
    if (live_tab && ptier >= 0) {
        const int len = (int)bget(T.sw[SW_DECK], ptier);
        const uint8_t *live = live_rec(A, t, T.sw[SW_MISC]);
        SPL_CHECK(len <= tier_size(ptier), BC_DECK);
        if (len > 0) pre.top = abl(ABL_DECK_GATHER) ? (uint32_t)(len + 3 * ptier) : live[tier_base(ptier) + len - 1];
    }
    if (live_tab && action >= 0 && action < SPL_NUM_ACTIONS) {
        const int tp = get_to_play(T.sw);
        uint32_t pw4[4];
        get_player(T, tp, pw4);
        int bank[6];
        get_bank(T.sw, bank);
        pre.key = predict_lut_key(unpack_pl(pw4), bank, action, get_turn(T.sw), tp);
        SPL_CHECK(pre.key < kLutEntries, BC_LUT);
        if (pre.key >= 0) pre.e = abl(ABL_LUT_GATHER) ? make_uint4(0x12345678u, 0x9abcdef0u, 0x0fedcba9u, (uint32_t)pre.key) : Tb.lut[pre.key];
    }
    return pre;
}

constexpr uint64_t kMaskDeferred = 1ull << 63;  // step_rules(defer_mask): legal mask still to evaluate

struct StepOut {
    uint32_t flags;
    float reward;
    bool term;
    uint64_t mask;  // info["action_mask"] after the step (before any autoreset)
};

// envs/splendor_env.py:51-90 on the table in registers.  `known` (k_rollout after its first
// step): `known_mask` is legal_moves of the table's current state, computed by the previous step,
// so "any legal move?" and mask[action] need no re-evaluation.
template <int P, class Stamp = NoStamp>
__device__ __forceinline__ StepOut step_rules(Tab<P> &T, int action, const StepPre &pre, bool valid, const Consts &L,
                                              const KTables &Tb, uint32_t *mtx, bool known = false,
                                              uint64_t known_mask = 0ull, bool defer_mask = false,
                                              Stamp stamp = Stamp()) {
    StepOut o{0u, 0.0f, false, 0ull};
    bool want_mask = false;
    if (valid) {
        if (is_terminal(T.sw)) {                                  // :53-54 RuntimeError
            o.flags = SPL_F_AFTER_TERMINAL;
        } else {
            const bool in_range = action >= 0 && action < SPL_NUM_ACTIONS;
            uint32_t pw4[4];
            get_player(T, get_to_play(T.sw), pw4);
            const Pl cur = unpack_pl(pw4);
            int bank[6];
            get_bank(T.sw, bank);
            // :55 mask = legal_moves(state): only "any legal?" and mask[action] are needed here
            bool anyl, ok;
            if (known) {
                anyl = known_mask != 0ull;
                ok = in_range && ((known_mask >> (action & 63)) & 1ull);
            } else {
                anyl = abl(ABL_LEGAL_PRE) || any_legal(T.sw, cur, bank, L);
                ok = abl(ABL_LEGAL_PRE) || (in_range && action_legal(T.sw, cur, bank, action, L));
            }
            if (!anyl) {                                          // :56-61 no legal move: draw
                T.sw[SW_MISC] = (T.sw[SW_MISC] | ST_GAME_OVER) & 0x00FFFFFFu;
                T.sw[SW_BANK1] &= 0xFF00FFFFu;                    // to_play = 0
                o.term = true;
                o.flags = SPL_F_DRAW;
            } else if (!in_range) {                               // :62-63 ValueError, mask of the unchanged state
                o.flags = SPL_F_OOB;
                want_mask = true;
            } else if (!ok) {                                     // :64-66 illegal, mask of the unchanged state
                o.flags = SPL_F_ILLEGAL;
                o.reward = -0.01f;
                want_mask = true;
            } else {
                STAMP(2);
                stamp(4);
                if (!abl(ABL_APPLY)) apply_action(T, action, pre.top, L, Tb.lut, pre.key, pre.e, mtx, stamp);  // :68
                STAMP(3);
                stamp(5);
                o.term = is_terminal(T.sw);                       // :70
                if (o.term) {                                     // :71-80
                    const int w = get_winner(T.sw);
                    const bool tl = (T.sw[SW_MISC] & ST_TURN_LIMIT) != 0;
                    o.reward = (w < 0 && tl) ? -0.1f : (w < 0 ? 0.0f : (w == P - 1 ? 1.0f : -1.0f));
                    o.flags |= tl ? SPL_F_TURN_LIMIT : 0u;        // :82-83
                } else {
                    want_mask = true;                             // :81
                }
            }
        }
    }
    stamp(6);
    // one legal_moves evaluation per lane (a single call site keeps one copy in the code).
    // defer_mask: left to the caller (kMaskDeferred marks the lanes that need it; k_step_ws
    // evaluates it after handing the state to its output wave)
    if (defer_mask) o.mask = want_mask ? kMaskDeferred : 0ull;
    else if (want_mask) o.mask = abl(ABL_LEGAL_POST) ? (uint64_t)action : legal_of(T, L);
    return o;
}

// player 0's final reward of a finished episode (envs/splendor_env.py:92-115)
template <int P>
__device__ __forceinline__ float final_reward_p0(const Tab<P> &T) {
    const int w = get_winner(T.sw);
    const bool tl = (T.sw[SW_MISC] & ST_TURN_LIMIT) != 0;
    return w < 0 ? (tl ? -0.1f : 0.0f) : (w == 0 ? 1.0f : -1.0f);
}

// Reset to the next episode of the table's engine-seed stream (envs/splendor_env.py:43-44:
// reset() continues self.np_random): the live record moves to the next pool record, whose
// board / noble words `pool` holds.  With every pool record consumed since the last refill the
// next one is dealt inline — correct, only slower.  When the pool record after it is dealt, its
// words are gathered into `pool` for the next reset (the caller stores them to the pool
// planes); returns true in that case.
template <int P>
__device__ __forceinline__ bool flip_to_pool(Tab<P> &T, const KArena &A, int t, Deal &pool, uint8_t *scr,
                                             uint32_t *mtx, uint32_t &flags) {
    constexpr int kPools = kSlotRecords - 1;
    const uint32_t misc = T.sw[SW_MISC];
    const int a = active_of(misc), pend = pend_of(misc);
    const int nxt = (a + 1) % kSlotRecords;
    if (pend >= kPools) flags |= deal_next<P>(A, t, nxt, scr, pool, mtx);
    const int pend2 = pend >= kPools ? kPools : pend + 1;  // the old live record is free now
    fresh_state(T, ring_bits(nxt, pend2), pool);
    if (pend2 < kPools) pool = rec_deal(slot_rec(A, t, (nxt + 1) % kSlotRecords));
    return pend2 < kPools;
}

// One pool refill of table t (spl_refill's unit of work; status `misc` has pend > 0): re-deal the
// earliest consumed record in ring order (the next episode's deal comes first in the engine-seed
// stream).  When that record is the next pool, its words go to `pool` (`pool_dirty`).  Returns
// the new status word.
template <int P>
__device__ __forceinline__ uint32_t refill_table(const KArena &A, int t, uint32_t misc, uint8_t *scr, uint32_t *mtx,
                                                 Deal &pool, bool &pool_dirty) {
    const int pend = pend_of(misc);
    const int slot = (active_of(misc) + kSlotRecords - pend) % kSlotRecords;
    Deal d;
    deal_next<P>(A, t, slot, scr, d, mtx);
    if (pend == kSlotRecords - 1) {
        pool = d;
        pool_dirty = true;
    }
    return (misc & ~ST_PEND) | ((uint32_t)(pend - 1) << ST_PEND_SHIFT);
}

// same-step autoreset of a terminal table; `pool_dirty` is set when the pool planes changed
template <int P>
__device__ __forceinline__ void autoreset_table(Tab<P> &T, const KArena &A, int t, Deal &pool, uint8_t *scr,
                                                uint32_t *mtx, StepOut &o, bool &pool_dirty) {
    pool_dirty |= flip_to_pool<P>(T, A, t, pool, scr, mtx, o.flags);
    o.flags |= SPL_F_RESET;
    o.mask = kFreshDealMask;
}

// The step mask of a lane whose table was just re-dealt (o.flags carries SPL_F_RESET; autoreset_table and
// dealer_step left kFreshDealMask): under a card table with a free card, legal_moves of the dealt state.
// The branch on the table's flag is wave-uniform (a kernel argument); other contexts do no work here.
template <int P>
__device__ __forceinline__ void fresh_deal_mask(StepOut &o, const Tab<P> &T, const Consts &L, const KTables &Tb) {
    if (has_free_card(Tb) && (o.flags & SPL_F_RESET)) o.mask = legal_of(T, L);
}

// Terminal rows staged in L.frows (bits of `fin`) -> final_obs rows of this wave.
__device__ __forceinline__ void store_final_rows(const uint8_t *rows_lds, uint64_t fin, int32_t *final_obs, int t0) {
    while (fin) {
        const int r = __ffsll((unsigned long long)fin) - 1;
        fin &= fin - 1;
        int32_t *dst = final_obs + (size_t)(t0 + r) * kObsDim;
        for (int e = lane_id(); e < kObsDim; e += 64) dst[e] = (int32_t)rows_lds[r * kObsDim + e];
    }
}

// spl_step_args_t.gate_*: the dual step's opponent moves only where the agent's move was applied
// and left the game running (wrappers/dual_step_native.py:120-140, spl_dual_gate); elsewhere its
// action becomes -1 (out of range: no move), written back so the caller sees the gated action.
__device__ __forceinline__ int gated_action(const KStep &S, int t) {
    int action = S.actions[t];
    if (S.gate_terminated && (S.gate_terminated[t] != 0 || (S.gate_flags[t] & (SPL_F_ILLEGAL | SPL_F_OOB)) != 0)) {
        action = -1;
        const_cast<int32_t *>(S.actions)[t] = -1;
    }
    return action;
}

// spl_step's gymnasium info planes (illegal_action, draw, turn_limit as 0/1 bytes; truncated = 0) and the running
// count of tables whose flags carry the reference's exceptions (out-of-range action, step after
// termination): one atomic per wave that has any.  Wave-uniform call (the ballot).
__device__ __forceinline__ void store_step_info(const KStep &S, int n, int t, bool valid, uint32_t f) {
    if (S.info && valid) {
        S.info[t] = (f & SPL_F_ILLEGAL) ? 1 : 0;
        S.info[(size_t)n + t] = (f & SPL_F_DRAW) ? 1 : 0;
        S.info[2 * (size_t)n + t] = (f & SPL_F_TURN_LIMIT) ? 1 : 0;
        S.info[3 * (size_t)n + t] = 0;  // truncated
    }
    if (S.errors) {
        const uint64_t bad = __ballot(valid && (f & (SPL_F_OOB | SPL_F_AFTER_TERMINAL)) != 0);
        if (bad && lane_id() == __ffsll((unsigned long long)bad) - 1)
            atomicAdd(S.errors, (unsigned long long)__popcll(bad));
    }
}

// Fused pool refills of one rollout launch: `count` refills (one per refill period the launch
// crosses), one per segment of K / count steps, each workgroup at its own offset within the segment
// so that deals (VALU-bound) overlap other workgroups' stores.  Results do not depend on the slots.
struct RefillSlots {
    int seg, count, off;
    __device__ __forceinline__ bool due(int k) const { return count > 0 && k < seg * count && k % seg == off; }
};
// `key` staggers the refill step per workgroup (per team in the multi-team kernels); results do not
// depend on the schedule
__device__ __forceinline__ RefillSlots refill_slots(int K, int count, uint32_t key = blockIdx.x) {
    RefillSlots r{1, 0, 0};
    if (count > 0) {
        r.count = min(count, K);
        r.seg = K / r.count;
        r.off = (int)(((key * 0x9E3779B1u) >> 16) % (uint32_t)r.seg);
    }
    return r;
}

}  // namespace spl
