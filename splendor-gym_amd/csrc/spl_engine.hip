// spl_engine.hip — MI355X (gfx950) Splendor rollout engine: kernels + C-ABI.
//
// One wavefront lane = one table; a workgroup is ONE wave (64 tables) so small batches still
// spread over all 256 CUs.  State lives in HBM as 32-bit word planes (spl_layout.h) and is
// held in VGPRs for the whole step; branchy rules are predicated per lane (no MFMA: this is
// small-integer work).  Observations are staged in LDS as bytes (every value <= 255 except
// move_count, patched separately) and leave the CU as coalesced 16-byte int32x4 stores; masks
// leave as packed bytes built from per-lane 45-bit words in LDS.
//
// This file is the engine's one translation unit (a kernel is launched from the file that defines it).  Every layer
// without a kernel is a header, included in layer order, which is the order their definitions always had; a layer
// includes only layers below it (tests/test_engine_headers.py):
//   spl_engine_args.h      kernel argument blocks, build switches (SPL_ABL, SPL_CHECK), lane_id
//   spl_engine_stamps.h    the SPL_STAMPS diagnostics                                  (on args)
//   spl_engine_base.h      stream limit, defaults, wg_block, LDS blocks, small helpers
//   spl_engine_rules.h     the rules on a table in registers                           (on args, base)
//   spl_engine_obs.h       the observation encoder and the block stores                (on args, base, rules)
//   spl_engine_deal.h      the deal, PCG / pool / state I/O, legal_of, policy_action   (on args, base, rules)
//   spl_engine_step.h      one env step of one table, autoreset, refill slots          (on the four bottom layers, deal)
//   spl_engine_cols.h      the column-parallel final rows                              (on args, base)
//   spl_engine_ws.h        what the multi-wave kernels share, the bounded waits' parts (on args, base, rules, step)
//   spl_engine_handoff.h   delegation, the dealer wave, the partner hand-off           (on all above but stamps, cols)
//   spl_engine_succ.h      one-ply successors of every table, read-only               (on args, base, rules, obs, deal, step)
//   spl_engine_pairs.h     the successors of the legal pairs only, compacted           (on the succ layer and what it is on)
// What stays here needs the translation unit, in the order it always had: k_build_lut (between the deal and the step
// include), k_rollout, spl_step's kernels and kStepKernels (before the hand-off include: a kernel and a device
// variable keep their order in the host object), the split-wave rollouts and kRolloutKernels, the utility kernels,
// k_successors (behind its include: the kernels before it keep their order) and the pairs kernels (last, behind
// theirs, for the same reason); then the host side and the C ABI.
//
// Reference semantics restated here (paths relative to the reference root):
//   engine/rules.py:40-93 legal_moves, :101-122 _pay_for_card, :125-129 _refill_slot,
//   :132-147 _grant_noble_if_applicable, :150-193 auto_return_tokens/_enforce_token_limit,
//   :196-287 apply_action, :290-312 compute_winner/is_terminal; engine/state.py:61-71
//   can_afford, :181-211 initial_state; engine/encode.py:124-187 encode_observation;
//   envs/splendor_env.py:41-115 reset/step/get_final_rewards.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/splendor_amd.h"
#include "../../include/splendor_search.h"
#include "spl_common.h"
#include "spl_layout.h"
#include "spl_rng.h"
#include "spl_scripted.h"

#include "spl_engine_args.h"
#include "spl_engine_stamps.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_obs.h"
#include "spl_engine_deal.h"

namespace spl {

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

// Token-return table: for every (turn_count, to_play, sum(tokens), sum(bank)) in the domain,
// the top 3 bits of the first 40 outputs of random.Random(seed) (engine/rules.py:170-176).
__global__ __launch_bounds__(64) void k_build_lut(uint4 *lut) {
    const int e = blockIdx.x * 64 + lane_id();
    if (e >= kLutEntries) return;
    const int sb = e % kLutSb, st = 11 + (e / kLutSb) % kLutSt, tp = (e / (kLutSb * kLutSt)) % kLutTp,
              tc = e / (kLutSb * kLutSt * kLutTp);
    const uint64_t seed = ((uint64_t)tc * 1315423911ull) ^ ((uint64_t)tp * 2654435761ull) ^ ((uint64_t)st * 97531ull) ^
                          ((uint64_t)sb * 31337ull);
    MTStream ms;
    ms.init(seed);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int j = 0; j < kLutOutputs; ++j) {
        const uint32_t top = ms.next(j) >> 29;
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] |= (j / 10 == q) ? top << (3 * (j % 10)) : 0u;
    }
    lut[e] = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace spl

#include "spl_engine_step.h"
#include "spl_engine_cols.h"
#include "spl_engine_ws.h"

namespace spl {

// K consecutive env steps of every table with the device uniform-random policy: exactly K
// spl_step launches with next_actions fed back as the next launch's actions (plies ply ..
// ply+K-1), without the launch boundaries.  The table state stays in registers; each step's
// block stores are issued and left to drain while the wave computes the next step, and the
// next step's deck-card / token-table gathers are issued a whole step ahead.  Step k's outputs
// go to block k of each output array when `per_step` (rollout storage [K][n][...]), else every
// step overwrites block 0.
//
// refill != 0 (a pool refill is due in this launch): the refill is fused — each wave re-deals its
// tables' earliest consumed pool record (k_refill's work) at a step of its own, spread over the
// K steps.  The deal is a long serial integer chain per lane; inside the rollout it runs while
// this wave's stores drain and the other waves keep HBM busy, where a separate k_refill launch
// leaves HBM idle for its whole duration.  Trajectories do not depend on when a refill happens
// (deals are taken from each table's engine-seed stream in episode order either way).
template <int P>
__global__ __launch_bounds__(64) void k_rollout(KArena A, KTables Tb, KStep S, int K, int per_step, int refill) {
    __shared__ BlockLDS L;
    const RefillSlots rs = refill_slots(K, S.autoreset ? refill : 0);
    const int lane = lane_id();
    uint32_t *const deal_mtx = reinterpret_cast<uint32_t *>(&L.rows[64 * kScratchStride]);  // LaneMT continuation
    const int t0 = blockIdx.x * 64;
    const int t = t0 + lane;
    const bool valid = t < A.n;
    const int rows = min(64, A.n - t0);
    load_tables_lds(L, Tb);

    Tab<P> T;
    int action = 0;
    Deal pool = empty_deal();
    if (valid) {
        load_tab(T, A, t);
        action = S.actions[t];
        if (S.autoreset) pool = load_pool(A, t);
    } else {
        fresh_state(T, 0u, empty_deal());
    }
    StepPre pre = step_prefetch(T, action, valid, A, t, Tb);
    bool pool_dirty = false;
    const uint64_t ply0 = S.ply + (S.ply_base ? *S.ply_base : 0ull);
    const bool want_final = S.autoreset && S.final_obs != nullptr;
    // A wave may have 63 memory instructions in flight; a step's ~90 stores would stall it until
    // its own first stores drained.  So the obs block leaves in two parts: the first with the
    // step's other outputs, the rest after the NEXT step's rules (from the same LDS rows, before
    // anything overwrites them), and the wave computes while each part drains.
    int32_t *obs_tail = nullptr;  // second part of the previous step's obs block, not yet issued
    uint64_t cur_mask = 0ull;     // legal_moves of the current state, once a step has computed it
#ifdef SPL_STAMPS
    int rst_lo[kRStamps] = {0}, rst_hi[kRStamps] = {0};
#endif
    for (int k = 0; k < K; ++k) {
        const size_t blk = per_step ? (size_t)k * (size_t)A.n : 0;
        wave_lds_sync();  // previous step's LDS reads done (rows, mask, frows)
        RSTAMP(0, k);
        // token-return continuation (LaneMT) in frows: rows still hold the last step's obs tail
        StepOut o = step_rules(T, action, pre, valid, L, Tb, reinterpret_cast<uint32_t *>(L.frows), k > 0, cur_mask);
        RSTAMP(1, k);
        if (obs_tail) store_obs_range(L.rows, obs_tail, kObsSplit, kObsBlockWords);
        obs_tail = nullptr;
        if (rs.due(k)) {  // fused pool refill (wave-uniform)
            wave_lds_sync();  // the tail's LDS reads are done: the rows serve as deal scratch
            if (valid && pend_of(T.sw[SW_MISC]) > 0)
                T.sw[SW_MISC] = refill_table<P>(A, t, T.sw[SW_MISC], &L.rows[lane * kScratchStride], deal_mtx, pool,
                                                pool_dirty);
        }
        RSTAMP(2, k);
        const int8_t wnr = (int8_t)get_winner(T.sw);
        const uint64_t fin = __ballot(valid && o.term && want_final);
        if (__any(valid && o.term && want_final)) encode_row(T, L.frows, L);  // rows of other lanes are not stored
        const int fin_moves = get_moves(T.sw);
        if (valid && o.term) {  // per termination, as step_ws (same float rounding)
            if (S.ep_return) unsafeAtomicAdd(&S.ep_return[t], final_reward_p0(T));
            if (S.ep_count) atomicAdd(&S.ep_count[t], 1u);
        }
        if (valid && o.term && S.autoreset)
            autoreset_table(T, A, t, pool, &L.rows[lane * kScratchStride], deal_mtx, o, pool_dirty);
        fresh_deal_mask(o, T, L, Tb);
        wave_lds_sync();
        if (!abl(ABL_ENCODE)) encode_row(T, L.rows, L);
        L.mask[lane] = o.mask;
        wave_lds_sync();
        RSTAMP(3, k);
        // the policy's next action and its prefetches go out before this step's stores
        action = policy_action(S.policy, o.mask, T, L, S.policy_seed, (uint64_t)(S.table0 + t), ply0 + (uint64_t)k);
        cur_mask = o.mask;
        if (k + 1 < K) pre = step_prefetch(T, action, valid, A, t, Tb);
        int32_t *obs = S.obs + blk * kObsDim;
        const bool patch = valid && get_moves(T.sw) > 255;
        const bool fpatch = valid && o.term && want_final && fin_moves > 255;
        const bool split = rows == 64 && !__any(patch || fpatch);  // crafted states store at once
        if (abl(ABL_OBS_STORE)) {
        } else if (split) {
            store_obs_range(L.rows, obs + (size_t)t0 * kObsDim, 0, kObsSplit);
            obs_tail = obs + (size_t)t0 * kObsDim;
        } else {
            store_obs_block(L.rows, rows, obs + (size_t)t0 * kObsDim);
        }
        store_mask_block(L.mask, L.mbits, rows, S.mask + blk * 45 + (size_t)t0 * 45);
        int32_t *fobs = want_final ? S.final_obs + blk * kObsDim : nullptr;
        if (want_final) store_final_rows(L.frows, fin, fobs, t0);
        if (!split && __any(patch || fpatch)) {  // move_count > 255 (crafted states only) does not fit the byte staging: patched after the block stores
            __builtin_amdgcn_s_waitcnt(0);
            if (patch) obs[(size_t)t * kObsDim + 295] = get_moves(T.sw);
            if (fpatch) fobs[(size_t)t * kObsDim + 295] = fin_moves;
        }
        if (valid) {
            S.reward[blk + t] = o.reward;
            S.terminated[blk + t] = o.term ? 1 : 0;
            S.flags[blk + t] = (uint8_t)o.flags;
            if (S.winner) S.winner[blk + t] = wnr;
        }
        RSTAMP(4, k);
    }
    if (obs_tail) store_obs_range(L.rows, obs_tail, kObsSplit, kObsBlockWords);
#ifdef SPL_STAMPS
    if (g_rstamps) {
        RSTAMP(5, 0);  // kernel end for this wave (lane 0)
        if (lane < K && lane < 16)
            for (int i = 0; i < kRStamps; ++i)
                g_rstamps[((size_t)blockIdx.x * 16 + lane) * kRStamps + i] =
                    ((uint64_t)(uint32_t)rst_hi[i] << 32) | (uint32_t)rst_lo[i];
    }
#endif
    if (valid) {
        if (S.next_actions) S.next_actions[t] = action;
        store_tab(T, A, t, cur_mask, K > 0 ? Tb.mtag : 0u);  // cur_mask: the last step's mask of this state
        if (pool_dirty) store_pool(A, t, pool);
    }
}

// SplendorEnv.step for every table with the rules / output split of the two-wave rollout, for ONE step:
// 128-thread workgroups of 64 tables.  The RULES wave loads, steps and autoresets its tables and
// hands the new state words (and the pre-reset words of tables that just ended) to the OUTPUT
// wave through LDS; the output wave encodes and stores the observation rows (terminal rows first)
// while the rules wave evaluates the legal mask of the new state (engine legal_moves,
// envs/splendor_env.py:81) and stores the masks, small outputs, next action and state.  The
// output wave also stages the constant tables while the rules wave's state loads
// are in flight.  (Terminal rows written per lane by the rules wave instead: 27.5 -> 29.0 us.)
// The TAIL wave (round 6; k_step_wst_<P>p): a third wave per 64 tables takes the legal mask of the new
// state (engine legal_moves, envs/splendor_env.py:81), the mask block, the fused policy's next action
// and the legal-mask cache entry off the rules wave's tail; hand-off 2 (rules -> output: row halves
// staged) becomes an LDS counter, so the tail wave never waits on the other two after hand-off 1.
// Without it (k_step_ws_<P>p, round 5's two waves) the rules wave evaluates the mask after hand-off 2.
// Same outputs either way.  Measured alternating on one box (profiles/r06/stepab_r06g_h.txt, graph
// events per step): 16 384 tables 17.4 -> 14.7 us with the tail wave; 65 536 tables 22.4 -> 22.9 us
// (four workgroups per CU: 12 waves share the SIMDs and the LDS) — so spl_step picks it by grid size
// (spl_ctx_set_step_tail: auto = at most ctx->step_tail_blocks workgroups).  Row store policy: kStepRowCpol.

template <int P>
struct __align__(16) StepWsLDS : Consts {
    static constexpr int kW = SW_COUNT + 4 * P;  // state words per table
    uint32_t st[kW][64];   // state after the step (and autoreset)
    uint32_t fst[kW][64];  // pre-reset state of the tables that ended (final_observation)
    uint64_t mask[64];
    uint64_t omask[64];    // rules -> tail wave: each lane's step mask (kMaskDeferred: legal_moves to evaluate)
    uint32_t halves;       // rules -> output wave: row halves staged (hand-off 2 with the tail wave)
    uint32_t mbits[96];
    // observation staging (rows of 297 bytes, or 300 for obs_u8); before hand-off 1 the rules wave's
    // deal scratch + LaneMT
    alignas(16) uint8_t rows[64 * kObsU8];
};
static_assert(sizeof(StepWsLDS<4>) <= 40960, "k_step_ws_* needs four workgroups per CU");

// hand-off 2 of the three-wave step (rules -> output wave) as an LDS counter: a bounded wait (a lost
// hand-off faults the launch loudly, as the dealer rollout's waits do, instead of spinning)
__device__ __forceinline__ void step_publish(uint32_t *p) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's row halves have landed in LDS
    if (lane_id() == 0) __hip_atomic_store(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ bool step_wait(const uint32_t *p) {
    const uint32_t limit = g_spin_limit;
    for (uint32_t spins = 0;; ++spins) {
        const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // later LDS reads stay below the poll
        if (v) return true;
        if (spins >= limit) {
            SPL_CHECK(false, BC_SPIN);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// The tail of a step, by whichever wave of step_ws takes the new state's legal mask.
// A lane's step mask with the deferred evaluation done (kMaskDeferred: engine legal_moves of the new state;
// reset tables carry the fresh deal's, terminal ones none).  `ablated`: what an ABL_LEGAL_POST build takes instead.
template <int P>
__device__ __forceinline__ uint64_t resolved_mask(uint64_t m, const Tab<P> &T, const Consts &L, uint64_t ablated = 0ull) {
    if (m & kMaskDeferred) m = abl(ABL_LEGAL_POST) ? ablated : legal_of(T, L);
    return m;
}
// the wave's mask block, plain stores (kStepRowCpol's comment)
template <int P>
__device__ __forceinline__ void store_step_mask(StepWsLDS<P> &L, const KStep &S, uint64_t m, int t0, int rows) {
    L.mask[lane_id()] = m;
    wave_lds_sync();
    if (!abl(ABL_MASK_STORE)) store_mask_block<false>(L.mask, L.mbits, rows, S.mask + (size_t)t0 * 45);
}
// the fused policy's action on the stored state
template <int P>
__device__ __forceinline__ void store_next_action(const KStep &S, const Consts &L, const Tab<P> &T, uint64_t m, int t) {
    if (S.next_actions) {
        const uint64_t ply = S.ply + (S.ply_base ? *S.ply_base : 0ull);
        S.next_actions[t] = policy_action(S.policy, m, T, L, S.policy_seed, (uint64_t)(S.table0 + t), ply);
    }
}
// Publish m as the legal mask of the state the rules wave stores (tail and output wave): the mask block, the
// next action and the legal-mask cache entry.  The rules wave (kShape 0) ends in store_tab instead, after its
// small outputs.
template <int P>
__device__ __forceinline__ void publish_mask(StepWsLDS<P> &L, const KArena &A, const KTables &Tb, const KStep &S,
                                             const Tab<P> &T, uint64_t m, int t0, int rows, bool valid) {
    const int t = t0 + lane_id();
    store_step_mask(L, S, m, t0, rows);
    if (valid) {
        store_next_action(S, L, T, m, t);
        store_legal(A, t, m, Tb.mtag);
    }
}

// kShape: 0 two waves (the rules wave takes the new state's mask), 1 three waves (the TAIL wave takes
// it), 2 two waves with the OUTPUT wave taking it in the middle of its row-block stores (k_step_wso)
template <int P, int kShape>
__device__ __forceinline__ void step_ws(StepWsLDS<P> &L, KArena A, KTables Tb, KStep S) {
    constexpr bool kStepTail = kShape == 1, kOMask = kShape == 2, kRulesMask = kShape == 0;
    constexpr int kW = StepWsLDS<P>::kW;
    const int lane = lane_id();
    const int role = (int)(threadIdx.x >> 6);  // 0 rules, 1 output, 2 tail (kStepTail)
    const bool rules_wave = role == 0;
    const int t0 = wg_block() * 64;
    const int t = t0 + lane;
    const bool valid = t < A.n;
    const int rows = min(64, A.n - t0);
    const bool want_final = S.autoreset && S.final_obs != nullptr;
    const bool compact = S.obs_u8 != nullptr && S.obs == nullptr;  // obs_u8 rows instead of int32 obs rows
    STAMP(0);
    if (kStepTail && rules_wave && lane == 0) L.halves = 0u;  // read only after hand-off 1
    if (rules_wave) {
        __builtin_amdgcn_s_setprio(1);  // as in the rollout: 27.9 -> 27.3 us
        Tab<P> T;
        int action = 0;
        Deal pool = empty_deal();
        // the constant tables by LDS-DMA first: they land while the state loads are in flight, and the
        // vmcnt(0) below (which the state needs anyway) covers them — no staging wave, no hand-off 0
        // (a barrier that the stamps put at 2.8 us, ~0.7 us after the state had landed)
        dma_tables_lds(L, Tb);
        LegalCache lc{0u, 0u};
        if (valid) {
            load_tab(T, A, t);
            lc = load_legal(A, t);  // legal_moves of this state, stored by the kernel that stored the state
            action = gated_action(S, t);
            if (S.autoreset) pool = load_pool(A, t);
        } else {
            fresh_state(T, 0u, empty_deal());
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): state, action, pool and the tables' DMA have landed
        const StepPre pre = step_prefetch(T, action, valid, A, t, Tb);
        STAMP(1);
        uint32_t *const mtx = reinterpret_cast<uint32_t *>(&L.rows[64 * kScratchStride]);
        // the pre-step check (envs/splendor_env.py:55-66: any legal move? is the action legal?) from the
        // cached mask where it is this context's; tables whose cache is unknown (after an upload, or under
        // another card table) evaluate legal_moves as before
        StepOut o = step_rules(T, action, pre, valid, L, Tb, mtx, valid && lc.known(Tb.mtag), lc.mask(), true);
        // autoreset 2: a table terminal on entry is re-dealt without a move (dual-step opponent phase)
        const bool entry_reset = valid && S.autoreset == 2 && (o.flags & SPL_F_AFTER_TERMINAL);
        if (entry_reset) o.flags = 0u;
        const bool ended = valid && (o.term || entry_reset);
        const int8_t wnr = (int8_t)get_winner(T.sw);
        STAMP(2);
        const bool fin_me = ended && want_final;
        if (fin_me) {
#pragma unroll
            for (int w = 0; w < kW; ++w) L.fst[w][lane] = tab_word(T, w);
        }
        // terminal rows: stored by this wave after hand-off 2, column-parallel (store_row_columns)
        const uint64_t fin_all = __ballot(fin_me);
        const float ep_add = (valid && o.term) ? final_reward_p0(T) : 0.0f;
        bool pool_dirty = false;
        if (ended && S.autoreset)
            autoreset_table(T, A, t, pool, &L.rows[lane * kScratchStride], mtx, o, pool_dirty);
#pragma unroll
        for (int w = 0; w < kW; ++w) L.st[w][lane] = tab_word(T, w);
        // a free card in the table (wave-uniform): the re-dealt lanes' masks are legal_moves of the dealt
        // state, evaluated with the other lanes' deferred ones by whichever wave takes the masks
        const bool redealt = has_free_card(Tb) && (o.flags & SPL_F_RESET) != 0u;
        if (!kRulesMask) L.omask[lane] = redealt ? kMaskDeferred : o.mask;  // the tail / output wave evaluates the deferred lanes' masks
        STAMP(3);
        ws_sync();  // hand-off 1: state words (deal scratch in `rows` free again)
        // this wave encodes the first half of every row while the output wave encodes the second
        // (encode 2.7 -> ~1.4 us before the obs stores start)
        if (abl(ABL_ENCODE)) {
        } else if (compact) encode_row_u8<0>(T, L.rows, L);
        else encode_row_half<0>(T, L.rows, L);
        if (kStepTail) step_publish(&L.halves);  // hand-off 2 (the tail wave takes no part)
        else ws_sync();                          // hand-off 2: first row halves staged
        STAMP(4);
        if (fin_all && !abl(ABL_FINAL)) {  // info["final_observation"] rows: each by the whole wave, from its listed words
            // (four rows at a time, their LDS lookups overlapped, measured slower: 23.4 vs 23.2 us per step
            // at 65 536 tables, 19.5 vs 18.1 at 16 384; profiles/r05/fin_group_ab_r05zz4.txt)
            const ColRecipes crc = col_recipes();
            for (uint64_t m = fin_all; m; m &= m - 1) {
                const int r = __ffsll((unsigned long long)m) - 1;
                store_row_columns<P>(&L.fst[0][r], 64, L, crc, S.final_obs + (size_t)(t0 + r) * kObsDim);
            }
        }
        STAMP(7);
        STAMPV(9, __popcll(fin_all) | (__popcll(__ballot((o.mask & kMaskDeferred) != 0)) << 8));
        if (kRulesMask) {
            o.mask = resolved_mask(redealt ? kMaskDeferred : o.mask, T, L, (uint64_t)action);
            STAMP(5);
            // masks and small outputs leave from this wave while the output wave streams the rows
            store_step_mask(L, S, o.mask, t0, rows);
        }
        STAMP(8);
        store_step_info(S, A.n, t, valid, o.flags);
        if (valid) {
            S.reward[t] = o.reward;
            S.terminated[t] = o.term ? 1 : 0;
            S.flags[t] = (uint8_t)o.flags;
            if (S.winner) S.winner[t] = wnr;
            if (o.term) {
                if (S.ep_return) unsafeAtomicAdd(&S.ep_return[t], ep_add);
                if (S.ep_count) atomicAdd(&S.ep_count[t], 1u);
            }
            if (!kRulesMask) {
                store_words(T, A, t);  // the legal-mask cache entry is the tail / output wave's
            } else {
                store_next_action(S, L, T, o.mask, t);
                store_tab(T, A, t, o.mask, Tb.mtag);  // o.mask: legal_moves of the stored (stepped, autoreset) state
            }
            if (pool_dirty) store_pool(A, t, pool);
        }
        STAMP(6);
    } else if (role == 1) {
        STAMP(1);
        STAMP(2);
        ws_sync();  // hand-off 1 (the rules wave's table DMA landed before it)
        STAMP(3);
        Tab<P> T;
#pragma unroll
        for (int w = 0; w < kW; ++w) set_tab_word(T, w, L.st[w][lane]);
        if (abl(ABL_ENCODE)) {
        } else if (compact) encode_row_u8<1>(T, L.rows, L);
        else encode_row_half<1>(T, L.rows, L);
        if (kStepTail) {
            if (!step_wait(&L.halves)) signal_fault(S);  // hand-off 2 lost: the launch says so (rows stale)
        } else {
            ws_sync();  // hand-off 2
        }
        STAMP(4);
        STAMP(5);
        uint64_t m = 0ull;  // kOMask: the new state's legal mask, evaluated between the row stores
        auto mask_now = [&]() { m = resolved_mask(L.omask[lane], T, L); };
        if (compact) {
            store_obs_u8_block(L.rows, rows, S.obs_u8 + (size_t)t0 * kObsU8);
            if (kOMask) mask_now();
        } else {
            if (abl(ABL_OBS_STORE)) {
                if (kOMask) mask_now();
            } else if (kOMask) {
                store_obs_block_mid(L.rows, rows, S.obs + (size_t)t0 * kObsDim, mask_now);
            } else {
                store_obs_block<64, false, kStepRowCpol>(L.rows, rows, S.obs + (size_t)t0 * kObsDim);
            }
            if (S.obs_u8)  // both outputs: the compact copy of the same rows (a fused actor's input)
                store_u8_from_rows(L.rows, rows, S.obs_u8 + (size_t)t0 * kObsU8, valid ? (uint32_t)get_moves(T.sw) >> 8 : 0u);
        }
        STAMP(6);
        if (kOMask) publish_mask(L, A, Tb, S, T, m, t0, rows, valid);
        if (!compact && __any(valid && get_moves(T.sw) > 255)) {  // patch after this wave's block stores of the same dwords
            __builtin_amdgcn_s_waitcnt(0);
            if (valid && get_moves(T.sw) > 255) S.obs[(size_t)t * kObsDim + 295] = get_moves(T.sw);
        }
        STAMP(7);
    } else if (kStepTail) {
        // the TAIL wave: from hand-off 1 on, the new state's legal mask and everything that hangs on it
        ws_sync();  // hand-off 1
        Tab<P> T;
#pragma unroll
        for (int w = 0; w < kW; ++w) set_tab_word(T, w, L.st[w][lane]);
        publish_mask(L, A, Tb, S, T, resolved_mask(L.omask[lane], T, L), t0, rows, valid);
    }
}

// spl_step's kernels, one line each: X(name, players, shape), in the order of kStepKernels ([shape][players - 2]).
// One kernel name per player count and shape (see SPL_ROLLOUT_KERNELS).
#define SPL_STEP_KERNELS(X) \
    X(k_step_ws_2p, 2, 0)   \
    X(k_step_ws_3p, 3, 0)   \
    X(k_step_ws_4p, 4, 0)   \
    X(k_step_wst_2p, 2, 1)  \
    X(k_step_wst_3p, 3, 1)  \
    X(k_step_wst_4p, 4, 1)  \
    X(k_step_wso_2p, 2, 2)  \
    X(k_step_wso_3p, 3, 2)  \
    X(k_step_wso_4p, 4, 2)
#define SPL_STEP_THREADS(SHAPE_) (SHAPE_ == 1 ? 192 : 128)
#define X(NAME, P_, SHAPE_)                                                                           \
    __global__ __launch_bounds__(SPL_STEP_THREADS(SHAPE_)) void NAME(KArena A, KTables Tb, KStep S) { \
        __shared__ StepWsLDS<P_> L;                                                                   \
        step_ws<P_, SHAPE_>(L, A, Tb, S);                                                             \
    }
SPL_STEP_KERNELS(X)
#undef X
struct StepKernel {
    void (*fn)(KArena, KTables, KStep);
    int threads;  // per workgroup of 64 tables
};
#define X(NAME, P_, SHAPE_) {NAME, SPL_STEP_THREADS(SHAPE_)},
static const StepKernel kStepKernels[3 * 3] = {SPL_STEP_KERNELS(X)};
#undef X
#undef SPL_STEP_THREADS

}  // namespace spl

#include "spl_engine_handoff.h"

namespace spl {

// TPW = tables per workgroup: 64, or 32 for grids too small to give every SIMD a wave (e.g. the
// 32 768-table share of a 4-player 8-GPU run): twice the workgroups, lanes 32-63 idle.  The rules
// work is latency-bound at one wave per SIMD, so half-populated waves on every SIMD finish a step
// in about the time full ones take on half of them.
// kStore: per-step outputs (a [K][n][...] rollout store) or every step into the same [n][...] block;
// a template argument so that the two variants are separate kernels in a profile.
// kDealer: a third wave deals the pool refills (DealerLDS above; 64 tables per workgroup).
// kTeams: 64-table teams per workgroup (the six-wave dealer 2, the quad kernel 4; one workgroup per CU)
// Which of the two cross-XCC hand-offs a shape can use follows from these; the code of each is compiled
// into those kernels only.
template <int P_, int TPW_, bool kStore_, bool kDealer_, int kTeams_>
struct WsShape {
    static_assert(TPW_ == 64 || TPW_ == 32, "64 or 32 tables per workgroup");
    static_assert(!kDealer_ || TPW_ == 64, "the dealer variant runs 64 tables per workgroup");
    static constexpr int P = P_, TPW = TPW_, kTeams = kTeams_;
    static constexpr bool kStore = kStore_, kDealer = kDealer_;
    // rollout-store delegation (Deleg): the full two-wave store kernel
    static constexpr bool kDeleg = TPW == 64 && kStore && !kDealer && kTeams == 1;
    // partner hand-off (PartnerLink; per-step outputs, 64 tables per team): the multi-team kernels only —
    // one workgroup per CU, the guide's first measured row (the six-wave dealer and, round 5, the quad
    // kernel; not the two-wave kernel at four workgroups per CU)
    static constexpr bool kPartner = kStore && kTeams > 1;
};
// A wave's role in rollout_ws (0 rules, 1 output, 2 dealer) and the block of TPW tables it serves, as a
// multi-team kernel assigns them (team_assign); a one-team kernel takes both from the thread index and
// the workgroup (one block per workgroup).
struct WaveRole {
    int role, block;
};
// What a wave of rollout_ws knows about itself, settled once before the roles split.
struct WsWave {
    int lane, role;   // role: 0 rules, 1 output, 2 dealer
    int t0, t;        // the team's first table, this lane's table
    bool valid;       // the lane has a table
    int rows;         // the team's tables (TPW, fewer in the grid's last block)
    int sid;          // the team's number in the grid (its 64-table block in a multi-team kernel, else the
                      // workgroup): stamp slot of the diagnostic builds, stagger of the fused refills
    bool want_final;  // terminal rows are wanted (info["final_observation"])
    bool multi;       // a multi-team kernel: role and block came with a WaveRole
};

// The rules wave lists its terminal states of a step, before the autoreset replaces them, for the output
// wave: the first kTerm in L.tst[b], in lane order; any further row it stores itself (`row`: the table's
// row index in final_obs).  Returns the lanes listed (L.fin[b], once the step is handed off).
template <int P, class LdsT>
__device__ __forceinline__ uint64_t list_terminal(const Tab<P> &T, LdsT &L, int b, bool fin_me, int32_t *final_obs,
                                                  size_t row) {
    const int idx = __popcll(__ballot(fin_me) & ((1ull << lane_id()) - 1ull));
    if (fin_me) {
        if (idx < WsLDS<P>::kTerm) {
#pragma unroll
            for (int w = 0; w < WsLDS<P>::kW; ++w) L.tst[b][idx][w] = tab_word(T, w);
        } else {
            store_row_direct(T, L, final_obs + row * kObsDim);
        }
    }
    return __ballot(fin_me && idx < WsLDS<P>::kTerm);
}
// The output wave stores a lane's small outputs of a step as the rules wave packed them (pack_small),
// at index i = blk + t, and the episode statistics of table t.
__device__ __forceinline__ void store_small(uint32_t sm, const KStep &S, size_t i, int t) {
    if (!(sm & (1u << 9))) return;  // no table in this lane
    if (!abl(ABL_SMALL_OUT)) {
        S.reward[i] = reward_of_code((sm >> 13) & 7u);
        S.terminated[i] = (uint8_t)((sm >> 8) & 1u);
        S.flags[i] = (uint8_t)(sm & 0xFFu);
        if (S.winner) S.winner[i] = (int8_t)((int)((sm >> 10) & 7u) - 1);
    }
    if (sm & (1u << 18)) {  // same per-table order and float rounding as step_ws
        if (S.ep_return) unsafeAtomicAdd(&S.ep_return[t], ep_of_code((sm >> 16) & 3u));
        if (S.ep_count) atomicAdd(&S.ep_count[t], 1u);
    }
}
// A faulted workgroup's steps k.. are not stored: their flags say so (the blocks keep stale rows)
template <bool per_step>
__device__ __forceinline__ void mark_unstored(const KStep &S, int k, int K, int n, int t, bool valid) {
    for (int j = per_step ? k : 0; j < K && (per_step || j == 0); ++j)
        if (valid) S.flags[(per_step ? (size_t)j * (size_t)n : 0) + t] = (uint8_t)SPL_F_FAULT;
}

// The rules wave of a team: K steps of its tables, each handed to the output wave in buffers k & 1.
// Barrier invariant: without a dealer wave the two waves of a team hand off through
// ws_sync(), an s_barrier of the WHOLE workgroup — in the quad kernel (kTeams = 4) all eight waves pass
// each barrier together.  That is correct only because every wave makes exactly 1 + K ws_sync() calls
// (one in rollout_ws before the roles split, one per step of the loop below and of output_wave's) and
// none returns early: a per-team early exit or an extra barrier would deadlock the workgroup or pair
// different steps.  Only the dealer variants leave early (their fault path), and they hand off through
// LDS counters, not barriers.  The bounds-check build counts each wave's barriers and flags BC_BARRIER
// when a wave ends with another count.
template <class Sh, class LdsT>
__device__ __forceinline__ void rules_wave(LdsT &L, const KArena &A, const KTables &Tb, const KStep &S, int K, int refill,
                                           const WsWave &w, const PartnerLink &pl) {
    constexpr int P = Sh::P;
    constexpr bool per_step = Sh::kStore, kDealer = Sh::kDealer;
    constexpr int kW = WsLDS<P>::kW;
    const int lane = w.lane, t = w.t;
    const bool valid = w.valid;
    WsStamps st;
    st.start();
    const RefillSlots rs = refill_slots(K, (S.autoreset && !kDealer) ? refill : 0, (uint32_t)w.sid);
    // dealer bookkeeping (per lane): slots whose deal is in flight (valid while a batch is
    // outstanding) and whether `pool` still lacks the next record's words
    uint32_t my_req = 0, infl = 0;
    bool pool_stale = false;
    bool faulted = false;  // a dealer hand-off ran out (wave-uniform): stop, store nothing more
    Tab<P> T;
    int action = 0;
    Deal pool = empty_deal();
    if (valid) {
        load_tab(T, A, t);
        action = S.actions[t];
        if (S.autoreset) pool = load_pool(A, t);
    } else {
        fresh_state(T, 0u, empty_deal());
    }
    StepPre pre = step_prefetch(T, action, valid, A, t, Tb);
    bool pool_dirty = false;
    const uint64_t ply0 = S.ply + (S.ply_base ? *S.ply_base : 0ull);
    uint64_t cur_mask = 0ull;
    PtPolled polled{0u, 0u, 0u, 0u, 0u};  // quad kernel's partner poller (loaded a step ahead)
    int nsync = 0;  // ws_sync() calls in the steps (the barrier invariant above)
    for (int k = 0; k < K; ++k) {
        const int b = k & 1;
        const size_t blk = per_step ? (size_t)k * (size_t)A.n : 0;
        st.at(0, k);
        if constexpr (kDealer) {
            if (k >= 2 && !lds_wait_ge(L.dl, &L.dl.odone, (uint32_t)(k - 1))) {  // slot b: step k-2 is stored
                faulted = true;
                break;
            }
        }
        // token-return continuation (LaneMT) in this step's free state slot
        StepOut o = step_rules(T, action, pre, valid, L, Tb, &L.st[b][0][0], k > 0, cur_mask, false, st.sub(k));
        st.at(1, k);
        if (rs.due(k) && valid && pend_of(T.sw[SW_MISC]) > 0)  // fused pool refill
            T.sw[SW_MISC] = refill_table<P>(A, t, T.sw[SW_MISC], L.scratch(b, lane), L.deal_mtx(b), pool, pool_dirty);
        const int8_t wnr = (int8_t)get_winner(T.sw);
        const uint64_t fin_listed = list_terminal(T, L, b, valid && o.term && w.want_final, S.final_obs, blk + (size_t)t);
        const float ep_add = (valid && o.term) ? final_reward_p0(T) : 0.0f;  // per termination, as step_ws
        if constexpr (kDealer) {
            if (!dealer_step<P>(L.dl, T, A, t, valid, valid && o.term && S.autoreset, S.autoreset != 0, pool,
                                pool_dirty, my_req, infl, pool_stale, o)) {
                faulted = true;
                break;
            }
        } else {
            if (valid && o.term && S.autoreset)
                autoreset_table(T, A, t, pool, L.scratch(b, lane), L.deal_mtx(b), o, pool_dirty);
        }
        fresh_deal_mask(o, T, L, Tb);
        st.at(7, k);
        L.small[b][lane] = pack_small(valid, o, wnr, valid && o.term, ep_add);  // stored by the output wave
        if (kDealer && S.policy == SPL_POLICY_UNIFORM && k >= 2) {
            // the Philox word was drawn by the output wave at step k - 2 (it published odone >= k - 1
            // after writing it, which this step waited for): only the scaling stays on this chain
            if constexpr (kDealer) action = sample_uniform_word(o.mask, L.dl.rnd[b][lane]);
        } else {
            action = policy_action(S.policy, o.mask, T, L, S.policy_seed, (uint64_t)(S.table0 + t), ply0 + (uint64_t)k);
        }
        cur_mask = o.mask;
        if (k + 1 < K) pre = step_prefetch(T, action, valid, A, t, Tb);
#pragma unroll
        for (int i = 0; i < kW; ++i) L.st[b][i][lane] = tab_word(T, i);
        L.mask[b][lane] = o.mask;
        if (lane == 0) L.fin[b] = fin_listed;
        st.at(2, k);
        if constexpr (kDealer) {
            lds_publish(&L.dl.rdone, (uint32_t)(k + 1));  // hand-off of step k
        } else {
            if constexpr (Sh::kPartner) {
                if (pl.on) pt_poll_ahead(L.pt, pl, polled, k);
            }
            ws_sync();  // hand-off of step k
            ++nsync;
        }
        st.at(3, k);
    }
    if constexpr (kDealer) {  // no more batches; the last one lands before the state is stored
        lds_publish(&L.dl.stop, 1u);
        if (!faulted && !lds_wait_ge(L.dl, &L.dl.ddone, my_req)) faulted = true;
        if (pool_stale && !faulted) {
            pool = deal_of_lds(L.dl, lane);
            pool_dirty = true;
        }
        if (faulted) {  // the tables' state is not stored: the host sees the fault and resets
            signal_fault(S);
            return;
        }
    }
    st.flush_clocks(w.sid);
    st.flush(w.sid, 0, K);
    SPL_CHECK(kDealer || nsync == K, BC_BARRIER);
    (void)nsync;
    if (valid) {
        if (S.next_actions) S.next_actions[t] = action;
        store_tab(T, A, t, cur_mask, K > 0 ? Tb.mtag : 0u);  // cur_mask: the last step's mask of this state
        if (pool_dirty) store_pool(A, t, pool);
    }
}

// The output wave of a team: every global write of a step (why: the comment at pack_small), from the
// buffers the rules wave handed off.  `extra`: the delegation period (read by the Sh::kDeleg kernels only).
template <class Sh, class LdsT>
__device__ __forceinline__ void output_wave(LdsT &L, const KArena &A, const KStep &S, int K, int extra, const WsWave &w,
                                            const PartnerLink &pl) {
    constexpr int P = Sh::P, TPW = Sh::TPW;
    constexpr bool per_step = Sh::kStore, kDealer = Sh::kDealer, kDeleg = Sh::kDeleg, kPartner = Sh::kPartner;
    constexpr int kW = WsLDS<P>::kW;
    const int lane = w.lane, t = w.t, t0 = w.t0;
    const bool valid = w.valid;
    const ColRecipes crc = col_recipes();  // this lane's bytes of a column-parallel terminal row
    const uint64_t ply0 = S.ply + (S.ply_base ? *S.ply_base : 0ull);  // the policy words drawn ahead (dealer)
    (void)ply0;
    WsStamps st;
    Deleg dl{};
    if constexpr (kDeleg) dl = deleg_open(A, extra);
    PtOut po{0u, 0u, -1, 0, 0u};
    int osync = 0;  // ws_sync() calls in the steps (the barrier invariant at rules_wave)
    for (int k = 0; k < K; ++k) {
        if constexpr (kPartner) {
            if (pl.on) pt_step_top<P, kDealer>(pl, po, L.pt, k, L.rows, L, S.obs, A.n);
        }
        if constexpr (kDealer) {
            if (!lds_wait_ge(L.dl, &L.dl.rdone, (uint32_t)(k + 1))) {  // hand-off of step k
                mark_unstored<per_step>(S, k, K, A.n, t, valid);
                // steps before k that were handed to the partner: DONE, and those it has not taken are
                // stored here (they were stepped before the fault)
                if constexpr (kPartner) {
                    if (pl.on) pt_close<P>(pl, po, L.rows, L, S.obs, A.n, t0);
                }
                signal_fault(S);
                return;
            }
        } else {
            ws_sync();  // hand-off of step k
            ++osync;
        }
        st.at(0, k);
        const int b = k & 1;
        const size_t blk = per_step ? (size_t)k * (size_t)A.n : 0;
        Tab<P> T;
#pragma unroll
        for (int i = 0; i < kW; ++i) set_tab_word(T, i, L.st[b][i][lane]);
        // terminal rows (info["final_observation"]) first: each by the whole wave, column-parallel,
        // straight from its listed state words (no staging, no LDS barrier)
        // (readfirstlane returns int: widen through uint32_t, or bit 31 sign-extends into lanes 32-63)
        uint64_t fin = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)L.fin[b]) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(L.fin[b] >> 32)) << 32);
        if (fin) {
            int32_t *fobs = S.final_obs + blk * kObsDim;
            for (int idx = 0; fin; fin &= fin - 1, ++idx) {
                const int r = __ffsll((unsigned long long)fin) - 1;
                store_row_columns<P>(&L.tst[b][idx][0], 1, L, crc, fobs + (size_t)(t0 + r) * kObsDim);
            }
        }
        const bool big_moves = __any(valid && get_moves(T.sw) > 255);
        bool deleg_now = false;  // a delegated step: the rows are encoded by the partner workgroup
        if constexpr (kDeleg) deleg_now = dl.producer && deleg_step(k, K, dl.every);
        bool handed = false;  // partner hand-off of this step's rows
        if constexpr (kPartner) {
            if (pl.on && !big_moves) handed = pt_hand_off(pl, po, L.pt, T, k);
        }
        if (!handed && (!deleg_now || big_moves)) {
            encode_row(T, L.rows, L);
            wave_lds_sync();
        }
        st.at(1, k);
        int32_t *obs = S.obs + blk * kObsDim;
        if (handed) {
        } else if (deleg_now) {
            if constexpr (kDeleg) deleg_stage(dl, T, k, big_moves, L.rows, obs + (size_t)t0 * kObsDim);
        } else if (abl(ABL_OBS_STORE)) {
        } else {  // per-step blocks through the NT stream, in-place ones plain (kRollCpol's comment)
            store_obs_block<TPW, per_step>(L.rows, w.rows, obs + (size_t)t0 * kObsDim);
        }
        st.at(2, k);
        if (!abl(ABL_MASK_STORE)) store_mask_block<per_step>(L.mask[b], L.mbits, w.rows, S.mask + blk * 45 + (size_t)t0 * 45);
        store_small(L.small[b][lane], S, blk + t, t);
        if (big_moves) {
            __builtin_amdgcn_s_waitcnt(0);
            if (valid && get_moves(T.sw) > 255) obs[(size_t)t * kObsDim + 295] = get_moves(T.sw);
        }
        if constexpr (kDeleg) deleg_release(dl, k);
        if constexpr (kDealer) {
            if (S.policy == SPL_POLICY_UNIFORM && k + 2 < K)  // step k + 2's policy word, slot b again
                L.dl.rnd[b][lane] = uniform_draw(S.policy_seed, (uint64_t)(S.table0 + t), ply0 + (uint64_t)(k + 2));
            lds_publish(&L.dl.odone, (uint32_t)(k + 1));  // slot b is free again
        }
        if constexpr (kPartner) {
            if (pl.on)  // this side's progress, for the partner's decisions (a write-through store, no wait)
                flag_store(pl.line(pt_progress_line(pl.side)), pl.e << 16 | (uint32_t)(k + 1));
        }
        st.at(3, k);
    }
    SPL_CHECK(kDealer || osync == K, BC_BARRIER);
    (void)osync;
    if constexpr (kPartner) {
        if (pl.on) {
            pt_close<P>(pl, po, L.rows, L, S.obs, A.n, t0);
            pt_drain<P>(pl, po.cseq, L.rows, L, S.obs, A.n);  // then the partner's, until it is done
        }
    }
    st.end(w.sid, 0, false);
    if constexpr (kDeleg) {
        if (dl.on && !dl.producer) deleg_consume<P>(dl, K, L.rows, L, S.obs, A.n);
        if (dl.producer && dl.staged) deleg_reclaim<P>(dl, L.rows, L, S.obs, A.n, t0);
    }
    st.end(w.sid, 1, true);
    st.flush(w.sid, 1, K);
}

// A team of the multi-wave rollout: the set-up all its waves share, the first ws_sync(), then each wave
// to its role (rules_wave, output_wave, dealer_loop).
// `extra` is the kernel's last argument, whose meaning the kernel's RolloutExtra names: the delegation
// period (kExtraDeleg, the Sh::kDeleg kernels), the partner lead in steps (kExtraLead, the Sh::kPartner
// kernels; 0 = off, -1 = forced), or nothing (kExtraNone).
template <int P, int TPW, bool kStore, bool kDealer = false, class LdsT = WsLDS<P>, int kTeams = 1>
__device__ __forceinline__ void rollout_ws(LdsT &L, KArena A, KTables Tb, KStep S, int K, int refill, int extra,
                                           WaveRole wr = WaveRole{-1, -1}) {
    using Sh = WsShape<P, TPW, kStore, kDealer, kTeams>;
    WsWave w;
    w.lane = lane_id();
    w.multi = kTeams > 1;
    w.role = w.multi ? wr.role : (int)(threadIdx.x >> 6);
    // delegation pairs neighbouring workgroups (blockIdx b and b + 1 on adjacent XCCs): identity map
    const bool deleg_ids = Sh::kDeleg && deleg_period(extra);
    w.t0 = (w.multi ? wr.block : (deleg_ids ? (int)blockIdx.x : wg_block())) * TPW;
    w.t = w.t0 + w.lane;
    w.valid = w.lane < TPW && w.t < A.n;
    w.rows = min(TPW, A.n - w.t0);
    w.sid = w.multi ? wr.block : (int)blockIdx.x;
    w.want_final = S.autoreset && S.final_obs != nullptr;
    load_tables_lds(L, Tb);
    if constexpr (kDealer) {  // the hand-off counters start at zero (LDS is not initialised)
        if (w.role == 0 && w.lane == 0) {
            L.dl.dreq = L.dl.ddone = L.dl.rdone = L.dl.odone = L.dl.stop = L.dl.abort = 0u;
        }
    }
    // partner link: team j of workgroups b and b ^ 1, both full, K < 2^14 (the step fits a flag)
    PartnerLink pl{false, 0, 0, 0u, nullptr, nullptr, 0};
    if constexpr (Sh::kPartner) {
        const int lead = extra;
        if (lead != 0 && K < (1 << 14)) {
            const uint32_t b = blockIdx.x, pb = b ^ 1u;
            const int team = wr.block - kTeams * wg_block();
            const int t0p = (kTeams * wg_block_of(pb) + team) * 64;
            const int pair = (int)(b >> 1) * kTeams + team;
            if (pb < gridDim.x && w.t0 + 64 <= A.n && t0p + 64 <= A.n && pair < A.n / 128) {
                pl.on = true;
                pl.lead = lead;
                pl.side = (int)(b & 1u);
                pl.t0p = t0p;
                pl.fl = A.dflags + (size_t)pair * kDelegFlagWords;
                pl.pay = A.deleg + (size_t)pair * kDelegTasks * kDelegPayload;
            }
        }
        if (pl.on && w.role == 1) {  // this side's launch counter: the output wave counts, the poller reads it
            uint32_t *el = pl.line(pt_epoch_line(pl.side));
            uint32_t e = ((uint32_t)__builtin_amdgcn_readfirstlane(flag_load(el)) + 1u) & 0xFFFFu;
            e = e == 0u ? 1u : e;
            flag_store(el, e);
            pl.e = e;
            if (w.lane == 0) {
                L.pt.pepoch = e;
                L.pt.seq[0] = L.pt.seq[1] = 0u;
                L.pt.in[0] = 0ull;
                L.pt.in[1] = L.pt.in[2] = ~0ull;  // no snapshot yet (tags match no sequence number)
                L.pt.qcons[0] = L.pt.qcons[1] = ~0ull;
            }
        }
    }
    ws_sync();  // the first of every wave's 1 + K (the barrier invariant at rules_wave)
    if constexpr (Sh::kPartner) {
        if (pl.on && w.role != 1) pl.e = (uint32_t)__builtin_amdgcn_readfirstlane(L.pt.pepoch);
    }
    WSHWID(w.sid, w.role == 0 ? 0 : 1);
    // the rules wave is the critical path: it wins issue arbitration against the CU's output
    // waves (rollout store 1134 -> 1103 us per launch on one box; 1 and 3 measure the same)
    if (w.role == 0) __builtin_amdgcn_s_setprio(1);
    if constexpr (kDealer) {
        if (w.role >= 2) {
            dealer_loop<P>(L.dl, A, w.t0, pl, L.pt);
            return;
        }
    }
    if (w.role == 0) rules_wave<Sh>(L, A, Tb, S, K, refill, w, pl);
    else output_wave<Sh>(L, A, S, K, extra, w, pl);
}

// The one-workgroup-per-CU variants: kTeams teams of rollout_ws in ONE workgroup, each on its own part
// of the LDS, so the roles can be given to waves by the SIMD each one landed on; only which wave plays
// which part changes, so results are those of every other rollout shape.
//
// The six-wave dealer variant (round 4; k_rollout_*_dealer2_<P>p, 128 tables per workgroup): two
// dealer-rollout teams (rules, output, dealer wave, 64 tables each).  With two 3-wave
// workgroups per CU the dispatcher's placement is blind to the roles: a rules wave — the latency-bound
// critical path of the 4-player step — may share its SIMD with the other team's output or dealer
// wave, and the 4-player C4 share's stamps showed the workgroups dispatched second on their CU
// ending ~20 % after the first ones.  Here every wave reads its SIMD (HW_ID.SIMD_ID), the six are
// exchanged through LDS, and all waves make the same choice: the two rules waves go to the least
// occupied SIMDs (distinct ones), then the output waves, the dealers take the rest.
//
// The quad variant (round 5; k_rollout_*_quad_<P>p, 256 tables per workgroup):
// four two-wave teams (rules + output wave, 64 tables each) in ONE 512-thread workgroup — the
// headline's 65 536 tables in 256 workgroups, all resident.  At one workgroup per CU the partner
// hand-off (PartnerLink; the rules wave polls the pair's flag words, as it did in round 4's two-wave
// kernel) is a hand-off of the guide's first measured row ("hipMalloc; one per CU", 4-byte sc1 stores
// and loads, one signalling lane per storing wave after its vmcnt(0)), which the two-wave kernel at
// four workgroups per CU was not.  Roles by SIMD as in the six-wave dealer: every
// wave reads its SIMD, and the rules waves go to distinct SIMDs (each SIMD: one rules + one output
// wave).
template <class TeamLds, int kTeams>
struct __align__(16) WsTeamsLDS {
    TeamLds team[kTeams];
    uint32_t simd[kTeams * TeamLds::kWaves];
};
template <int P>
using WsDeal2LDS = WsTeamsLDS<WsDealLDS<P>, 2>;
template <int P>
using WsQuadLDS = WsTeamsLDS<WsLDS<P>, 4>;
static_assert(sizeof(WsDeal2LDS<2>) <= 163840 && sizeof(WsDeal2LDS<3>) <= 163840 && sizeof(WsDeal2LDS<4>) <= 163840,
              "the six-wave dealer rollout needs one workgroup per CU");
static_assert(sizeof(WsQuadLDS<2>) <= 163840 && sizeof(WsQuadLDS<3>) <= 163840 && sizeof(WsQuadLDS<4>) <= 163840,
              "the quad rollout needs one workgroup per CU");

// wave-uniform: (team * kRoles + role) of wave w given the kWaves waves' SIMDs.  Waves are taken in the
// order (occupancy of their SIMD, wave index); each role takes kWaves / kRoles of them, preferring SIMDs
// that do not hold a wave of that role yet: rules first, then output, then (kRoles = 3) dealer.  Static
// indexing only.
template <int kWaves, int kRoles>
__device__ __forceinline__ int team_assign(const uint32_t (&simd)[kWaves], int w) {
    static_assert(kWaves <= 8 && kWaves % kRoles == 0, "the sort key holds 8 waves; whole teams");
    int key[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        int occ = 0;
#pragma unroll
        for (int j = 0; j < kWaves; ++j) occ += simd[j] == simd[i] ? 1 : 0;
        key[i] = occ * 8 + i;
    }
    int rank[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        int r = 0;
#pragma unroll
        for (int j = 0; j < kWaves; ++j) r += key[j] < key[i] ? 1 : 0;
        rank[i] = r;
    }
    int code[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) code[i] = -1;
#pragma unroll
    for (int role = 0; role < kRoles; ++role) {
        uint32_t used = 0u;  // SIMDs that already hold a wave of this role
        int got = 0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int r = 0; r < kWaves; ++r)
#pragma unroll
                for (int i = 0; i < kWaves; ++i) {
                    const bool take = rank[i] == r && got < kWaves / kRoles && code[i] < 0 &&
                                      (pass == 1 || ((used >> (simd[i] & 3u)) & 1u) == 0u);
                    code[i] = take ? got * kRoles + role : code[i];
                    used |= take ? 1u << (simd[i] & 3u) : 0u;
                    got += take ? 1 : 0;
                }
    }
    int mine = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) mine = i == w ? code[i] : mine;
    return mine;
}

template <int P, bool kStore, bool kDealer, int kTeams, class TeamLds>
__device__ __forceinline__ void rollout_teams(WsTeamsLDS<TeamLds, kTeams> &L, KArena A, KTables Tb, KStep S, int K,
                                              int refill, int lead) {
    constexpr int kRoles = TeamLds::kWaves, kWaves = kTeams * kRoles;
    static_assert(kRoles == (kDealer ? 3 : 2), "a dealer team has three waves, the others two");
    const int w = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) L.simd[w] = (__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 4) & 3u;
    __syncthreads();
    uint32_t simd[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) simd[i] = __builtin_amdgcn_readfirstlane(L.simd[i]);
    const int code = __builtin_amdgcn_readfirstlane(team_assign<kWaves, kRoles>(simd, w));
    const int team = code / kRoles;
    rollout_ws<P, 64, kStore, kDealer, TeamLds, kTeams>(L.team[team], A, Tb, S, K, refill, lead,
                                                        WaveRole{code % kRoles, kTeams * wg_block() + team});
}

// Every multi-wave rollout kernel, one line each:
//   X(name, threads per workgroup, tables per workgroup, extra argument, LDS type, body)
// in the order of kRolloutKernels: [shape - 2][per_step][players - 2], the shapes being
// spl_ctx_set_rollout_pipeline's 2 two waves, 3 two waves half-populated (32 tables), 4 the three-wave dealer,
// 5 the six-wave dealer, 6 quad.  (Shape 0, the one-wave k_rollout<P>, takes other arguments and is launched
// by name.)  One kernel name per instantiation: a rocprofv3 --stats summary names kernels by the text before
// the template argument list when it truncates, so the per-step store (the headline), the in-place variant
// and the shapes must differ there to be separate rows.
// The extra (last) kernel argument, 0 unless every workgroup of the grid is resident at once: the two-wave
// store's static delegation period, or the partner lead of the one-workgroup-per-CU stores.
enum RolloutExtra { kExtraNone, kExtraDeleg, kExtraLead };
#define SPL_ROLLOUT_KERNELS(X)                                                                        \
    X(k_rollout_inplace_2p, 128, 64, kExtraNone, WsLDS<2>, rollout_ws<2, 64, false>)                  \
    X(k_rollout_inplace_3p, 128, 64, kExtraNone, WsLDS<3>, rollout_ws<3, 64, false>)                  \
    X(k_rollout_inplace_4p, 128, 64, kExtraNone, WsLDS<4>, rollout_ws<4, 64, false>)                  \
    X(k_rollout_store_2p, 128, 64, kExtraDeleg, WsLDS<2>, rollout_ws<2, 64, true>)                    \
    X(k_rollout_store_3p, 128, 64, kExtraDeleg, WsLDS<3>, rollout_ws<3, 64, true>)                    \
    X(k_rollout_store_4p, 128, 64, kExtraDeleg, WsLDS<4>, rollout_ws<4, 64, true>)                    \
    X(k_rollout_inplace_half_2p, 128, 32, kExtraNone, WsLDS<2>, rollout_ws<2, 32, false>)             \
    X(k_rollout_inplace_half_3p, 128, 32, kExtraNone, WsLDS<3>, rollout_ws<3, 32, false>)             \
    X(k_rollout_inplace_half_4p, 128, 32, kExtraNone, WsLDS<4>, rollout_ws<4, 32, false>)             \
    X(k_rollout_store_half_2p, 128, 32, kExtraNone, WsLDS<2>, rollout_ws<2, 32, true>)                \
    X(k_rollout_store_half_3p, 128, 32, kExtraNone, WsLDS<3>, rollout_ws<3, 32, true>)                \
    X(k_rollout_store_half_4p, 128, 32, kExtraNone, WsLDS<4>, rollout_ws<4, 32, true>)                \
    X(k_rollout_inplace_dealer_2p, 192, 64, kExtraNone, WsDealLDS<2>, rollout_ws<2, 64, false, true>) \
    X(k_rollout_inplace_dealer_3p, 192, 64, kExtraNone, WsDealLDS<3>, rollout_ws<3, 64, false, true>) \
    X(k_rollout_inplace_dealer_4p, 192, 64, kExtraNone, WsDealLDS<4>, rollout_ws<4, 64, false, true>) \
    X(k_rollout_store_dealer_2p, 192, 64, kExtraNone, WsDealLDS<2>, rollout_ws<2, 64, true, true>)    \
    X(k_rollout_store_dealer_3p, 192, 64, kExtraNone, WsDealLDS<3>, rollout_ws<3, 64, true, true>)    \
    X(k_rollout_store_dealer_4p, 192, 64, kExtraNone, WsDealLDS<4>, rollout_ws<4, 64, true, true>)    \
    X(k_rollout_inplace_dealer2_2p, 384, 128, kExtraNone, WsDeal2LDS<2>, rollout_teams<2, false, true, 2>) \
    X(k_rollout_inplace_dealer2_3p, 384, 128, kExtraNone, WsDeal2LDS<3>, rollout_teams<3, false, true, 2>) \
    X(k_rollout_inplace_dealer2_4p, 384, 128, kExtraNone, WsDeal2LDS<4>, rollout_teams<4, false, true, 2>) \
    X(k_rollout_store_dealer2_2p, 384, 128, kExtraLead, WsDeal2LDS<2>, rollout_teams<2, true, true, 2>) \
    X(k_rollout_store_dealer2_3p, 384, 128, kExtraLead, WsDeal2LDS<3>, rollout_teams<3, true, true, 2>) \
    X(k_rollout_store_dealer2_4p, 384, 128, kExtraLead, WsDeal2LDS<4>, rollout_teams<4, true, true, 2>) \
    X(k_rollout_inplace_quad_2p, 512, 256, kExtraNone, WsQuadLDS<2>, rollout_teams<2, false, false, 4>) \
    X(k_rollout_inplace_quad_3p, 512, 256, kExtraNone, WsQuadLDS<3>, rollout_teams<3, false, false, 4>) \
    X(k_rollout_inplace_quad_4p, 512, 256, kExtraNone, WsQuadLDS<4>, rollout_teams<4, false, false, 4>) \
    X(k_rollout_store_quad_2p, 512, 256, kExtraLead, WsQuadLDS<2>, rollout_teams<2, true, false, 4>) \
    X(k_rollout_store_quad_3p, 512, 256, kExtraLead, WsQuadLDS<3>, rollout_teams<3, true, false, 4>) \
    X(k_rollout_store_quad_4p, 512, 256, kExtraLead, WsQuadLDS<4>, rollout_teams<4, true, false, 4>)
#define X(NAME, THREADS_, TPW_, EXTRA_, LDS_, ...)                                                                  \
    __global__ __launch_bounds__(THREADS_) void NAME(KArena A, KTables Tb, KStep S, int K, int refill, int extra) { \
        __shared__ LDS_ L;                                                                                          \
        __VA_ARGS__(L, A, Tb, S, K, refill, extra);                                                                 \
    }
SPL_ROLLOUT_KERNELS(X)
#undef X
struct RolloutKernel {
    const char *name;
    void (*fn)(KArena, KTables, KStep, int, int, int);
    int threads, tpw;  // per workgroup: threads, tables
    RolloutExtra extra;
};
#define X(NAME, THREADS_, TPW_, EXTRA_, LDS_, ...) {#NAME, NAME, THREADS_, TPW_, EXTRA_},
static const RolloutKernel kRolloutKernels[5 * 2 * 3] = {SPL_ROLLOUT_KERNELS(X)};
#undef X
static const RolloutKernel &rollout_kernel(int shape, bool per_step, int players) {
    return kRolloutKernels[((shape - 2) * 2 + (per_step ? 1 : 0)) * 3 + players - 2];
}

// Explicit reset (SplendorEnv.reset / VectorEnv.reset), then observation + mask of all tables.
template <int P>
__global__ __launch_bounds__(64) void k_reset(KArena A, KTables Tb, const uint64_t *pcg_in, const uint8_t *mask_in,
                                              int32_t *obs, int8_t *mask_out, const uint32_t *eseed_in) {
    __shared__ BlockLDS L;
    const int lane = lane_id();
    const int t0 = blockIdx.x * 64;
    const int t = t0 + lane;
    const bool valid = t < A.n;
    const int rows = min(64, A.n - t0);
    load_tables_lds(L, Tb);
    Tab<P> T;
    if (valid) load_tab(T, A, t);
    else fresh_state(T, 0u, empty_deal());
    wave_lds_sync();
    const bool doit = valid && (mask_in == nullptr || mask_in[t] != 0);
    uint8_t *scr = &L.rows[lane * kScratchStride];
    uint32_t *const mtx = reinterpret_cast<uint32_t *>(&L.rows[64 * kScratchStride]);  // LaneMT continuation
    if (doit) {
        if (eseed_in) {  // engine/state.py:181-211 initial_state(P, seed) from an explicit engine seed
            Deal d0;     // no pool: a later reset() without a seed deals inline
            deal_into(eseed_in[t], P, slot_rec(A, t, 0), scr, d0, mtx);
            fresh_state(T, ring_bits(0, kSlotRecords - 1), d0);
        } else if (pcg_in) {  // reset(seed=...): restart this table's np_random stream, deal every record
            Pcg64 g;
            g.s_hi = pcg_in[4 * (size_t)t];
            g.s_lo = pcg_in[4 * (size_t)t + 1];
            g.inc_hi = pcg_in[4 * (size_t)t + 2];
            g.inc_lo = pcg_in[4 * (size_t)t + 3];
            g.has32 = 0;
            g.u32 = 0;
            // record 0 = this episode, records 1.. = the next episodes in stream order: the ring
            // starts full, so refills (one deal per table per call) only have to keep pace
            Deal d0, d;
            deal_into(g.engine_seed(), P, slot_rec(A, t, 0), scr, d0, mtx);
            for (int r = 1; r < kSlotRecords; ++r) {
                deal_into(g.engine_seed(), P, slot_rec(A, t, r), scr, d, mtx);
                if (r == 1) store_pool(A, t, d);
            }
            store_pcg(A, t, g);
            fresh_state(T, ring_bits(0, 0), d0);
        } else {       // reset() without a seed: continue the stream (pool deal)
            Deal d = pend_of(T.sw[SW_MISC]) < kSlotRecords - 1 ? load_pool(A, t) : empty_deal();
            uint32_t fl = 0;
            if (flip_to_pool<P>(T, A, t, d, scr, mtx, fl)) store_pool(A, t, d);
        }
    }
    wave_lds_sync();
    // env info mask, also the legal-mask cache of every stored state (reset or not)
    const uint64_t lm = (valid && !is_terminal(T.sw)) ? legal_of(T, L) : 0ull;
    if (obs || mask_out) {
        encode_row(T, L.rows, L);
        L.mask[lane] = lm;
        wave_lds_sync();
        if (obs) store_obs_block(L.rows, rows, obs + (size_t)t0 * kObsDim);
        if (mask_out) store_mask_block(L.mask, L.mbits, rows, mask_out + (size_t)t0 * 45);
    }
    if (valid) store_tab(T, A, t, lm, Tb.mtag);
}

// Pool refill: every table with consumed pool records gets ONE of them re-dealt per call, the
// earliest free one in ring order (the next episode's deal comes first in the engine-seed
// stream), so a call costs one deal per wave however many resets happened since the last one.
// The deal is one long serial chain per lane (CPython init_by_array + the shuffle's MT outputs):
// a wave's time is the same whether it carries 5 or 64 pending tables, so the scratch is padded
// to a quarter of the CU's LDS and the dispatcher spreads the waves one per SIMD.
constexpr int kRefillLds = 40 * 1024;
template <int P>
__global__ __launch_bounds__(64) void k_refill(KArena A) {
    __shared__ uint8_t scr_all[kRefillLds] __attribute__((aligned(16)));
    const int t = blockIdx.x * 64 + lane_id();
    if (t >= A.n) return;
    const size_t mi = (size_t)SW_MISC * A.n + t;
    const uint32_t misc = A.planes[mi];
    if (pend_of(misc) == 0) return;
    Deal pool;
    bool pool_dirty = false;
    A.planes[mi] = refill_table<P>(A, t, misc, &scr_all[lane_id() * kScratchStride],
                                   reinterpret_cast<uint32_t *>(&scr_all[64 * kScratchStride]), pool, pool_dirty);
    if (pool_dirty) store_pool(A, t, pool);  // it was the next pool: words to the pool planes
}

// Observation and/or mask of the current state (spl_encode / spl_legal).
template <int P>
__global__ __launch_bounds__(64) void k_observe(KArena A, KTables Tb, int32_t *obs, int8_t *mask_out) {
    __shared__ BlockLDS L;
    const int lane = lane_id();
    const int t0 = blockIdx.x * 64;
    const int t = t0 + lane;
    const bool valid = t < A.n;
    const int rows = min(64, A.n - t0);
    load_tables_lds(L, Tb);
    Tab<P> T;
    if (valid) load_tab(T, A, t);
    else fresh_state(T, 0u, empty_deal());
    wave_lds_sync();
    if (obs) encode_row(T, L.rows, L);
    L.mask[lane] = valid ? legal_of(T, L) : 0ull;  // engine legal_moves (no terminal check)
    wave_lds_sync();
    if (obs) {
        store_obs_block(L.rows, rows, obs + (size_t)t0 * kObsDim);
        if (__any(valid && get_moves(T.sw) > 255)) {
            __builtin_amdgcn_s_waitcnt(0);
            if (valid && get_moves(T.sw) > 255) obs[(size_t)t * kObsDim + 295] = get_moves(T.sw);
        }
    }
    if (mask_out) store_mask_block(L.mask, L.mbits, rows, mask_out + (size_t)t0 * 45);
}

// One wave per 64 tables: the wave's 64 x 45 mask bytes are read coalesced (64 consecutive bytes
// per instruction) into LDS, then each lane packs its table's row (a per-lane stride-45 byte
// walk would touch a new 64-byte segment per lane per byte).
__global__ __launch_bounds__(64) void k_sample(int n, const int8_t *mask, int32_t *actions, uint64_t seed, uint64_t ply,
                                               int64_t table0) {
    __shared__ uint32_t rows_w[64 * 45 / 4];
    int8_t *rows = reinterpret_cast<int8_t *>(rows_w);
    const int t0 = blockIdx.x * 64, lane = lane_id();
    const int nb = min(64, n - t0) * 45;
    const int8_t *src = mask + (size_t)t0 * 45;
    if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && nb == 64 * 45) {  // 720 dwords, 12 per lane
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
    wave_lds_sync();
    const int t = t0 + lane;
    if (t >= n) return;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 45; ++i) m |= (uint64_t)(rows[lane * 45 + i] != 0) << i;
    actions[t] = sample_uniform(m, seed, (uint64_t)(table0 + t), ply);
}

// spl_step_info: the per-table flags byte split into the gymnasium info planes (illegal_action,
// draw, turn_limit as 0/1 bytes, [3][n]) and a running count of the tables whose flags carry an
// error (out-of-range action, step after termination), one atomic per wave that has any
__global__ __launch_bounds__(256) void k_step_info(int n, const uint8_t *flags, uint8_t *info,
                                                   unsigned long long *errors) {
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    const uint32_t f = t < n ? flags[t] : 0u;
    if (t < n) {
        info[t] = (f & SPL_F_ILLEGAL) ? 1 : 0;
        info[(size_t)n + t] = (f & SPL_F_DRAW) ? 1 : 0;
        info[2 * (size_t)n + t] = (f & SPL_F_TURN_LIMIT) ? 1 : 0;
    }
    const uint64_t bad = __ballot((f & (SPL_F_OOB | SPL_F_AFTER_TERMINAL)) != 0);
    if (bad && lane_id() == __ffsll((unsigned long long)bad) - 1) atomicAdd(errors, (unsigned long long)__popcll(bad));
}

// host view <-> arena (splendor_table.h)
template <int P>
__global__ __launch_bounds__(64) void k_download(KArena A, int first, int count, spl_table_t *out) {
    const int i = blockIdx.x * 64 + lane_id();
    if (i >= count) return;
    const int t = first + i;
    Tab<P> T;
    load_tab(T, A, t);
    spl_table_t &v = out[i];
    const uint32_t *sw = T.sw;
    v.num_players = P;
    int bank[6];
    get_bank(sw, bank);
    for (int c = 0; c < 6; ++c) v.bank[c] = bank[c];
    const uint32_t owners = (sw[SW_NOB1] >> 8) & 0x7FFFu;
    const int nn = (int)bget(sw[SW_DECK], 3);
    for (int q = 0; q < SPL_MAX_PLAYERS; ++q) {
        spl_player_t &pv = v.players[q];
        for (int k = 0; k < 3; ++k) pv.reserved[k] = -1, pv.revealed[k] = 0;
        for (int k = 0; k < 5; ++k) pv.nobles[k] = -1;
        for (int c = 0; c < 6; ++c) pv.tokens[c] = 0;
        for (int c = 0; c < 5; ++c) pv.bonuses[c] = 0;
        pv.prestige = pv.n_reserved = pv.n_nobles = 0;
        if (q >= P) continue;
        const Pl p = unpack_pl(T.pw[q]);
        for (int c = 0; c < 6; ++c) pv.tokens[c] = p.tok[c];
        for (int c = 0; c < 5; ++c) pv.bonuses[c] = p.bon[c];
        pv.prestige = p.pres;
        pv.n_reserved = p.nres;
        for (int k = 0; k < p.nres; ++k) {
            pv.reserved[k] = p.res[k];
            pv.revealed[k] = (p.rev >> k) & 1;
        }
        int nk = 0;
        for (int s = 0; s < nn && s < 5; ++s) {
            if ((int)((owners >> (3 * s)) & 7u) == q + 1)
                pv.nobles[nk++] = s < 4 ? (int)bget(sw[SW_NOB0], s) : (int)bget(sw[SW_NOB1], 0);
        }
        pv.n_nobles = nk;
    }
    for (int k = 0; k < 12; ++k) {
        const int id = (int)bget(sw[SW_BOARD + k / 4], k % 4);
        v.board[k] = id == 0xFF ? -1 : id;
    }
    const uint8_t *rec = live_rec(A, t, sw[SW_MISC]);
    for (int tt = 0; tt < 3; ++tt) {
        const int len = (int)bget(sw[SW_DECK], tt);
        v.deck_len[tt] = len;
        for (int k = 0; k < 40; ++k) v.decks[tt][k] = k < len ? (int)rec[tier_base(tt) + k] : -1;
    }
    v.n_nobles = nn;
    for (int s = 0; s < 5; ++s) {
        const int idx = s < 4 ? (int)bget(sw[SW_NOB0], s) : (int)bget(sw[SW_NOB1], 0);
        const bool taken = ((owners >> (3 * s)) & 7u) != 0 || idx >= 10;
        v.nobles[s] = (s < nn && !taken) ? idx : -1;
    }
    v.to_play = get_to_play(sw);
    v.turn_count = get_turn(sw);
    v.move_count = get_moves(sw);
    v.game_over = (sw[SW_MISC] & ST_GAME_OVER) ? 1 : 0;
    v.winner = get_winner(sw);
    v.turn_limit_reached = (sw[SW_MISC] & ST_TURN_LIMIT) ? 1 : 0;
}

template <int P>
__global__ __launch_bounds__(64) void k_upload(KArena A, int first, int count, const spl_table_t *in) {
    const int i = blockIdx.x * 64 + lane_id();
    if (i >= count) return;
    const int t = first + i;
    const spl_table_t &v = in[i];
    Tab<P> T;
    uint32_t *sw = T.sw;
    const uint32_t old_misc = A.planes[(size_t)SW_MISC * A.n + t];
    int bank[6];
    for (int c = 0; c < 6; ++c) bank[c] = v.bank[c];
    sw[SW_BANK1] = ((uint32_t)v.to_play << 16) | ((uint32_t)v.turn_count << 24);
    put_bank(sw, bank);
    sw[SW_MISC] = ((uint32_t)v.move_count & 0xFFFFu) | (v.game_over ? ST_GAME_OVER : 0u) |
                  (v.turn_limit_reached ? ST_TURN_LIMIT : 0u) | (old_misc & (ST_ACTIVE | ST_PEND)) |
                  ((uint32_t)(v.winner + 1) << 24);
    for (int tt = 0; tt < 3; ++tt) {
        uint32_t w = 0;
        for (int s = 0; s < 4; ++s) w |= (uint32_t)(v.board[tt * 4 + s] < 0 ? 0xFF : v.board[tt * 4 + s]) << (8 * s);
        sw[SW_BOARD + tt] = w;
    }
    sw[SW_DECK] = (uint32_t)v.deck_len[0] | ((uint32_t)v.deck_len[1] << 8) | ((uint32_t)v.deck_len[2] << 16) |
                  ((uint32_t)v.n_nobles << 24);
    // visible slots keep their noble; taken slots get the players' nobles in order
    int slot_idx[5];
    uint32_t owners = 0;
    int next_taken = 0;
    for (int s = 0; s < 5; ++s) slot_idx[s] = (s < v.n_nobles && v.nobles[s] >= 0) ? v.nobles[s] : 0xFF;
    for (int s = 0; s < 5 && s < v.n_nobles; ++s)
        if (v.nobles[s] < 0) owners |= 7u << (3 * s);
    for (int q = 0; q < P; ++q) {
        for (int k = 0; k < v.players[q].n_nobles; ++k) {
            while (next_taken < v.n_nobles && !(v.nobles[next_taken] < 0)) ++next_taken;
            if (next_taken < v.n_nobles) {
                slot_idx[next_taken] = v.players[q].nobles[k];
                owners = (owners & ~(7u << (3 * next_taken))) | ((uint32_t)(q + 1) << (3 * next_taken));
                ++next_taken;
            }
        }
    }
    sw[SW_NOB0] = (uint32_t)slot_idx[0] | ((uint32_t)slot_idx[1] << 8) | ((uint32_t)slot_idx[2] << 16) |
                  ((uint32_t)slot_idx[3] << 24);
    sw[SW_NOB1] = (uint32_t)slot_idx[4] | (owners << 8);
    for (int q = 0; q < P; ++q) {
        Pl p;
        const spl_player_t &pv = v.players[q];
        for (int c = 0; c < 6; ++c) p.tok[c] = pv.tokens[c];
        for (int c = 0; c < 5; ++c) p.bon[c] = pv.bonuses[c];
        p.pres = pv.prestige;
        p.nres = pv.n_reserved;
        p.rev = 0;
        for (int k = 0; k < 3; ++k) {
            p.res[k] = k < pv.n_reserved ? pv.reserved[k] : 0xFF;
            p.rev |= (k < pv.n_reserved && pv.revealed[k]) ? (1 << k) : 0;
        }
        pack_pl(p, T.pw[q]);
    }
    store_tab(T, A, t, 0ull, 0u);  // a crafted state: its legal mask is unknown until a step evaluates it
    uint8_t *rec = slot_rec(A, t, active_of(old_misc));
    for (int tt = 0; tt < 3; ++tt)
        for (int k = 0; k < tier_size(tt); ++k) rec[tier_base(tt) + k] = (uint8_t)(k < v.deck_len[tt] ? v.decks[tt][k] : 0xFF);
}

}  // namespace spl

#include "spl_engine_succ.h"

namespace spl {

// spl_successors: one wave per (64-table block, action); grid (blocks, 45), the action in blockIdx.y (scalar)
template <int P>
__global__ __launch_bounds__(64) void k_successors(KArena A, KTables Tb, spl_succ_args_t S) {
#ifdef SPL_SUCC_BLOCKLDS  // experiment builds: the rollout's staging block, the continuation in its terminal rows
    __shared__ BlockLDS L;
    uint32_t *const mtx = reinterpret_cast<uint32_t *>(L.frows);
#else
    __shared__ SuccLDS L;
    uint32_t *const mtx = L.mtx;
#endif
    successors_wave<P>(L, mtx, A, Tb, S, (int)blockIdx.y);
}

}  // namespace spl

#include "spl_engine_pairs.h"

namespace spl {

// spl_successors_pairs, three launches on one stream: the legal masks and block counts (one wave per 64 tables), their
// prefix (one workgroup), and the rows: one wave per (64-table block, action), grid (blocks, 45) as k_successors
template <int P>
__global__ __launch_bounds__(64) void k_pairs_count(KArena A, KTables Tb, uint64_t *legal, int32_t *base) {
    __shared__ Consts L;
    pairs_count_wave<P>(L, A, Tb, legal, base);
}

__global__ __launch_bounds__(kPairsScanThreads) void k_pairs_scan(int32_t *base, int nb) {
    __shared__ int32_t wsum[kPairsScanThreads / 64];
    pairs_scan_block(base, nb, wsum);
}

template <int P>
__global__ __launch_bounds__(64) void k_successors_pairs(KArena A, KTables Tb, spl_succ_pairs_args_t S) {
    __shared__ SuccLDS L;
    pairs_write_wave<P>(L, A, Tb, S, (int)blockIdx.y);
}

}  // namespace spl

// ==========================================================================================
// host side: C-ABI
// ==========================================================================================
using namespace spl;

struct spl_ctx_s {
    int device;
    uint4 *cards;
    uint2 *nobles;
    uint4 *lut;
    int refill_period;
    int refill_fused;  // spl_rollout: refill inside the rollout launch (default) or as a k_refill launch after it
    int pipeline;      // spl_rollout's shape: 0 one wave per 64 tables, 1 auto (rollout_shape), 2-6 see SPL_ROLLOUT_KERNELS
    int resident[7][5];  // [shape 2..6][players]: workgroups of the shape's per-step store kernel resident per
                         // device (occupancy x CUs)
    int deleg_every;     // spl_rollout per-step store: rollout-store delegation every n-th step (0 = off)
    int partner_lead;    // per-step store partner hand-off lead in steps (0 off, < 0 forced)
    uint32_t mtag;         // legal-mask cache tag of this context's card table (card_table_tag), 1..65535, or 0
    uint32_t free_card;    // 1 when a card of the table costs nothing (kTagFreeCard of KTables::mtag)
    int step_tail;         // spl_step shape: -1 auto (the tail wave up to step_tail_blocks workgroups), 0 two waves, 1 three
    int64_t step_tail_blocks;
    uint64_t *fault_host;  // host-mapped, fine-grained: the serial of a launch that faulted (0 = none), spl_ctx_faults
    uint64_t *fault_dev;   // its device address (KStep::fault)
    uint64_t launches;     // launch serial (KStep::fault_tag)
    void *stage;
    size_t stage_bytes;
};

static thread_local std::string g_err;

// every translation unit's error channel (spl_common.h)
int spl_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
static inline int fail(int code, const std::string &msg) { return spl_fail(code, msg); }

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return fail(SPL_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

static KTables ktables(const spl_ctx_t *c) {
    return KTables{c->cards, c->nobles, c->lut, c->mtag | (c->free_card ? kTagFreeCard : 0u)};
}

static int check_arena(const spl_ctx_t *ctx, const spl_arena_t *a) {
    if (!ctx) return fail(SPL_E_ARG, "null context");
    if (!a || !a->base) return fail(SPL_E_ARG, "null arena");
    if (a->players < 2 || a->players > 4) return fail(SPL_E_ARG, "players must be 2..4");
    if (a->n <= 0) return fail(SPL_E_ARG, "arena must hold at least one table");
    if (((uintptr_t)a->base & 255u) != 0) return fail(SPL_E_ARG, "arena base must be 256-byte aligned");
    if (a->bytes < spl_arena_bytes(a->n, a->players)) return fail(SPL_E_ARG, "arena too small");
    return SPL_OK;
}

static KArena karena(const spl_arena_t *a) {
    const ArenaLayout L = arena_layout(a->n, a->players);
    uint8_t *b = static_cast<uint8_t *>(a->base);
    return KArena{reinterpret_cast<uint32_t *>(b + L.planes), reinterpret_cast<uint32_t *>(b + L.pool), b + L.slots,
                  b + L.pcg, a->n, b + L.deleg, reinterpret_cast<uint32_t *>(b + L.dflags),
                  reinterpret_cast<uint32_t *>(b + L.legal)};
}

static int launch_check() { return spl_launched("kernel launch"); }

static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 63) / 64); }

extern "C" {

int spl_abi_version(void) { return SPL_ABI_VERSION; }

#ifdef SPL_STAMPS
int spl_debug_set_stamps(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)));
    return SPL_OK;
}
int spl_debug_set_ws_clk(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wsclk), &buf, sizeof(buf)));
    return SPL_OK;
}
int spl_debug_set_ws_end(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wsend), &buf, sizeof(buf)));
    return SPL_OK;
}
int spl_debug_set_ws_hwid(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wshwid), &buf, sizeof(buf)));
    return SPL_OK;
}
int spl_debug_set_ws_stamps(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wsstamps), &buf, sizeof(buf)));
    return SPL_OK;
}
int spl_debug_set_rollout_stamps(void *buf) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rstamps), &buf, sizeof(buf)));
    return SPL_OK;
}
#endif

int spl_debug_bounds_flags(uint32_t *flags, int clear) {
#ifdef SPL_BOUNDS_CHECK
    if (!flags) return fail(SPL_E_ARG, "null flags");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(flags, HIP_SYMBOL(g_bounds_flags), sizeof(uint32_t)));
    if (clear) {
        const uint32_t z = 0;
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bounds_flags), &z, sizeof(z)));
    }
    return SPL_OK;
#else
    (void)flags;
    (void)clear;
    return fail(SPL_E_ARG, "not a bounds-check build (-DSPL_BOUNDS_CHECK)");
#endif
}

int spl_debug_set_stream_limit(int outputs) {
    if (outputs < 1 || outputs > MTStream::kMaxOut) return fail(SPL_E_ARG, "stream limit must be 1..454");
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stream_limit), &outputs, sizeof(outputs)));
    return SPL_OK;
}

int spl_debug_set_spin_limit(int64_t polls) {
    if (polls > (int64_t)kSpinLimit) return fail(SPL_E_ARG, "spin limit must be <= 2^22 (negative = default)");
    const uint32_t v = polls < 0 ? kSpinLimit : (uint32_t)polls;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_spin_limit), &v, sizeof(v)));
    return SPL_OK;
}

const char *spl_last_error(void) { return g_err.c_str(); }

int64_t spl_arena_bytes(int32_t n, int32_t players) {
    if (n <= 0 || players < 2 || players > 4) return -1;
    return arena_layout(n, players).total;
}

// The legal-mask cache tag of a card table (the 90 card and 10 noble records the kernels read; legal_moves
// depends on the state and the card costs only): one tag per DISTINCT table in this process, never
// recycled, so an arena stepped under two contexts reuses masks exactly when their tables are equal (an
// edited table gets a tag of its own; contexts of the canonical table share one).  Past 65 535 distinct
// tables a context gets tag 0: it neither trusts a cached mask nor publishes one (LegalCache::known).
static uint32_t card_table_tag(const std::vector<uint4> &crec, const std::vector<uint2> &nrec) {
    static std::mutex mu;
    static std::map<std::string, uint32_t> tags;
    std::string key(reinterpret_cast<const char *>(crec.data()), crec.size() * sizeof(uint4));
    key.append(reinterpret_cast<const char *>(nrec.data()), nrec.size() * sizeof(uint2));
    std::lock_guard<std::mutex> g(mu);
    const auto it = tags.find(key);
    if (it != tags.end()) return it->second;
    if (tags.size() >= kLegalTagMax) return 0u;
    const uint32_t tag = (uint32_t)tags.size() + 1u;
    tags.emplace(std::move(key), tag);
    return tag;
}

int spl_ctx_create(int device, const int32_t *cards, const int32_t *nobles, spl_ctx_t **out) {
    if (!cards || !nobles || !out) return fail(SPL_E_ARG, "null argument");
    *out = nullptr;
    // constant records: observation-ready card bytes (engine/encode.py:77-96) + costs
    std::vector<uint4> crec(90);
    bool free_card = false;
    int max_card_points = 0, max_noble_points = 0;
    for (int i = 0; i < 90; ++i) {
        const int32_t *c = cards + 8 * i;
        if (c[0] < 1 || c[0] > 3 || c[1] < 0 || c[1] > 4 || c[2] < 0 || c[2] > 255)
            return fail(SPL_E_ARG, "bad card table row " + std::to_string(i));
        uint8_t b[16] = {0};
        b[0] = 1;
        b[1] = (uint8_t)c[0];
        b[2] = (uint8_t)c[2];
        b[3 + c[1]] = 1;
        for (int k = 0; k < 5; ++k) {
            if (c[3 + k] < 0 || c[3 + k] > 255) return fail(SPL_E_ARG, "bad card cost");
            b[8 + k] = (uint8_t)c[3 + k];
        }
        b[13] = (uint8_t)c[1];
        free_card |= c[3] + c[4] + c[5] + c[6] + c[7] == 0;
        max_card_points = std::max(max_card_points, (int)c[2]);
        memcpy(&crec[i], b, 16);
    }
    std::vector<uint2> nrec(10);
    for (int i = 0; i < 10; ++i) {
        const int32_t *n = nobles + 6 * i;
        uint8_t b[8] = {0};
        b[0] = 1;
        for (int k = 0; k < 5; ++k) {
            if (n[k] < 0 || n[k] > 255) return fail(SPL_E_ARG, "bad noble table");
            b[1 + k] = (uint8_t)n[k];
        }
        if (n[5] < 0 || n[5] > 255) return fail(SPL_E_ARG, "bad noble points");
        b[6] = (uint8_t)n[5];
        max_noble_points = std::max(max_noble_points, (int)n[5]);
        memcpy(&nrec[i], b, 8);
    }
    // a player enters a move with at most 14 prestige (15 ends the game) and gains at most one card and
    // one noble in it: the largest value the prestige byte of the packed player words has to hold
    if (14 + max_card_points + max_noble_points > 255)
        return fail(SPL_E_RANGE, "card and noble points overflow the prestige byte: 14 + max card points (" +
                                     std::to_string(max_card_points) + ") + max noble points (" +
                                     std::to_string(max_noble_points) + ") must not exceed 255");
    HIP_TRY(hipSetDevice(device));
    int resident[7][5] = {};
    {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        for (int shape = 2; shape <= 6; ++shape)
            for (int p = 2; p <= 4; ++p) {
                const RolloutKernel &k = rollout_kernel(shape, true, p);
                int occ = 0;
                HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.fn, k.threads, 0));
                resident[shape][p] = occ * cus;
            }
    }
    spl_ctx_t *c = new spl_ctx_t();
    c->device = device;
    c->mtag = card_table_tag(crec, nrec);
    c->free_card = free_card ? 1u : 0u;
    c->refill_period = 64;
    c->refill_fused = 1;
    c->deleg_every = kDelegEveryDefault;
    c->partner_lead = kPartnerLeadDefault;
    c->step_tail = -1;
    {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        // up to three workgroups per CU (49 152 tables on 256 CUs): per step 20.0 against 20.45 us there,
        // 24.2 against 22.35 us at four (profiles/r06/step_shape_48k_64k_r06al.txt)
        c->step_tail_blocks = 3 * (int64_t)cus;
    }
    c->pipeline = 1;
    memcpy(c->resident, resident, sizeof(resident));
    if (hipMalloc(&c->cards, sizeof(uint4) * 90) != hipSuccess || hipMalloc(&c->nobles, sizeof(uint2) * 10) != hipSuccess ||
        hipMalloc(&c->lut, sizeof(uint4) * kLutEntries) != hipSuccess) {
        spl_ctx_destroy(c);
        return fail(SPL_E_HIP, "hipMalloc of constant tables failed");
    }
    // the fault word: host memory the kernels write through to (fine-grained), so the host reads a
    // launch's fault without synchronising the stream
    if (hipHostMalloc(reinterpret_cast<void **>(&c->fault_host), sizeof(uint64_t),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&c->fault_dev), c->fault_host, 0) != hipSuccess) {
        spl_ctx_destroy(c);
        return fail(SPL_E_HIP, "hipHostMalloc of the fault word failed");
    }
    *c->fault_host = 0;
    HIP_TRY(hipMemcpy(c->cards, crec.data(), sizeof(uint4) * 90, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->nobles, nrec.data(), sizeof(uint2) * 10, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_build_lut, dim3(blocks_for(kLutEntries)), dim3(64), 0, 0, c->lut);
    if (int r = launch_check()) {
        spl_ctx_destroy(c);
        return r;
    }
    HIP_TRY(hipDeviceSynchronize());
    *out = c;
    return SPL_OK;
}

int spl_ctx_destroy(spl_ctx_t *ctx) {
    if (!ctx) return SPL_OK;
    if (ctx->cards) (void)hipFree(ctx->cards);
    if (ctx->nobles) (void)hipFree(ctx->nobles);
    if (ctx->lut) (void)hipFree(ctx->lut);
    if (ctx->stage) (void)hipFree(ctx->stage);
    if (ctx->fault_host) (void)hipHostFree(ctx->fault_host);
    delete ctx;
    return SPL_OK;
}

int spl_ctx_faults(spl_ctx_t *ctx, uint64_t *launch, int clear) {
    if (!ctx || !launch) return fail(SPL_E_ARG, "null argument");
    volatile uint64_t *w = ctx->fault_host;
    *launch = *w;
    if (clear) *w = 0;
    return SPL_OK;
}

const volatile uint64_t *spl_ctx_fault_word(spl_ctx_t *ctx) {
    if (!ctx) {
        fail(SPL_E_ARG, "null ctx");
        return nullptr;
    }
    return ctx->fault_host;
}

uint64_t spl_ctx_launches(spl_ctx_t *ctx) { return ctx ? ctx->launches : 0; }

int spl_host_mapped(const void *host, int32_t *same_address) {
    if (!host || !same_address) return fail(SPL_E_ARG, "null argument");
    void *dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, const_cast<void *>(host), 0);
    *same_address = (e == hipSuccess && dev == host) ? 1 : 0;
    if (e != hipSuccess) (void)hipGetLastError();  // not page-locked by HIP: not an error of this call
    return SPL_OK;
}

int spl_ctx_set_refill_period(spl_ctx_t *ctx, int period) {
    if (!ctx || period < 0) return fail(SPL_E_ARG, "bad refill period");
    ctx->refill_period = period;
    return SPL_OK;
}

int spl_ctx_set_rollout_pipeline(spl_ctx_t *ctx, int on) {
    if (!ctx) return fail(SPL_E_ARG, "null ctx");
    if (on < 0 || on > 6) return fail(SPL_E_ARG, "rollout pipeline must be 0..6");
    ctx->pipeline = on;
    return SPL_OK;
}

int spl_ctx_set_step_tail(spl_ctx_t *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 2) return fail(SPL_E_ARG, "step shape must be -1 (auto), 0, 1 or 2");
    ctx->step_tail = mode;
    return SPL_OK;
}

int spl_ctx_set_partner_lead(spl_ctx_t *ctx, int lead) {
    if (!ctx || lead < -1 || lead > 64) return fail(SPL_E_ARG, "partner lead must be in [-1, 64]");
    ctx->partner_lead = lead;
    return SPL_OK;
}

int spl_debug_partner_stats(uint64_t *stats, int clear) {
    if (!stats) return fail(SPL_E_ARG, "stats must be non-null");
    unsigned long long v[2] = {0ull, 0ull};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_partner_stats), sizeof(v)));
    stats[0] = v[0];
    stats[1] = v[1];
    if (clear) {
        const unsigned long long z[2] = {0ull, 0ull};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_partner_stats), z, sizeof(z)));
    }
    return SPL_OK;
}

int spl_ctx_set_rollout_delegation(spl_ctx_t *ctx, int every) {
    if (!ctx || every < 0 || (every > 0 && every < 4)) return fail(SPL_E_ARG, "delegation period must be 0 or >= 4");
    ctx->deleg_every = every;
    return SPL_OK;
}

int spl_ctx_set_refill_fused(spl_ctx_t *ctx, int fused) {
    if (!ctx) return fail(SPL_E_ARG, "null ctx");
    ctx->refill_fused = fused != 0;
    return SPL_OK;
}

int64_t spl_ctx_token_lut(spl_ctx_t *ctx, uint32_t *out, int64_t words) {
    const int64_t need = (int64_t)kLutEntries * 4;
    if (!ctx) return fail(SPL_E_ARG, "null context");
    if (!out) return need;
    if (words < need) return fail(SPL_E_ARG, "output too small");
    HIP_TRY(hipMemcpy(out, ctx->lut, need * 4, hipMemcpyDeviceToHost));
    return need;
}

#define DISPATCH_P(P_, call)                        \
    switch (P_) {                                   \
        case 2: { constexpr int PP = 2; call; } break; \
        case 3: { constexpr int PP = 3; call; } break; \
        case 4: { constexpr int PP = 4; call; } break; \
        default: return fail(SPL_E_ARG, "players must be 2..4"); \
    }

int spl_reset(spl_ctx_t *ctx, spl_arena_t *arena, const uint64_t *pcg, const uint8_t *reset_mask, int32_t *obs,
              int8_t *mask, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (obs && ((uintptr_t)obs & 15u)) return fail(SPL_E_ARG, "obs must be 16-byte aligned");
    if (mask && ((uintptr_t)mask & 3u)) return fail(SPL_E_ARG, "mask must be 4-byte aligned");
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_reset<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A,
                                                  ktables(ctx), pcg, reset_mask, obs, mask, (const uint32_t *)nullptr));
    if (int r = launch_check()) return r;
    arena->steps = 0;
    return SPL_OK;
}

int spl_deal(spl_ctx_t *ctx, spl_arena_t *arena, const uint32_t *engine_seeds, const uint8_t *deal_mask,
             int32_t *obs, int8_t *mask, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!engine_seeds) return fail(SPL_E_ARG, "engine_seeds is required");
    if (obs && ((uintptr_t)obs & 15u)) return fail(SPL_E_ARG, "obs must be 16-byte aligned");
    if (mask && ((uintptr_t)mask & 3u)) return fail(SPL_E_ARG, "mask must be 4-byte aligned");
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_reset<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A,
                                                  ktables(ctx), (const uint64_t *)nullptr, deal_mask, obs, mask,
                                                  engine_seeds));
    return launch_check();
}

int spl_arena_init(spl_ctx_t *ctx, spl_arena_t *arena, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(arena->base, 0, (size_t)spl_arena_bytes(arena->n, arena->players), s));
    // no pool deal yet: a reset() without seed deals inline, the refill kernel deals it
    const KArena A = karena(arena);
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(A.planes + (size_t)SW_MISC * arena->n),
                              (int)((uint32_t)(kSlotRecords - 1) << ST_PEND_SHIFT),
                              (size_t)arena->n, s));
    arena->steps = 0;
    arena->epoch = 0;
    return SPL_OK;
}

int spl_refill(spl_ctx_t *ctx, spl_arena_t *arena, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_refill<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A));
    if (int r = launch_check()) return r;
    arena->epoch += 1;
    return SPL_OK;
}

static int check_step_args(const spl_step_args_t *a) {
    if (!a || !a->actions || !(a->obs || a->obs_u8) || !a->mask || !a->reward || !a->terminated || !a->flags)
        return fail(SPL_E_ARG, "actions/obs/mask/reward/terminated/flags are required");
    if ((uintptr_t)a->obs_u8 & 15u) return fail(SPL_E_ARG, "obs_u8 must be 16-byte aligned");
    if (!a->gate_terminated != !a->gate_flags) return fail(SPL_E_ARG, "gate_terminated and gate_flags go together");
    if (a->autoreset < 0 || a->autoreset > 2) return fail(SPL_E_ARG, "autoreset must be 0, 1 or 2");
    if (a->policy < SPL_POLICY_UNIFORM || a->policy > SPL_POLICY_BASIC_PRIORITY) return fail(SPL_E_ARG, "unknown policy");
    if (((uintptr_t)a->obs & 15u) || (a->final_obs && ((uintptr_t)a->final_obs & 3u)))
        return fail(SPL_E_ARG, "obs must be 16-byte aligned");
    if ((uintptr_t)a->mask & 3u) return fail(SPL_E_ARG, "mask must be 4-byte aligned");
    return SPL_OK;
}

static KStep kstep(spl_ctx_t *ctx, const spl_step_args_t *a) {
    KStep S;
    S.fault = ctx->fault_dev;
    S.fault_tag = ++ctx->launches;
    S.actions = a->actions;
    S.obs = a->obs;
    S.mask = a->mask;
    S.reward = a->reward;
    S.terminated = a->terminated;
    S.flags = a->flags;
    S.winner = a->winner;
    S.final_obs = a->final_obs;
    S.next_actions = a->next_actions;
    S.ep_return = a->ep_return;
    S.ep_count = a->ep_count;
    S.info = a->info;
    S.obs_u8 = a->obs_u8;
    S.gate_terminated = a->gate_terminated;
    S.gate_flags = a->gate_flags;
    S.errors = reinterpret_cast<unsigned long long *>(a->errors);
    S.ply_base = a->ply_base;
    S.policy_seed = a->policy_seed;
    S.ply = a->ply;
    S.table0 = a->table0;
    S.autoreset = a->autoreset;
    S.policy = a->policy;
    return S;
}

int spl_step(spl_ctx_t *ctx, spl_arena_t *arena, const spl_step_args_t *a, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (int r = check_step_args(a)) return r;
    const KStep S = kstep(ctx, a);
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned blocks = blocks_for(arena->n);
    // auto: the tail wave up to three workgroups per CU, and for compact-only outputs (obs_u8 without the
    // int32 rows: a quarter of the row stores, so the rules wave's tail is the longer one)
    const int shape = ctx->step_tail >= 0 ? ctx->step_tail
                                          : (((int64_t)blocks <= ctx->step_tail_blocks || a->obs == nullptr) ? 1 : 0);
    const StepKernel &k = kStepKernels[shape * 3 + arena->players - 2];
    hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(k.threads), 0, s, A, ktables(ctx), S);
    if (int r = launch_check()) return r;
    arena->steps += 1;
    if (a->autoreset && ctx->refill_period > 0 && arena->steps % ctx->refill_period == 0)
        return spl_refill(ctx, arena, stream);
    return SPL_OK;
}

// whether every workgroup of the shape's grid over n tables is resident at once
static bool rollout_fits(const spl_ctx_t *ctx, int shape, int32_t n, int32_t players) {
    const int tpw = rollout_kernel(shape, true, players).tpw;
    return ((int64_t)n + tpw - 1) / tpw <= ctx->resident[shape][players];
}

// The rollout kernel shape (0 the one-wave k_rollout, 2-6 see SPL_ROLLOUT_KERNELS).  Auto (pipeline 1):
// the six-wave dealer variant when every 128-table workgroup is resident at once (one
// per CU, e.g. C4's 32 768 tables per GPU: 1 120-1 137 against 1 166-1 172 us per 128-step launch
// for the three-wave one, alternating on one box, profiles/r04/c4ab_r04b.txt), else the three-wave
// one when it fits, else (2 players) the quad kernel when every 256-table workgroup is resident, else
// two waves at 64 tables per workgroup.
static int rollout_shape(const spl_ctx_t *ctx, int32_t n, int32_t players) {
    if (ctx->pipeline != 1) return ctx->pipeline;
    // auto: the six-wave dealer (SIMD-aware roles, -3.5 % on C4's share), else three-wave
    if (rollout_fits(ctx, 5, n, players)) return 5;
    if (rollout_fits(ctx, 4, n, players)) return 4;
    // 2 players up to one quad workgroup per CU (the headline's 65 536 tables): the quad kernel with its
    // partner hand-off, 1 959-1 983 against 2 008-2 031 us per 128-step launch for the two-wave kernel,
    // alternating on one box (profiles/r05/headline_quad_ab_r05h.txt); 3-4 players keep the two-wave
    if (players == 2 && rollout_fits(ctx, 6, n, players)) return 6;
    return 2;
}

const char *spl_rollout_kernel_name(spl_ctx_t *ctx, int32_t n, int32_t players, int32_t per_step_outputs) {
    static const char *const one_wave[3] = {"k_rollout<2>", "k_rollout<3>", "k_rollout<4>"};
    if (!ctx || n <= 0 || players < 2 || players > 4) {
        fail(SPL_E_ARG, "spl_rollout_kernel_name: bad arguments");
        return nullptr;
    }
    const int shape = rollout_shape(ctx, n, players);
    return shape == 0 ? one_wave[players - 2] : rollout_kernel(shape, per_step_outputs != 0, players).name;
}

int spl_rollout(spl_ctx_t *ctx, spl_arena_t *arena, const spl_step_args_t *a, int32_t steps, int32_t per_step_outputs,
                void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (int r = check_step_args(a)) return r;
    if (!a->obs) return fail(SPL_E_ARG, "spl_rollout writes int32 obs (obs_u8 is spl_step only)");
    if (a->gate_terminated || a->gate_flags) return fail(SPL_E_ARG, "the gate is spl_step only");
    if (steps < 1) return fail(SPL_E_ARG, "spl_rollout: steps must be >= 1");
    if (per_step_outputs && (arena->n & 3))
        return fail(SPL_E_ARG, "spl_rollout: per-step outputs need a table count divisible by 4 (16-byte obs blocks)");
    const KStep S = kstep(ctx, a);
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t before = arena->steps;
    const bool due = a->autoreset && ctx->refill_period > 0 &&
                     (before + steps) / ctx->refill_period != before / ctx->refill_period;
    // fused: every refill the launch is due (one per refill period it crosses) runs inside it
    const int fused = (due && ctx->refill_fused)
                          ? (int)std::min<int64_t>(steps, (before + steps) / ctx->refill_period - before / ctx->refill_period)
                          : 0;
    const int shape = rollout_shape(ctx, arena->n, arena->players);
    if (shape == 0) {
        DISPATCH_P(arena->players, hipLaunchKernelGGL(k_rollout<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A,
                                                      ktables(ctx), S, (int)steps, (int)(per_step_outputs != 0), fused));
    } else {
        const RolloutKernel &k = rollout_kernel(shape, per_step_outputs != 0, arena->players);
        // delegation / partner pairs must run at the same time: off when the grid exceeds what is resident
        // at once (pipeline "dealer2" forced on a larger grid).  The delegation period is >= 4 or 0.
        int extra = 0;
        if (k.extra != kExtraNone && rollout_fits(ctx, shape, arena->n, arena->players))
            extra = k.extra == kExtraLead ? ctx->partner_lead : ctx->deleg_every;
        hipLaunchKernelGGL(k.fn, dim3((unsigned)((arena->n + k.tpw - 1) / k.tpw)), dim3(k.threads), 0, s, A, ktables(ctx), S,
                           (int)steps, fused, extra);
    }
    if (int r = launch_check()) return r;
    arena->steps += steps;
    if (fused) arena->epoch += fused;
    else if (due) return spl_refill(ctx, arena, stream);
    return SPL_OK;
}

int spl_encode(spl_ctx_t *ctx, spl_arena_t *arena, int32_t *obs, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!obs || ((uintptr_t)obs & 15u)) return fail(SPL_E_ARG, "obs must be non-null and 16-byte aligned");
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_observe<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A,
                                                  ktables(ctx), obs, (int8_t *)nullptr));
    return launch_check();
}

int spl_legal(spl_ctx_t *ctx, spl_arena_t *arena, int8_t *mask, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!mask || ((uintptr_t)mask & 3u)) return fail(SPL_E_ARG, "mask must be non-null and 4-byte aligned");
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_observe<PP>, dim3(blocks_for(arena->n)), dim3(64), 0, s, A,
                                                  ktables(ctx), (int32_t *)nullptr, mask));
    return launch_check();
}

int spl_sample_uniform(spl_ctx_t *ctx, int32_t n, const int8_t *mask, int32_t *actions, uint64_t seed, uint64_t ply,
                       int64_t table0, void *stream) {
    if (!ctx || n <= 0 || !mask || !actions) return fail(SPL_E_ARG, "bad sample arguments");
    hipLaunchKernelGGL(k_sample, dim3(blocks_for(n)), dim3(64), 0, static_cast<hipStream_t>(stream), n, mask, actions,
                       seed, ply, table0);
    return launch_check();
}

int spl_step_info(int32_t n, const uint8_t *flags, uint8_t *info, uint64_t *errors, void *stream) {
    if (n <= 0 || !flags || !info || !errors || ((uintptr_t)errors & 7u)) return fail(SPL_E_ARG, "bad step-info arguments");
    hipLaunchKernelGGL(k_step_info, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n,
                       flags, info, reinterpret_cast<unsigned long long *>(errors));
    return launch_check();
}

static int ensure_stage(spl_ctx_t *ctx, size_t bytes) {
    if (ctx->stage_bytes >= bytes) return SPL_OK;
    if (ctx->stage) (void)hipFree(ctx->stage);
    ctx->stage = nullptr;
    ctx->stage_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->stage, bytes));
    ctx->stage_bytes = bytes;
    return SPL_OK;
}

int spl_table_download(spl_ctx_t *ctx, spl_arena_t *arena, int32_t first, int32_t count, spl_table_t *host,
                       void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!host || first < 0 || count <= 0 || first + count > arena->n) return fail(SPL_E_ARG, "bad download range");
    if (int r = ensure_stage(ctx, sizeof(spl_table_t) * (size_t)count)) return r;
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    spl_table_t *st = static_cast<spl_table_t *>(ctx->stage);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_download<PP>, dim3(blocks_for(count)), dim3(64), 0, s, A, first, count, st));
    if (int r = launch_check()) return r;
    HIP_TRY(hipMemcpyAsync(host, st, sizeof(spl_table_t) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SPL_OK;
}

static int validate_view(const spl_table_t &v, int P) {
    if (v.num_players != P) return fail(SPL_E_RANGE, "num_players does not match the arena");
    for (int c = 0; c < 6; ++c)
        if (v.bank[c] < 0 || v.bank[c] > 255) return fail(SPL_E_RANGE, "bank out of range");
    int owned = 0;
    for (int q = 0; q < P; ++q) {
        const spl_player_t &p = v.players[q];
        for (int c = 0; c < 6; ++c)
            if (p.tokens[c] < 0 || p.tokens[c] > 255) return fail(SPL_E_RANGE, "tokens out of range");
        for (int c = 0; c < 5; ++c)
            if (p.bonuses[c] < 0 || p.bonuses[c] > 255) return fail(SPL_E_RANGE, "bonuses out of range");
        if (p.prestige < 0 || p.prestige > 255) return fail(SPL_E_RANGE, "prestige out of range");
        if (p.n_reserved < 0 || p.n_reserved > 3) return fail(SPL_E_RANGE, "n_reserved out of range");
        for (int k = 0; k < p.n_reserved; ++k)
            if (p.reserved[k] < 0 || p.reserved[k] >= 90) return fail(SPL_E_RANGE, "reserved card id out of range");
        if (p.n_nobles < 0 || p.n_nobles > 5) return fail(SPL_E_RANGE, "player nobles out of range");
        for (int k = 0; k < p.n_nobles; ++k)
            if (p.nobles[k] < 0 || p.nobles[k] >= 10) return fail(SPL_E_RANGE, "player noble id out of range");
        owned += p.n_nobles;
    }
    for (int k = 0; k < 12; ++k)
        if (v.board[k] < -1 || v.board[k] >= 90) return fail(SPL_E_RANGE, "board card id out of range");
    for (int t = 0; t < 3; ++t) {
        if (v.deck_len[t] < 0 || v.deck_len[t] > tier_size(t)) return fail(SPL_E_RANGE, "deck too long for its record");
        for (int k = 0; k < v.deck_len[t]; ++k)
            if (v.decks[t][k] < 0 || v.decks[t][k] >= 90) return fail(SPL_E_RANGE, "deck card id out of range");
    }
    if (v.n_nobles < 0 || v.n_nobles > 5) return fail(SPL_E_RANGE, "visible noble slots out of range");
    int taken = 0;
    for (int s = 0; s < v.n_nobles; ++s) {
        if (v.nobles[s] >= 10 || v.nobles[s] < -1) return fail(SPL_E_RANGE, "noble id out of range");
        taken += v.nobles[s] < 0;
    }
    if (owned > taken) return fail(SPL_E_RANGE, "players hold more nobles than taken slots");
    if (v.to_play < 0 || v.to_play >= P) return fail(SPL_E_RANGE, "to_play out of range");
    if (v.turn_count < 0 || v.turn_count > 255) return fail(SPL_E_RANGE, "turn_count out of range");
    if (v.move_count < 0 || v.move_count > 508) return fail(SPL_E_RANGE, "move_count out of range (<= 508)");
    if (v.winner < -1 || v.winner >= P) return fail(SPL_E_RANGE, "winner out of range");
    return SPL_OK;
}

int spl_table_upload(spl_ctx_t *ctx, spl_arena_t *arena, int32_t first, int32_t count, const spl_table_t *host,
                     void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!host || first < 0 || count <= 0 || first + count > arena->n) return fail(SPL_E_ARG, "bad upload range");
    for (int i = 0; i < count; ++i)
        if (int r = validate_view(host[i], arena->players)) return r;
    if (int r = ensure_stage(ctx, sizeof(spl_table_t) * (size_t)count)) return r;
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    spl_table_t *st = static_cast<spl_table_t *>(ctx->stage);
    HIP_TRY(hipMemcpyAsync(st, host, sizeof(spl_table_t) * (size_t)count, hipMemcpyHostToDevice, s));
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_upload<PP>, dim3(blocks_for(count)), dim3(64), 0, s, A, first, count, st));
    if (int r = launch_check()) return r;
    HIP_TRY(hipStreamSynchronize(s));
    return SPL_OK;
}

int spl_search_abi_version(void) { return SPL_SEARCH_ABI; }

int spl_successors(spl_ctx_t *ctx, spl_arena_t *arena, const spl_succ_args_t *a, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!a) return fail(SPL_E_ARG, "null successor arguments");
    if (!a->obs && !a->obs_u8) return fail(SPL_E_ARG, "at least one of obs and obs_u8 must be given");
    if (!a->flags || !a->reward) return fail(SPL_E_ARG, "null buffer: flags and reward are required");
    if (spl_misaligned(a->obs, 16) || spl_misaligned(a->obs_u8, 16)) return fail(SPL_E_ARG, "obs and obs_u8 must be 16-byte aligned");
    if (spl_misaligned(a->reward, 4) || spl_misaligned(a->mask_bits, 8))
        return fail(SPL_E_ARG, "reward must be 4-byte aligned, mask_bits 8-byte aligned");
    const KArena A = karena(arena);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_successors<PP>, dim3(blocks_for(arena->n), SPL_NUM_ACTIONS), dim3(64), 0,
                                                  static_cast<hipStream_t>(stream), A, ktables(ctx), *a));
    return launch_check();
}

int spl_successors_pairs(spl_ctx_t *ctx, spl_arena_t *arena, const spl_succ_pairs_args_t *a, void *stream) {
    if (int r = check_arena(ctx, arena)) return r;
    if (!a) return fail(SPL_E_ARG, "null successor arguments");
    if (!a->obs_u8 || !a->flags || !a->reward || !a->pair || !a->legal || !a->base)
        return fail(SPL_E_ARG, "null buffer: obs_u8, flags, reward, pair, legal and base are required");
    if (spl_misaligned(a->obs_u8, 16)) return fail(SPL_E_ARG, "obs_u8 must be 16-byte aligned");
    if (spl_misaligned(a->reward, 4) || spl_misaligned(a->pair, 4) || spl_misaligned(a->base, 4) ||
        spl_misaligned(a->mask_bits, 8) || spl_misaligned(a->legal, 8))
        return fail(SPL_E_ARG, "reward, pair and base must be 4-byte aligned, mask_bits and legal 8-byte aligned");
    if (a->capacity < 1) return fail(SPL_E_ARG, "capacity must be positive");
    if ((int64_t)SPL_NUM_ACTIONS * arena->n > INT32_MAX) return fail(SPL_E_ARG, "45 n pair indices do not fit int32: too many tables");
    const KArena A = karena(arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned blocks = blocks_for(arena->n);
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_pairs_count<PP>, dim3(blocks), dim3(64), 0, s, A, ktables(ctx), a->legal, a->base));
    if (int r = launch_check()) return r;
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(kPairsScanThreads), 0, s, a->base, (int)blocks);
    if (int r = launch_check()) return r;
    DISPATCH_P(arena->players, hipLaunchKernelGGL(k_successors_pairs<PP>, dim3(blocks, SPL_NUM_ACTIONS), dim3(64), 0, s, A,
                                                  ktables(ctx), *a));
    return launch_check();
}

}  // extern "C"
