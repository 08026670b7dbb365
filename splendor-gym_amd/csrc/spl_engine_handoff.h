#pragma once
// spl_engine_handoff.h — the rollouts' hand-offs between workgroups and waves: rollout-store delegation to the
// partner workgroup on the neighbouring XCC (Deleg, deleg_*, flag_*, stage_state ...), the dealer wave that deals
// the pool refills beside the rules wave (DealerLDS, WsDealLDS, lds_*, deal_of_lds) and the partner hand-off of the
// multi-team kernels (PartnerLink, pt_*, dealer_loop, dealer_post, dealer_step), with g_partner_stats.
#include "../../include/splendor_amd.h"
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_obs.h"
#include "spl_engine_deal.h"
#include "spl_engine_step.h"
#include "spl_engine_ws.h"
#include "spl_layout.h"

namespace spl {

// Rollout-store delegation (rollout_ws<P, 64, true>, spl_ctx_set_rollout_delegation).  The
// XCCs of an MI355X do not drain stores equally fast: with the rollout store's own write pattern
// and nothing else running (tools/microbench_store_xcc.hip), workgroups on odd XCCs (odd blockIdx)
// finish ~20 % after those on even XCCs, whichever addresses they write; in the kernel the slowest
// XCC sets the launch time.  So workgroups pair up (2q on an even XCC, 2q+1 on the odd one next to
// it), and on every `every`-th step the odd one stages its 64 tables' state words after the step
// (4.3 KB at 2 players, against the 76 KB block it would store; it skips that step's encode) and
// its even partner, done with its own steps first, encodes and stores the rows into the rollout
// store (staging the encoded rows as bytes, 19 KB a block, measured ~1 % slower and moved 0.06 GB
// more per launch).  Cross-XCC hand-off (the guide's valid form):
// payload stored sc1 (write-through), the ready flag stored sc1 only after the payload has
// completed, the consumer polls sc1 and loads the payload sc1 behind an agent-scope acquire.
// Nothing waits unboundedly: a consumer that does not see a task within its time limit gives up,
// and the producer stores every task whose `taken` flag it does not see itself (a row stored
// twice is the same row).  Launch epochs live in the arena (each side counts its own launches),
// so flags from earlier launches, graph replays included, never match.
struct Deleg {
    bool on, producer;
    int every;
    uint32_t epoch;
    uint32_t *fl;      // the pair's flag lines
    uint8_t *pay;      // the pair's payload slots
    int pend, pend_k;  // producer: task staged at step pend_k, ready flag not yet set
    uint32_t staged;   // producer: tasks staged (not stored here)
    __device__ __forceinline__ uint32_t *ready_flag(int j) const { return fl + (DF_TASKS + 2 * j) * kFlagLine; }
    __device__ __forceinline__ uint32_t *taken_flag(int j) const { return fl + (DF_TASKS + 2 * j + 1) * kFlagLine; }
    __device__ __forceinline__ uint8_t *slot(int j) const { return pay + (size_t)j * kDelegPayload; }
};
__device__ __forceinline__ bool deleg_step(int k, int K, int every) {
    return every > 0 && k % every == every / 2 - 1 && k + 2 < K && k / every < kDelegTasks;
}
// the shortest period that delegates at all; from it on the workgroups take their tables by the identity
// map (delegation pairs blockIdx b and b + 1 on adjacent XCCs)
__device__ __forceinline__ bool deleg_period(int every) { return every >= 4; }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, 0x7FFFFFF0, 0x00020000);
}
constexpr int kSc1 = 16;  // buffer-op aux bit: sc1 (write-through store / L1-bypassing load)
// a flag poll: relaxed agent-scope atomic load = global_load_dword sc1 (MI355X_MICROARCH.md: L1
// bypassed, L2-served), the poll form of the guide's hand-off rows
__device__ __forceinline__ uint32_t flag_load(const uint32_t *f) {
    return __hip_atomic_load(const_cast<uint32_t *>(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void flag_store(uint32_t *f, uint32_t v) {  // lane 0 only
    if (lane_id() == 0) __builtin_amdgcn_raw_buffer_store_b32(v, rsrc_of(f), 0, 0, kSc1);
}
// a delegated step: the wave's 64 tables' state words after the step -> a delegation slot
// ([word][lane], 256 contiguous bytes per word), sc1 (write-through) dword stores: relaxed agent-scope
// atomic stores = global_store_dword sc1; slots are 128-byte aligned (kDelegPayload = 50 lines), so each
// 128-byte line is written whole by one store instruction of this wave (the guide's row 3 store cell)
template <int P>
__device__ __forceinline__ void stage_state(const Tab<P> &T, uint8_t *slot) {
    uint32_t *const base = reinterpret_cast<uint32_t *>(slot);
#pragma unroll
    for (int w = 0; w < num_words(P); ++w)
        __hip_atomic_store(base + w * 64 + lane_id(), tab_word(T, w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static_assert(kDelegPayload % 128 == 0, "partner / delegation slots stay 128-byte aligned");
// a delegation slot -> the staged tables' state (sc1 loads)
template <int P>
__device__ __forceinline__ void unstage_state(const uint8_t *slot, Tab<P> &T) {
    const __amdgpu_buffer_rsrc_t r = rsrc_of(slot);
    uint32_t v[num_words(P)];
#pragma unroll
    for (int w = 0; w < num_words(P); ++w)
        v[w] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, (w * 64 + lane_id()) * 4, 0, kSc1);
#pragma unroll
    for (int w = 0; w < num_words(P); ++w) set_tab_word(T, w, v[w]);
}
// one staged task's rows (delegation or partner hand-off): the staged words -> rows in LDS -> the row
// block (whole wave, 64 full rows)
template <int P>
__device__ __forceinline__ void store_staged_task(const uint8_t *slot, uint8_t *rows_lds, const Consts &C, int32_t *dst) {
    Tab<P> T;
    unstage_state(slot, T);
    encode_row(T, rows_lds, C);
    wave_lds_sync();
    store_obs_block<64, true>(rows_lds, 64, dst);
    wave_lds_sync();  // the block's LDS reads are done before the next task's rows land
}
// the output wave opens the launch: both workgroups of a full pair take part (the same test on both
// sides), each counting its own launches
__device__ __forceinline__ Deleg deleg_open(const KArena &A, int every) {
    const size_t pair = blockIdx.x >> 1;
    Deleg dl{false, false, every, 0u, A.dflags + pair * kDelegFlagWords, A.deleg + pair * kDelegTasks * kDelegPayload,
             -1, -1, 0u};
    if (deleg_period(every) && (int)(blockIdx.x | 1u) * 64 + 64 <= A.n) {
        dl.on = true;
        dl.producer = (blockIdx.x & 1u) != 0;
        uint32_t *ep = dl.fl + (dl.producer ? DF_PROD_EPOCH : DF_CONS_EPOCH) * kFlagLine;
        dl.epoch = __builtin_amdgcn_readfirstlane(flag_load(ep)) + 1u;
        flag_store(ep, dl.epoch);
    }
    return dl;
}
// producer, at a delegated step k: the tables' words go to the step's slot; a step with a patched row
// (`big_moves`; its rows are encoded in `rows_lds`) is stored here and the partner skips the task
template <int P>
__device__ __forceinline__ void deleg_stage(Deleg &dl, const Tab<P> &T, int k, bool big_moves, const uint8_t *rows_lds,
                                            int32_t *dst) {
    const int j = k / dl.every;
    if (big_moves) {
        store_obs_block<64, true>(rows_lds, 64, dst);
        flag_store(dl.ready_flag(j), dl.epoch << 1 | 1u);
    } else {
        stage_state(T, dl.slot(j));
        dl.staged |= 1u << j;
        dl.pend = j;
        dl.pend_k = k;
    }
}
// producer, at the end of every step: the task staged two steps ago turns ready
__device__ __forceinline__ void deleg_release(Deleg &dl, int k) {
    if (dl.pend >= 0 && k == dl.pend_k + 2) {
        // release (guide rule (2)): every sc1 store of the staged words has completed
        // before the ready flag is stored; by now two steps of block stores sit behind
        // them, so the wait also drains those
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        flag_store(dl.ready_flag(dl.pend), dl.epoch << 1);
        dl.pend = -1;
    }
}
// consumer, after its own steps: the partner's staged blocks, each as soon as its ready flag shows
template <int P>
__device__ __forceinline__ void deleg_consume(const Deleg &dl, int K, uint8_t *rows_lds, const Consts &C, int32_t *obs,
                                              int n) {
    const int64_t pt0 = (int64_t)(blockIdx.x + 1) * 64;
    const uint64_t limit = 200000;  // 2 ms of s_memrealtime (100 MHz) per task at most
    for (int k = 0; k < K; ++k) {
        if (!deleg_step(k, K, dl.every)) continue;
        const int j = k / dl.every;
        uint32_t f = 0;
        const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            f = __builtin_amdgcn_readfirstlane(flag_load(dl.ready_flag(j)));
            if ((f >> 1) == dl.epoch || __builtin_amdgcn_s_memrealtime() - t_start > limit) break;
            __builtin_amdgcn_s_sleep(8);
        }
        if ((f >> 1) != dl.epoch) break;  // not seen in time: the producer stores the rest
        if (f & 1u) continue;              // the producer stored it
        flag_store(dl.taken_flag(j), dl.epoch);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        store_staged_task<P>(dl.slot(j), rows_lds, C, obs + ((size_t)k * (size_t)n + pt0) * kObsDim);
    }
}
// producer, after its steps: every staged block whose taken flag is not visible is stored here
template <int P>
__device__ __forceinline__ void deleg_reclaim(const Deleg &dl, uint8_t *rows_lds, const Consts &C, int32_t *obs, int n,
                                              int t0) {
    for (int j = 0; j < kDelegTasks; ++j) {
        if (!((dl.staged >> j) & 1u)) continue;
        const int k = j * dl.every + dl.every / 2 - 1;
        if (__builtin_amdgcn_readfirstlane(flag_load(dl.taken_flag(j))) == dl.epoch) continue;
        store_staged_task<P>(dl.slot(j), rows_lds, C, obs + ((size_t)k * (size_t)n + t0) * kObsDim);
    }
}

// ---- the dealer wave (rollout for grids of at most two workgroups per CU) ----------------------
// A pool refill deal is a ~90 us serial integer chain per wave (MT19937 init, stream, Fisher-Yates).
// Fused into the rules wave it stalls that wave's steps for its whole length: at 4 players a
// 128-step launch needs ~8 of them per table, ~45 % of the rules wave's time on a half-full chip
// (C4's 32 768 tables per GPU).  When the grid leaves room for a third wave per workgroup (two
// workgroups of 64 tables per CU: 6 waves on 4 SIMDs), a DEALER wave deals instead, beside the
// rules and output waves:
//   * the rules wave owns the ring bookkeeping (status word: live record, pend = consumed records
//     not yet requested) and posts a batch -- one record per table, the earliest consumed one, the
//     next in the engine-seed stream -- whenever the dealer is idle and some table has pend > 0;
//   * the dealer owns the engine-seed streams (PCG64 records) and the deal scratch; it deals the
//     batch into the slot records (global) and the board / noble words into LDS, drains its stores
//     (s_waitcnt vmcnt(0): the waves of a workgroup share one L1, so that is the workgroup-scope
//     release), then counts the batch done;
//   * a table that ends while its next record is in flight waits for the batch; one whose pool is
//     spent (all three records consumed) posts a batch of its own and waits (the old inline deal).
// Deals are taken from each stream in episode order either way, so results do not depend on when
// a batch runs.  The three waves hand off through LDS counters (no s_barrier: the dealer cannot
// join a per-step barrier while it runs a 90 us deal).
struct DealerLDS {
    static constexpr int kStride = 100;  // deal scratch bytes per lane (25 dwords: odd, conflict-free)
    uint8_t scr[64 * kStride];
    uint32_t mtx[624];        // the dealer's LaneMT continuation (one lane at a time)
    uint32_t rdeal[5][64];    // board / noble words of the last batch's deals ([word][lane])
    uint8_t rq[64];           // slot record to deal per table, 0xFF = none
    uint32_t dreq, ddone;     // batches posted (rules wave) / dealt (dealer)
    uint32_t rdone, odone;    // steps handed off by the rules wave / finished by the output wave
    uint32_t stop;            // rules wave: no more batches
    uint32_t rnd[2][64];      // the uniform policy's words of step k in slot k & 1, drawn by the output wave at step k - 2
    uint32_t abort;           // a wait ran out (lds_wait_ge): every later wait returns at once
};
template <int P>
struct __align__(16) WsDealLDS : WsLDS<P> {
    static constexpr int kWaves = 3;  // rules + output + dealer
    DealerLDS dl;
};
static_assert(sizeof(WsDealLDS<2>) <= 81920 && sizeof(WsDealLDS<3>) <= 81920 && sizeof(WsDealLDS<4>) <= 81920,
              "the dealer rollout needs two workgroups per CU");

__device__ __forceinline__ uint32_t lds_poll(const uint32_t *p) {
    const uint32_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // later LDS reads stay below the poll
    return __builtin_amdgcn_readfirstlane(v);
}
// lane 0 publishes `v` after this wave's earlier LDS writes have landed
__device__ __forceinline__ void lds_publish(uint32_t *p, uint32_t v) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    if (lane_id() == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// Every wait is bounded (~2^22 polls, a fraction of a second; a legitimate wait is one deal, ~0.1 ms)
// so that a lost hand-off never leaves waves spinning on the GPU.  A wait that runs out FAULTS the
// workgroup, loudly, in every build (round 4; was a silent abort in the release library):
//   * it sets the workgroup's abort word, so every later wait of the three waves returns false at once;
//   * the rules wave stops stepping and leaves its tables' state unstored, the output wave stops storing
//     and marks SPL_F_FAULT in the flags of every step it did not store, the dealer stops dealing —
//     nothing reads or writes through an index taken from an unsettled hand-off;
//   * the launch's serial goes into the context's host-mapped fault word (signal_fault), which
//     spl_ctx_faults reads without synchronising (Engine / SplendorVectorEnv / bench.py raise on it).
// spl_debug_set_spin_limit lowers the limit so a test can force the path (BC_SPIN still marks it in
// the bounds-check build).
// true once *p >= v; false when the wait ran out or another wave of the workgroup already faulted
__device__ __forceinline__ bool lds_wait_ge(DealerLDS &D, const uint32_t *p, uint32_t v) {
    const uint32_t limit = g_spin_limit;
    for (uint32_t spins = 0; lds_poll(p) < v; ++spins) {
        if (spins >= limit || lds_poll(&D.abort)) {
            SPL_CHECK(false, BC_SPIN);
            if (lane_id() == 0) __hip_atomic_store(&D.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    return true;
}
__device__ __forceinline__ Deal deal_of_lds(const DealerLDS &D, int lane) {
    return Deal{{D.rdeal[0][lane], D.rdeal[1][lane], D.rdeal[2][lane]}, D.rdeal[3][lane], D.rdeal[4][lane]};
}

// ---- partner hand-off (six-wave dealer rollout, per-step outputs; ctx partner_lead) -------------
// Under the rollout store's write stream the XCCs do not keep the same pace: the C4 share's stamps put
// the teams of one or two XCCs 7-16 % behind the rest (their observation-row stores issue slower;
// without the row stores every XCC runs the same period, profiles/r04/wsstamps4_r04k.txt), and the
// launch ends with the slowest team.  So a team that falls behind hands whole steps of observation
// rows to the same team of the workgroup on the neighbouring XCC (blockIdx b ^ 1), whose OUTPUT wave
// encodes and stores them between its own steps:
//   * each side's output wave publishes its progress (steps done) every step and reads the partner's
//     from its dealer's snapshot; when the partner is `lead` or more steps ahead and the next task
//     slot is free (by a snapshot of that slot's flag), the step's state words go to the slot (sc1 stores, ~6 KB) instead of the encode
//     and the 76 KB row block, and the slot's flag turns READY(launch, step) after a vmcnt(0) at the
//     top of the next step (the guide's drained-sc1 hand-off: sc1 payload, vmcnt(0), sc1 flag);
//   * at the top of each step the partner's output wave looks at the snapshot of the next slot's flag
//     and takes at most one READY task: an agent-scope compare-and-swap READY -> TAKEN,
//     the words loaded sc1, encoded and stored, the slot freed; after its own steps it keeps serving
//     until the partner's DONE word shows (bounded by time: a partner that never finishes keeps its
//     tasks);
//   * at the end the producer posts DONE and claims back, by the same compare-and-swap, every task
//     still READY, and stores those rows itself: each task's rows are stored once, by its flag's winner.
// (The dealer wave as the consumer took too few tasks: a deal keeps it busy ~90 us at a time.  It does
// poll the pair's flag words for its output wave between batches (pt_poll: LDS snapshots tagged with
// the sequence numbers they are for), so that the output wave issues no global load it must wait for
// behind its own row stores in the one in-order vmcnt; polled by the output wave itself, the hand-off
// made every team slower than it won.)
// Masks, small outputs and terminal rows stay with the producer; rows are encoded by the same code
// from the same words, so results do not depend on who stores them.  Launch counters (one per side,
// in the arena, zeroed with it; both sides count the same launches) tag every flag, so nothing from
// an earlier launch or graph replay matches.
struct PartnerLink {
    bool on;
    int side, lead;    // lead < 0: hand off whenever a slot is free (tests)
    uint32_t e;        // this launch's counter value
    uint32_t *fl;      // the pair's flag lines
    uint8_t *pay;      // the pair's payload slots
    int t0p;           // the partner team's first table
    __device__ __forceinline__ uint32_t *line(int l) const { return fl + l * kFlagLine; }
    __device__ __forceinline__ uint8_t *slot(int j) const { return pay + (size_t)j * kDelegPayload; }
};
constexpr uint32_t kPtReady = 1u, kPtTaken = 2u;
constexpr uint64_t kPartnerWait = 500000;  // 5 ms of s_memrealtime (100 MHz): the consumer's wait for DONE
__device__ __forceinline__ uint32_t pt_flag(uint32_t e, int k, uint32_t st) { return e << 16 | (uint32_t)k << 2 | st; }
__device__ unsigned long long g_partner_stats[2];  // tasks stored by the partner / claimed back (diagnostics)

// READY(launch, step) posted by an agent-scope atomic add (the guide's row 3: "each storing wave for
// itself", after that wave's s_waitcnt vmcnt(0)).  `seen` is the producer's snapshot of the slot's flag
// when it chose the slot: 0 or a value of an earlier launch, which nobody else writes in this launch (the
// consumer writes only flags READY in this launch), so adding target - seen leaves exactly `target`.
__device__ __forceinline__ void pt_post_ready(uint32_t *f, uint32_t target, uint32_t seen) {
    if (lane_id() == 0) (void)__hip_atomic_fetch_add(f, target - seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The output wave's hand-off state: tasks posted (pseq) and the one staged but not yet READY (slot pend,
// step pend_k, pend_seen the slot's flag as the producer saw it, for pt_post_ready), partner tasks seen
// (cseq).  The flags and the partner's progress come from the poller's LDS snapshots.
struct PtOut {
    uint32_t pseq, cseq;
    int pend, pend_k;
    uint32_t pend_seen;
};
// the task staged last (if any): its words have completed, then READY
__device__ __forceinline__ void pt_ready_staged(const PartnerLink &pl, PtOut &po) {
    if (po.pend < 0) return;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    pt_post_ready(pl.line(pt_ready_line(po.pend)), pt_flag(pl.e, po.pend_k, kPtReady), po.pend_seen);
    po.pend = -1;
}
// lane 0 moves a task flag READY -> TAKEN (agent scope: performed past the XCC's L2); wave-uniform
__device__ __forceinline__ bool pt_claim(uint32_t *f, uint32_t ready) {
    uint32_t seen = 0u;
    if (lane_id() == 0) {
        seen = ready;
        __hip_atomic_compare_exchange_strong(f, &seen, (ready & ~3u) | kPtTaken, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane(seen) == ready;
}
// consumer (the partner team's output wave): `v` = the flag of the partner's slot cseq; if it is READY,
// claim it and store the task's rows (staged through `rows`); true if the slot held a task.  Which
// form makes the staged words visible (MI355X_MICROARCH.md, "Valid forms" / the hand-off table):
//   acquire = false: the quad kernel in its steps — the flag was polled by the rules wave (global_load_dword
//     sc1) before an s_barrier this wave has passed since (row 3: agent-atomic flag, barrier between the
//     poll and every load, sc1 global stores / buffer_load_dword sc1 loads, one workgroup per CU);
//   acquire = true: everywhere else (the six-wave dealer, whose poller is not separated from this wave by
//     a barrier, and every drain after the steps) — the consumer's "always" form: one poll, the claim,
//     ONE agent acquire, then the loads (this wave's own loads need no further wait).
template <int P>
__device__ __forceinline__ bool pt_serve_v(const PartnerLink &pl, uint32_t &cseq, uint32_t v, uint8_t *rows,
                                           const Consts &C, int32_t *obs, int n, bool acquire) {
    if ((v & 3u) != kPtReady || (v >> 16) != pl.e) return false;
    const int j = (pl.side ^ 1) * kPartnerSlots + (int)(cseq % kPartnerSlots);
    ++cseq;  // tasks fill the ring in order: the next one is in the next slot, whoever stores this one
    uint32_t *f = pl.line(pt_ready_line(j));
    if (!pt_claim(f, v)) return true;
    if (acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int k = (int)((v >> 2) & 0x3FFFu);
    store_staged_task<P>(pl.slot(j), rows, C, obs + ((size_t)k * (size_t)n + (size_t)pl.t0p) * kObsDim);
    // the slot's words were read (the encode used them) before it is free again; no vmcnt wait: the
    // rows' stores need not have completed
    __asm__ volatile("" ::: "memory");
    flag_store(f, 0u);
    if (lane_id() == 0) atomicAdd(&g_partner_stats[0], 1ull);
    return true;
}
__device__ __forceinline__ uint32_t pt_next_flag(const PartnerLink &pl, uint32_t cseq) {
    return flag_load(pl.line(pt_ready_line((pl.side ^ 1) * kPartnerSlots + (int)(cseq % kPartnerSlots))));
}
// consumer, after its own steps: serve until the partner's DONE word shows (or kPartnerWait passes)
template <int P>
__device__ __forceinline__ void pt_drain(const PartnerLink &pl, uint32_t &cseq, uint8_t *rows, const Consts &C,
                                         int32_t *obs, int n) {
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        if (pt_serve_v<P>(pl, cseq, (uint32_t)__builtin_amdgcn_readfirstlane(pt_next_flag(pl, cseq)), rows, C, obs, n,
                          true))
            continue;
        const uint32_t dn = (uint32_t)__builtin_amdgcn_readfirstlane(flag_load(pl.line(pt_done_line(pl.side ^ 1))));
        if (dn == pl.e) {  // its READY flags were stored before DONE: what is left of them, then out
            while (pt_serve_v<P>(pl, cseq, (uint32_t)__builtin_amdgcn_readfirstlane(pt_next_flag(pl, cseq)), rows, C,
                                 obs, n, true)) {
            }
            return;
        }
        if (__builtin_amdgcn_s_memrealtime() - t_start > kPartnerWait) return;
        __builtin_amdgcn_s_sleep(8);
    }
}
// producer, at the end of its steps — and on a fault of its workgroup: the task staged
// last (if any) turns READY, DONE is posted behind every READY flag (the partner's pt_drain stops
// waiting), then every task the partner has not taken is claimed back by the same compare-and-swap
// and its rows are stored here: each handed-off step's rows are stored once, whatever happened after
template <int P>
__device__ __forceinline__ void pt_close(const PartnerLink &pl, PtOut &po, uint8_t *rows, const Consts &C, int32_t *obs,
                                         int n, int t0) {
    pt_ready_staged(pl, po);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // every READY flag has completed before DONE
    flag_store(pl.line(pt_done_line(pl.side)), pl.e);
    if (po.pseq == 0u) return;
    uint32_t mine = 0u;  // lane j: slot j's flag (relaxed agent load: global_load sc1)
    if (lane_id() < kPartnerSlots)
        mine = __hip_atomic_load(pl.line(pt_ready_line(pl.side * kPartnerSlots + lane_id())), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
    uint64_t rm = __ballot(lane_id() < kPartnerSlots && (mine & 3u) == kPtReady && (mine >> 16) == pl.e);
    for (; rm; rm &= rm - 1) {
        const int j = __ffsll((unsigned long long)rm) - 1;
        const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
        uint32_t *f = pl.line(pt_ready_line(pl.side * kPartnerSlots + j));
        if (!pt_claim(f, vj)) continue;
        const int kk = (int)((vj >> 2) & 0x3FFFu);
        store_staged_task<P>(pl.slot(pl.side * kPartnerSlots + j), rows, C, obs + ((size_t)kk * (size_t)n + (size_t)t0) * kObsDim);
        if (lane_id() == 0) atomicAdd(&g_partner_stats[1], 1ull);
    }
}

// The poll of the pair's words for the output wave (a snapshot; tags say which slots), by the dealer
// wave between batches or by the quad kernel's rules wave.
// what a poller loads for its output wave: the partner's progress, this side's next slot's flag (slot
// of task ps) and the partner's next slot's flag (slot of task cs); the loads are not waited for here
struct PtPolled {
    uint32_t a, b, c, ps, cs;
};
__device__ __forceinline__ PtPolled pt_load(PtShared &X, const PartnerLink &pl) {
    PtPolled q;
    q.ps = lds_poll(&X.seq[0]);
    q.cs = lds_poll(&X.seq[1]);
    q.a = flag_load(pl.line(pt_progress_line(pl.side ^ 1)));
    q.b = flag_load(pl.line(pt_ready_line(pl.side * kPartnerSlots + (int)(q.ps % kPartnerSlots))));
    q.c = flag_load(pl.line(pt_ready_line((pl.side ^ 1) * kPartnerSlots + (int)(q.cs % kPartnerSlots))));
    return q;
}
// qpar >= 0: the consumer's entry by the polling step's parity (PtShared::qcons)
__device__ __forceinline__ void pt_publish(PtShared &X, const PtPolled &q, int qpar = -1) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane(q.a), b = (uint32_t)__builtin_amdgcn_readfirstlane(q.b),
                   c = (uint32_t)__builtin_amdgcn_readfirstlane(q.c);
    if (lane_id() == 0) {
        __hip_atomic_store(&X.in[0], (uint64_t)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&X.in[1], (uint64_t)q.ps << 32 | b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(qpar < 0 ? &X.in[2] : &X.qcons[qpar], (uint64_t)q.cs << 32 | c, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
__device__ __forceinline__ void pt_poll(PtShared &X, const PartnerLink &pl) { pt_publish(X, pt_load(X, pl)); }
// the quad kernel's poller, once per step of its rules wave (which issues no row stores): the words
// loaded last step go to the output wave's snapshots, then new loads
__device__ __forceinline__ void pt_poll_ahead(PtShared &X, const PartnerLink &pl, PtPolled &q, int k) {
    if (k > 0) pt_publish(X, q, k & 1);
    q = pt_load(X, pl);
}
__device__ __forceinline__ uint64_t lds_poll64(const uint64_t *p) {
    const uint64_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
}
// the output wave at the top of step k: the task staged last step turns READY, then at most one of the
// partner's tasks, between this team's steps (the poller's snapshot of its next slot, if it is for the
// task this wave expects).  The quad kernel reads the snapshot its rules wave published at step k - 1,
// before the s_barrier of step k - 1 that this wave has passed (PtShared::qcons); the six-wave dealer
// acquires instead.
template <int P, bool kDealer>
__device__ __forceinline__ void pt_step_top(const PartnerLink &pl, PtOut &po, PtShared &X, int k, uint8_t *rows,
                                            const Consts &C, int32_t *obs, int n) {
    pt_ready_staged(pl, po);
    const uint64_t nx = kDealer ? lds_poll64(&X.in[2]) : lds_poll64(&X.qcons[(k + 1) & 1]);
    if ((uint32_t)(nx >> 32) == po.cseq && pt_serve_v<P>(pl, po.cseq, (uint32_t)nx, rows, C, obs, n, kDealer) &&
        lane_id() == 0)
        __hip_atomic_store(&X.seq[1], po.cseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the output wave with step k's state: hand the step's rows to the partner if it is `lead` steps ahead and
// the next slot is free (or stale), by a snapshot taken for this very slot.  True: the words are staged
// (READY follows at the top of the next step, or in pt_close) and this wave skips the encode and the rows.
template <int P>
__device__ __forceinline__ bool pt_hand_off(const PartnerLink &pl, PtOut &po, PtShared &X, const Tab<P> &T, int k) {
    const uint32_t pp = (uint32_t)lds_poll64(&X.in[0]);
    const uint64_t ms = lds_poll64(&X.in[1]);
    const uint32_t sf = (uint32_t)ms;
    const bool ahead = pl.lead < 0 || ((pp >> 16) == pl.e && (int)(pp & 0xFFFFu) >= k + pl.lead);
    if (!(ahead && (uint32_t)(ms >> 32) == po.pseq && ((sf & 3u) == 0u || (sf >> 16) != pl.e))) return false;
    const int j = pl.side * kPartnerSlots + (int)(po.pseq % kPartnerSlots);
    stage_state(T, pl.slot(j));
    po.pend = j;
    po.pend_k = k;
    po.pend_seen = (uint32_t)__builtin_amdgcn_readfirstlane(sf);
    ++po.pseq;
    if (lane_id() == 0) __hip_atomic_store(&X.seq[0], po.pseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return true;
}

// The dealer wave: batches until the rules wave stops and none is left.  An idle wait that runs out
// ends the dealer quietly: a batch posted after that is never dealt, so the rules wave's wait for it
// runs out and faults the launch (lds_wait_ge).  A faulted workgroup's dealer ends after its batch.
template <int P>
__device__ __forceinline__ void dealer_loop(DealerLDS &D, const KArena &A, int t0, const PartnerLink &pl, PtShared &X) {
    const int lane = lane_id();
    const uint32_t limit = g_spin_limit;
    uint32_t done = 0;
    for (;;) {
        uint32_t req;
        for (uint32_t spins = 0;; ++spins) {
            if (lds_poll(&D.abort)) return;
            req = lds_poll(&D.dreq);
            if (req != done || lds_poll(&D.stop)) break;
            if (pl.on) pt_poll(X, pl);
            if (spins >= limit) {
                SPL_CHECK(false, BC_SPIN);
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
        if (req == done) break;  // stopped (or idle too long), nothing pending
        const int slot = D.rq[lane];
        const int t = t0 + lane;
        if (slot != 0xFF) {
            SPL_CHECK(t < A.n && slot < kSlotRecords, BC_TABLE);
            Deal d;
            deal_next<P>(A, t, slot, &D.scr[lane * DealerLDS::kStride], d, D.mtx);
            D.rdeal[0][lane] = d.board[0];
            D.rdeal[1][lane] = d.board[1];
            D.rdeal[2][lane] = d.board[2];
            D.rdeal[3][lane] = d.nob0;
            D.rdeal[4][lane] = d.nob1;
        }
        __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0): the records and engine-seed streams are written
        lds_publish(&D.ddone, ++done);
    }
}

// the rules wave posts a batch: lanes with `want` request slot record `slot` of their table
__device__ __forceinline__ void dealer_post(DealerLDS &D, bool want, int slot, uint32_t &my_req) {
    D.rq[lane_id()] = want ? (uint8_t)slot : (uint8_t)0xFF;
    lds_publish(&D.dreq, ++my_req);
}

// The rules wave's side of the dealer after step_rules (wave-uniform call): settle a finished
// batch, make sure every table that ended has its next record dealt (waiting for the batch in
// flight, or posting one for a spent pool), run the same-step autoreset (flip_to_pool without its
// inline deal), then post a new batch when the dealer is idle.  False: a wait for the dealer faulted
// (lds_wait_ge) and T / pool were left as they were, not filled from an unsettled batch.
template <int P>
__device__ __forceinline__ bool dealer_step(DealerLDS &D, Tab<P> &T, const KArena &A, int t, bool valid, bool ends,
                                            bool autoreset, Deal &pool, bool &pool_dirty, uint32_t &my_req,
                                            uint32_t &infl, bool &pool_stale, StepOut &o) {
    constexpr int kPools = kSlotRecords - 1;
    const int lane = lane_id();
    auto settle = [&]() {  // the last batch's records are dealt; its words fill a stale `pool`
        infl = 0u;
        if (pool_stale) {
            pool = deal_of_lds(D, lane);
            pool_stale = false;
            pool_dirty = true;
        }
    };
    bool idle = lds_poll(&D.ddone) == my_req;
    if (idle) settle();
    uint32_t misc = T.sw[SW_MISC];
    int pend = pend_of(misc);
    const int nxt = (active_of(misc) + 1) % kSlotRecords;
    const bool spent = ends && pend >= kPools;  // all three pool records consumed: deal the next now
    const bool blocked = ends && !spent && (((infl >> nxt) & 1u) != 0u || pool_stale);
    if (__any(spent || blocked)) {
        if (!idle) {
            if (!lds_wait_ge(D, &D.ddone, my_req)) return false;
            settle();
            idle = true;
        }
        if (__any(spent)) {
            dealer_post(D, spent, nxt, my_req);  // nxt is the earliest consumed record when pend == 3
            if (spent) {
                pend -= 1;
                misc = (misc & ~ST_PEND) | ((uint32_t)pend << ST_PEND_SHIFT);
                pool_stale = true;
            }
            if (!lds_wait_ge(D, &D.ddone, my_req)) return false;
            settle();
        }
    }
    if (ends) {  // flip_to_pool: the next record is dealt and `pool` holds its words
        const int pend2 = pend + 1;  // the old live record is consumed
        fresh_state(T, ring_bits(nxt, pend2), pool);
        if (pend2 < kPools) {
            const int nxt2 = (nxt + 1) % kSlotRecords;
            if ((infl >> nxt2) & 1u) pool_stale = true;  // in flight: its words come with the batch
            else pool = rec_deal(slot_rec(A, t, nxt2));
        }
        pool_dirty = true;
        o.flags |= SPL_F_RESET;
        o.mask = kFreshDealMask;
        misc = T.sw[SW_MISC];
        pend = pend2;
    } else {
        T.sw[SW_MISC] = misc;
    }
    const bool want = valid && autoreset && pend > 0;
    if (idle && __any(want)) {  // refill: every table's earliest consumed record, next in its stream
        const int slot = (active_of(misc) - pend + kSlotRecords) % kSlotRecords;
        dealer_post(D, want, slot, my_req);
        if (want) {
            T.sw[SW_MISC] = (misc & ~ST_PEND) | ((uint32_t)(pend - 1) << ST_PEND_SHIFT);
            infl = 1u << slot;
            if (pend == kPools) pool_stale = true;  // the next record itself is being dealt
        }
    }
    return true;
}

}  // namespace spl
