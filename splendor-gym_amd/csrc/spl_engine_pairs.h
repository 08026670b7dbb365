#pragma once
// spl_engine_pairs.h — the one-ply successors of the LEGAL pairs only (include/splendor_search.h
// spl_successors_pairs): about one (table, action) pair in six is legal, so the dense planes of spl_successors
// are mostly zero rows.  Three launches:
//   pairs_count_wave   one lane per table: legal_moves of its state into legal[t], the block's pair count
//   pairs_scan_block   the exclusive prefix of the block counts, in place, into base (one workgroup, a carry)
//   pairs_write_wave   one wave per (64-table block, action), as successors_wave: it leaves at once when no table of
//                      its block allows the action or its run does not fit under `capacity`; else the lanes with a
//                      legal pair step a register copy and their rows go out packed, at the run's offset
// The order of the pairs (by block, then action, then table) is the header's contract.  Nothing is written to the
// arena.
#include "../../include/splendor_search.h"
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_obs.h"
#include "spl_engine_deal.h"
#include "spl_engine_step.h"
#include "spl_engine_succ.h"
#include "spl_layout.h"

namespace spl {

constexpr int kPairsScanThreads = 1024;  // pairs_scan_block's workgroup: 65 536 tables are one chunk

// lanes below this one whose bit is set in `bal`
__device__ __forceinline__ int rank_in(uint64_t bal) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// legal[t] = legal_moves of table t's current state, evaluated here (the arena's legal-mask cache is not consulted,
// as in successors_wave), 0 for a table that is over; base[1 + block] = the block's number of legal pairs, which
// pairs_scan_block turns into the prefix.
template <int P>
__device__ __forceinline__ void pairs_count_wave(Consts &L, const KArena &A, const KTables &Tb, uint64_t *legal,
                                                 int32_t *base) {
    const int b = wg_block();
    const int t = b * 64 + lane_id();
    const bool in = t < A.n;
    load_tables_lds(L, Tb);
    Tab<P> T;
    if (in) load_tab(T, A, t);
    else fresh_state(T, 0u, empty_deal());
    wave_lds_sync();
    const uint64_t lg = (in && !is_terminal(T.sw)) ? legal_of(T, L) : 0ull;
    if (in) legal[t] = lg;
    int c = __popcll(lg);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane_id() == 0) base[1 + b] = c;
}

// base[0] = 0, base[1 + i] = count[0] + .. + count[i], the counts read from base[1 + i] itself: every element is
// read and written by the same thread, chunk after chunk with a carry, so the result does not depend on any order.
// One workgroup of kPairsScanThreads threads; wsum: 16 LDS words.
__device__ __forceinline__ void pairs_scan_block(int32_t *base, int nb, int32_t *wsum) {
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    constexpr int kWaves = kPairsScanThreads / 64;
    int carry = 0;
    if (tid == 0) base[0] = 0;
    for (int i0 = 0; i0 < nb; i0 += kPairsScanThreads) {
        const int i = i0 + tid;
        int v = i < nb ? base[1 + i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            v += lane >= o ? u : 0;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int s = wsum[w];
            before += w < wave ? s : 0;
            total += s;
        }
        if (i < nb) base[1 + i] = carry + before + v;
        carry += total;
        __syncthreads();  // wsum is read before the next chunk overwrites it
    }
}

// succ_encode_row_u8 of the `keep` lanes alone, lane's row at slot `rank`: the other lanes write nothing
template <int P>
__device__ __forceinline__ void pairs_encode_row_u8(const Tab<P> &T, uint8_t *rows_base, const Consts &L, bool keep,
                                                    int rank) {
    uint32_t R[76];
    build_row(T, L, R);
    R[74] = (R[74] & 0xFFu) | ((uint32_t)(get_moves(T.sw) >> 8) << 8);
    if (keep) {
        SPL_CHECK(rank >= 0 && rank < 64, BC_ROWS);
        uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsU8 * rank);
#pragma unroll
        for (int j = 0; j < 75; ++j) dst[j] = R[j];
    }
}

// `rows` staged compact rows -> dst, which is 4-byte aligned and 16-byte aligned only for one run offset in four:
// up to three head dwords, then 16-byte stores under cache policy CP, then the tail's dwords.  The LDS side is
// read dword by dword, so it needs no realignment.
template <int CP>
__device__ __forceinline__ void pairs_store_u8(const uint8_t *rows_lds, int rows, uint8_t *dst) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst);
    const int words = rows * (kObsU8 / 4);
    const int head = min(words, (int)(((16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u) >> 2));
    if (lane_id() < head) dst32[lane_id()] = src[lane_id()];
    const V4Sink<CP> out(dst32 + head);
    const int chunks = (words - head) >> 2;
    for (int c = lane_id(); c < chunks; c += 64) {
        const int w = head + 4 * c;
        const v4i v = {(int)src[w], (int)src[w + 1], (int)src[w + 2], (int)src[w + 3]};
        out.put(c, v);
    }
    for (int w = head + (chunks << 2) + lane_id(); w < words; w += 64) dst32[w] = src[w];
}

// The wave of 64-table block `wg_block()` and action `a` (wave-uniform, 0..44).  `legal` and `base` are complete
// (the two launches before this one, on the same stream).
template <int P>
__device__ __forceinline__ void pairs_write_wave(SuccLDS &L, const KArena &A, const KTables &Tb,
                                                 const spl_succ_pairs_args_t &S, int a) {
    const int lane = lane_id();
    const int b = wg_block();
    const int t = b * 64 + lane;
    const uint64_t lg = t < A.n ? S.legal[t] : 0ull;
    const bool ok = ((lg >> a) & 1ull) != 0ull;
    const uint64_t bal = __ballot(ok);
    if (bal == 0ull) return;  // nobody in this block may play a
    int off = S.base[b];
    for (int k = 0; k < a; ++k) off += __popcll(__ballot(((lg >> k) & 1ull) != 0ull));
    const int cnt = __popcll(bal);
    if (off + cnt > S.capacity) return;  // the run does not fit whole: none of it is written
    const int rank = rank_in(bal);
    SPL_CHECK(off >= 0 && (!ok || rank < cnt), BC_ROWS);
    load_tables_lds(L, Tb);
    Tab<P> T;
    if (ok) load_tab(T, A, t);
    else fresh_state(T, 0u, empty_deal());
    wave_lds_sync();
    const int ptier = pop_tier(a);
    const bool drew = ok && ptier >= 0 && bget(T.sw[SW_DECK], ptier) > 0u;
    const StepPre pre = step_prefetch(T, a, ok, A, t, Tb);
    const StepOut o = step_rules(T, a, pre, ok, L, Tb, L.mtx, true, 1ull << a);
    wave_lds_sync();
    pairs_encode_row_u8(T, L.rows, L, ok, rank);
    wave_lds_sync();
    pairs_store_u8<kSuccCpol>(L.rows, cnt, S.obs_u8 + (size_t)off * kObsU8);
    if (ok) {
        const int i = off + rank;
        SPL_CHECK(i < S.capacity, BC_ROWS);
        const uint32_t f = (uint32_t)SPL_SUCC_LEGAL | (o.term ? (uint32_t)SPL_SUCC_TERMINATED : 0u) |
                           ((o.flags & SPL_F_TURN_LIMIT) ? (uint32_t)SPL_SUCC_TURN_LIMIT : 0u) |
                           (drew ? (uint32_t)SPL_SUCC_DREW : 0u);
        S.flags[i] = (uint8_t)f;
        S.reward[i] = o.reward;
        S.pair[i] = a * A.n + t;
        if (S.mask_bits) S.mask_bits[i] = o.mask;
        if (S.winner) S.winner[i] = (int8_t)get_winner(T.sw);
    }
}

}  // namespace spl
