#pragma once
// spl_engine_succ.h — one-ply successors (include/splendor_search.h spl_successors): one wave takes 64 tables and
// ONE action a, steps a register copy of each table with it (step_prefetch, step_rules: the step kernels' own
// code) and stores the successor rows and small outputs of the pairs (t, a).  Nothing is written to the arena.
// `a` is wave-uniform, so the six branches of apply_action are scalar branches here.
#include "../../include/splendor_search.h"
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_engine_obs.h"
#include "spl_engine_deal.h"
#include "spl_engine_step.h"
#include "spl_layout.h"

namespace spl {

// One wave's staging: the constant tables, 64 rows (compact rows of 300 bytes, or the 297-byte staging of
// encode_row, whose last lane's trailing bytes stay inside the 300-byte block) and the token-return
// continuation's MT19937 state (LaneMT: one lane at a time).  23 KB, seven waves per CU; BlockLDS (the
// rollout's, 40 KB with its mask stream and terminal rows, three per CU) holds nothing else this kernel needs.
struct __align__(16) SuccLDS : Consts {
    alignas(16) uint8_t rows[64 * kObsU8];
    uint32_t mtx[624];
};

// Row store policy of spl_successors: plain stores, or the rollout's non-temporal stream (kRollCpol).  The rows
// are read back at once by the critic call behind them, so they should stay cache resident: see DESIGN.md §4.11
// for the A/B of the pair at 65 536 tables.
#ifndef SPL_SUCC_CPOL
#define SPL_SUCC_CPOL kPlainCpol
#endif
constexpr int kSuccCpol = SPL_SUCC_CPOL;

// encode_row / encode_row_u8<2> with the rows of lanes that are not `keep` written as zero bytes
template <int P>
__device__ __forceinline__ void succ_encode_row(const Tab<P> &T, uint8_t *rows_base, const Consts &L, bool keep) {
    uint32_t R[76];
    build_row(T, L, R);
#pragma unroll
    for (int j = 0; j < 76; ++j) R[j] = keep ? R[j] : 0u;
    R[74] |= (uint32_t)__shfl_down((int)R[0], 1) << 8;  // bytes 297..299: the next lane's row bytes 0..2
    const int lane = lane_id();
    const uint32_t o0 = (4u - ((uint32_t)lane & 3u)) & 3u;
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsDim * lane + o0);
#pragma unroll
    for (int j = 0; j < 74; ++j) dst[j] = __builtin_amdgcn_alignbyte(R[j + 1], R[j], o0);
    if (o0 == 0u) dst[74] = R[74];
}
template <int P>
__device__ __forceinline__ void succ_encode_row_u8(const Tab<P> &T, uint8_t *rows_base, const Consts &L, bool keep) {
    uint32_t R[76];
    build_row(T, L, R);
    R[74] = (R[74] & 0xFFu) | ((uint32_t)(get_moves(T.sw) >> 8) << 8);
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsU8 * lane_id());
#pragma unroll
    for (int j = 0; j < 75; ++j) dst[j] = keep ? R[j] : 0u;
}

// `rows` staged compact rows -> dst: 16-byte stores under cache policy CP when dst is 16-byte aligned (a table
// count divisible by 4 makes every block so), else dwords
template <int CP>
__device__ __forceinline__ void succ_store_u8(const uint8_t *rows_lds, int rows, uint8_t *dst) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    const int words = rows * (kObsU8 / 4);
    int w0 = 0;
    if (((uintptr_t)dst & 15u) == 0) {
        const V4Sink<CP> out(dst);
        const int chunks = words >> 2;
        for (int c = lane_id(); c < chunks; c += 64) {
            const v4i v = {(int)src[4 * c], (int)src[4 * c + 1], (int)src[4 * c + 2], (int)src[4 * c + 3]};
            out.put(c, v);
        }
        w0 = chunks << 2;
    }
    for (int w = w0 + lane_id(); w < words; w += 64) reinterpret_cast<uint32_t *>(dst)[w] = src[w];
}
// `rows` staged 297-byte rows -> int32 dst: store_obs_block when dst is 16-byte aligned, else dwords
template <int CP>
__device__ __forceinline__ void succ_store_obs(const uint8_t *rows_lds, int rows, int32_t *dst) {
    if (((uintptr_t)dst & 15u) == 0) {
        store_obs_block<64, false, CP>(rows_lds, rows, dst);
        return;
    }
    const int nbytes = rows * kObsDim;
    for (int b = lane_id(); b < nbytes; b += 64) dst[b] = (int32_t)rows_lds[b];
}

// The wave of 64-table block `wg_block()` and action `a` (wave-uniform, 0..44).  mtx: >= 624 LDS words.
template <int P, class LdsT>
__device__ __forceinline__ void successors_wave(LdsT &L, uint32_t *mtx, const KArena &A, const KTables &Tb,
                                                const spl_succ_args_t &S, int a) {
    const int lane = lane_id();
    const int t0 = wg_block() * 64;
    const int t = t0 + lane;
    const bool in = t < A.n;
    const int rows = min(64, A.n - t0);
    load_tables_lds(L, Tb);
    Tab<P> T;
    if (in) load_tab(T, A, t);
    else fresh_state(T, 0u, empty_deal());
    wave_lds_sync();
    // legal_moves(state)[a] of a live table, evaluated here: the arena's legal-mask cache is not consulted
    bool ok = false;
    if (in && !is_terminal(T.sw)) {
        uint32_t pw4[4];
        get_player(T, get_to_play(T.sw), pw4);
        int bank[6];
        get_bank(T.sw, bank);
        ok = action_legal(T.sw, unpack_pl(pw4), bank, a, L);
    }
    const int ptier = pop_tier(a);
    const bool drew = ok && ptier >= 0 && bget(T.sw[SW_DECK], ptier) > 0u;
    const StepPre pre = step_prefetch(T, a, ok, A, t, Tb);
    const StepOut o = step_rules(T, a, pre, ok, L, Tb, mtx, true, 1ull << a);
    const int moves = get_moves(T.sw);
    const size_t blk = (size_t)a * (size_t)A.n;  // the action's [n] plane; its rows t0.. are one contiguous block
    wave_lds_sync();
    if (S.obs) {  // the 297-byte staging serves both row forms
        succ_encode_row(T, L.rows, L, ok);
        wave_lds_sync();
        succ_store_obs<kSuccCpol>(L.rows, rows, S.obs + (blk + t0) * kObsDim);
        if (S.obs_u8) store_u8_from_rows(L.rows, rows, S.obs_u8 + (blk + t0) * kObsU8, ok ? (uint32_t)(moves >> 8) : 0u);
        if (__any(ok && moves > 255)) {  // move_count > 255 (crafted states only) does not fit the byte staging
            __builtin_amdgcn_s_waitcnt(0);
            if (ok && moves > 255) S.obs[(blk + t) * kObsDim + 295] = moves;
        }
    } else {
        succ_encode_row_u8(T, L.rows, L, ok);
        wave_lds_sync();
        succ_store_u8<kSuccCpol>(L.rows, rows, S.obs_u8 + (blk + t0) * kObsU8);
    }
    if (in) {
        const uint32_t f = !ok ? 0u
                               : (uint32_t)SPL_SUCC_LEGAL | (o.term ? (uint32_t)SPL_SUCC_TERMINATED : 0u) |
                                     ((o.flags & SPL_F_TURN_LIMIT) ? (uint32_t)SPL_SUCC_TURN_LIMIT : 0u) |
                                     (drew ? (uint32_t)SPL_SUCC_DREW : 0u);
        S.flags[blk + t] = (uint8_t)f;
        S.reward[blk + t] = ok ? o.reward : 0.0f;
        if (S.mask_bits) S.mask_bits[blk + t] = ok ? o.mask : 0ull;
        if (S.winner) S.winner[blk + t] = (int8_t)(ok ? get_winner(T.sw) : -1);
    }
}

}  // namespace spl
