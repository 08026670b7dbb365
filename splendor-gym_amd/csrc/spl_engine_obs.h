#pragma once
// spl_engine_obs.h — the observation encoder and the block stores: a table's 297 observation bytes assembled in
// registers (rput ... build_row), staged into the wave's LDS row block (encode_row, its halves and the compact
// form) or stored by the lane itself (store_row_direct), and the wave's coalesced 16-byte stores of the staged
// rows and masks (V4Sink, store_obs_*, store_u8_from_rows, store_mask_block).
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_layout.h"

namespace spl {

// ------------------------------------------------------------------------------------------
// observation (engine/encode.py:124-187) into the wave's LDS row block, as bytes
// ------------------------------------------------------------------------------------------
// The wave's rows are packed back to back (row r at byte 297r), so most fields of a lane's row
// sit at unaligned LDS addresses: written field by field they compile to unaligned ds_write_b96
// / b32 accesses that stall the LDS pipe (SQ_LDS_UNALIGNED_STALL) and to ~35 byte writes per row.
// Instead each lane assembles its 297 bytes as 75 dwords in registers (R[j] = bytes 4j..4j+3;
// every offset is a compile-time constant, so R stays in VGPRs) and writes the ALIGNED dwords
// that start inside its row, shifted into place with v_alignbyte_b32; the dword that straddles
// rows L and L+1 is completed with row L+1's first bytes (its bank counts) taken from lane L+1.

// n bytes of v at byte offset o of the row (o, n compile-time after unrolling)
__device__ __forceinline__ void rput(uint32_t (&R)[76], int o, int n, uint32_t v) {
    if (n < 4) v &= (1u << (8 * n)) - 1u;
    const int j = o >> 2, sh = (o & 3) * 8;
    R[j] |= v << sh;
    if (sh != 0 && (o & 3) + n > 4) R[j + 1] |= v >> (32 - sh);
}

__device__ __forceinline__ void rput_card13(uint32_t (&R)[76], int o, uint4 rec, bool present) {
    rput(R, o, 4, present ? rec.x : 0u);
    rput(R, o + 4, 4, present ? rec.y : 0u);
    rput(R, o + 8, 4, present ? rec.z : 0u);
    rput(R, o + 12, 1, present ? rec.w : 0u);
}

// The 297 observation bytes of table T as dwords R[0..74] (R[75] = 0).
template <int P>
__device__ __forceinline__ void build_row(const Tab<P> &T, const Consts &L, uint32_t (&R)[76]) {
    const uint32_t *sw = T.sw;
    const int tp = get_to_play(sw);
#pragma unroll
    for (int j = 0; j < 76; ++j) R[j] = 0u;
    rput(R, 0, 4, sw[SW_BANK0]);                // bank :128
    rput(R, 4, 2, sw[SW_BANK1]);
    uint32_t me[4], op[4];
    get_player(T, tp, me);                      // current :131-135
    get_player(T, (tp + 1) % P, op);            // opponent = next player :138-142
    rput(R, 6, 4, me[0]);
    rput(R, 10, 4, me[1]);
    rput(R, 14, 4, me[2]);
    rput(R, 18, 1, me[3] & 3u);
    rput(R, 19, 4, op[0]);
    rput(R, 23, 4, op[1]);
    rput(R, 27, 4, op[2]);
    rput(R, 31, 1, op[3] & 3u);
#pragma unroll
    for (int k = 0; k < 12; ++k) {              // board :144-147
        const int id = (int)bget(sw[SW_BOARD + k / 4], k % 4);
        rput_card13(R, 32 + 13 * k, card_rec(L, id), id != 0xFF);
    }
    const int mn = (int)(me[3] & 3u), on = (int)(op[3] & 3u), orev = (int)((op[3] >> 2) & 7u);
#pragma unroll
    for (int i = 0; i < 3; ++i) {               // own reserved, always revealed :151-155
        const bool pr = i < mn;
        rput_card13(R, 188 + 14 * i, card_rec(L, (int)bget(me[3], i + 1)), pr);
        rput(R, 188 + 14 * i + 13, 1, pr ? 1u : 0u);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {               // opponent reserved, hidden -> zeros :158-168
        const bool pr = i < on && ((orev >> i) & 1);
        rput_card13(R, 230 + 14 * i, card_rec(L, (int)bget(op[3], i + 1)), pr);
        rput(R, 230 + 14 * i + 13, 1, pr ? 1u : 0u);
    }
    const int nn = (int)bget(sw[SW_DECK], 3);
    const uint32_t owners = (sw[SW_NOB1] >> 8) & 0x7FFFu;
#pragma unroll
    for (int i = 0; i < 3; ++i) {               // nobles[:3] :171-178
        const int idx = (int)bget(sw[SW_NOB0], i);
        const bool pr = i < nn && ((owners >> (3 * i)) & 7u) == 0 && idx < 10;
        const uint2 rec = L.nobles[idx < 10 ? idx : 0];
        rput(R, 272 + 6 * i, 4, pr ? rec.x : 0u);
        rput(R, 276 + 6 * i, 2, pr ? rec.y : 0u);
    }
    rput(R, 290, 3, sw[SW_DECK]);               // deck sizes :180-181
    rput(R, 293, 1, (uint32_t)get_turn(sw));    // misc :183-186
    rput(R, 294, 1, (uint32_t)tp);
    rput(R, 295, 1, (uint32_t)get_moves(sw));   // > 255 patched after the block store
    rput(R, 296, 1, is_terminal(sw) ? 1u : 0u);
}

// Row of table T into rows_base[297*lane ...].  Every lane of the wave must call it (the row
// boundaries are shared with the neighbouring lanes); rows of lanes whose table is not needed
// are written too and simply not stored.
template <int P>
__device__ __forceinline__ void encode_row(const Tab<P> &T, uint8_t *rows_base, const Consts &L) {
    uint32_t R[76];
    build_row(T, L, R);
    // bytes 297..299: the next lane's row bytes 0..2 (its bank counts)
    R[74] |= (uint32_t)__shfl_down((int)R[0], 1) << 8;
    const int lane = lane_id();
    const uint32_t o0 = (4u - ((uint32_t)lane & 3u)) & 3u;  // row 297*lane starts at lane mod 4
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsDim * lane + o0);
#pragma unroll
    for (int j = 0; j < 74; ++j) dst[j] = __builtin_amdgcn_alignbyte(R[j + 1], R[j], o0);
    if (o0 == 0u) dst[74] = R[74];
}

// Half of encode_row: staged dwords [0, kRowHalf) (Half 0) or [kRowHalf, 75) (Half 1) of every
// lane's row, so two waves of a workgroup encode one block in parallel.  build_row is inlined
// with constant indices, so each half computes only the row bytes its dwords take.
constexpr int kRowHalf = 37;
template <int Half, int P>
__device__ __forceinline__ void encode_row_half(const Tab<P> &T, uint8_t *rows_base, const Consts &L) {
    uint32_t R[76];
    build_row(T, L, R);
    if (Half == 1) R[74] |= (uint32_t)__shfl_down((int)R[0], 1) << 8;
    const int lane = lane_id();
    const uint32_t o0 = (4u - ((uint32_t)lane & 3u)) & 3u;
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsDim * lane + o0);
    constexpr int j0 = Half == 0 ? 0 : kRowHalf, j1 = Half == 0 ? kRowHalf : 74;
#pragma unroll
    for (int j = j0; j < j1; ++j) dst[j] = __builtin_amdgcn_alignbyte(R[j + 1], R[j], o0);
    if (Half == 1 && o0 == 0u) dst[74] = R[74];
}

// The compact observation row (spl_step_args_t.obs_u8) of table T at rows_base[300*lane ...]:
// the row's 297 bytes, move_count >> 8, two zero bytes — 75 aligned dwords per row (no
// neighbouring-lane bytes).  Part 0: dwords [0, kRowHalf), 1: [kRowHalf, 75), 2: all.
template <int Part, int P>
__device__ __forceinline__ void encode_row_u8(const Tab<P> &T, uint8_t *rows_base, const Consts &L) {
    uint32_t R[76];
    build_row(T, L, R);
    R[74] = (R[74] & 0xFFu) | ((uint32_t)(get_moves(T.sw) >> 8) << 8);
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows_base + kObsU8 * lane_id());
    constexpr int j0 = Part == 1 ? kRowHalf : 0, j1 = Part == 0 ? kRowHalf : 75;
#pragma unroll
    for (int j = j0; j < j1; ++j) dst[j] = R[j];
}

// Observation of table T written by its own lane straight to dst[0..296] (int32; 297 dword
// stores): the rare path for terminal rows that do not fit the pipelined kernel's hand-off.
template <int P>
__device__ __forceinline__ void store_row_direct(const Tab<P> &T, const Consts &L, int32_t *dst) {
    uint32_t R[76];
    build_row(T, L, R);
#pragma unroll
    for (int e = 0; e < kObsDim; ++e) dst[e] = e == 295 ? get_moves(T.sw) : (int32_t)bget(R[e >> 2], e & 3);
}

// Block store of this wave's staged rows: obs[t0 .. t0+rows) as int32, 16 B per lane-store.
// LDS reads are issued in groups of 5 before their stores: one read-wait per store halves the
// store rate (tools/microbench_store.hip: 2.7 -> 5.2 TB/s).
// One 16-byte store per lane per instruction, typed as a native 4 x i32 vector indexed in vector
// units: with `int4` and 32-bit element indexing the compiler versions the loop and, in the
// unrolled copy, splits every store into four strided dword stores (half the store bandwidth).
typedef int v4i __attribute__((ext_vector_type(4)));

// The two output streams of a rollout.  NT: the per-step rollout store's row and mask blocks (written once
// and not read back by this launch) leave non-temporal, so the 5 GB stream does not push the token table,
// deck records and state out of L2 / the Infinity Cache — the rules wave's gathers stay fast (rollout store
// 1225 -> 1109 us per 64 steps at 65 536 tables; plain 13-22 % slower in the kernel, profiles/r06/roll_nt_ab_r06m.txt).
// In-place outputs keep plain stores: their block stays Infinity-Cache resident for the consumer (NT: 794 ->
// 1020 us).  So do the store's terminal rows and small outputs (through the NT stream: headline 1 972-1 984 vs
// 1 936-1 955 us, C4 1 177-1 178 vs 1 065-1 067; profiles/r06/small_outputs_nt_ab_r06ai.txt).
// The NT stream is a buffer store with a cache-policy immediate (gfx950: sc0 = 1, nt = 2, sc1 = 16) on a
// resource over the block: 19 = `sc0 nt sc1` (system scope, non-temporal), headline 1 941-1 952 against
// 1 975-2 002 us per launch with `nt` alone, four alternations on one box, 1.4 % on another; without nt
// 12 % slower (profiles/r06/store_policy_ab_r06u_v.txt)
constexpr int kRollCpol = 19;
constexpr int kPlainCpol = -2;
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
// 16-byte output stores into one wave-uniform block under cache policy CP: kPlainCpol plain stores, >= 0 a
// buffer store with that cache-policy immediate
template <int CP>
struct V4Sink {
    v4i *out;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ explicit V4Sink(void *p) : out(reinterpret_cast<v4i *>(p)) {
        if constexpr (CP >= 0) rs = __builtin_amdgcn_make_buffer_rsrc(p, (short)0, 0x7FFFFFF0, 0x00020000);
    }
    __device__ __forceinline__ void put(int i, v4i v) const {
        if constexpr (CP >= 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), rs, i * 16, 0, CP);
        else out[i] = v;
    }
};
// the policy of an output stream: the NT stream or plain stores
constexpr int stream_cpol(bool nt) { return nt ? kRollCpol : kPlainCpol; }

__device__ __forceinline__ v4i expand4(uint32_t w) {
    v4i v = {(int)(w & 0xFFu), (int)((w >> 8) & 0xFFu), (int)((w >> 16) & 0xFFu), (int)(w >> 24)};
    return v;
}

// Part [d0, d1) (LDS words, multiples of 64*5 except the end) of a FULL wave's observation block.
template <bool NT = false>
__device__ __forceinline__ void store_obs_range(const uint8_t *rows_lds, int32_t *dst, int d0, int d1) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    const V4Sink<stream_cpol(NT)> out(dst);
    constexpr int U = 5;
    int d = d0 + lane_id();
#pragma unroll 1
    for (; d + 64 * (U - 1) < d1; d += 64 * U) {
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = src[d + 64 * u];
#pragma unroll
        for (int u = 0; u < U; ++u) out.put(d + 64 * u, expand4(w[u]));
    }
    uint32_t w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = (d + 64 * u < d1) ? src[d + 64 * u] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (d + 64 * u < d1) out.put(d + 64 * u, expand4(w[u]));
}
constexpr int kObsBlockWords = 64 * kObsDim / 4;  // 4752 LDS words = 4752 16-byte stores per wave
constexpr int kObsSplit = 64 * 5 * 7;             // 2240: 35 stores per lane in the first part

// Block store of this wave's observation rows: LDS bytes [rows][297] -> int32 [rows][297] at
// dst (16-byte aligned: 64-row blocks are 76032 B).  Dword d of the block is LDS word d.
// R = the workgroup's table count (64, or 32 in the half-populated two-wave rollout).
template <int R = 64, bool NT = false, int CP = stream_cpol(NT)>
__device__ __forceinline__ void store_obs_block(const uint8_t *rows_lds, int rows, int32_t *dst) {
    const int nbytes = rows * kObsDim;
    const int full = nbytes >> 2;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    const V4Sink<CP> out(dst);
    constexpr int U = 5;
    int d = lane_id();
    if (rows == R) {  // every wave but a ragged last one: compile-time trip count
        constexpr int kFull = R * kObsDim / 4;  // 64 rows: 4752 = 14 x 320 + 272
#pragma unroll 1
        for (int it = 0; it < kFull / (64 * U); ++it, d += 64 * U) {
            uint32_t w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = src[d + 64 * u];
#pragma unroll
            for (int u = 0; u < U; ++u) out.put(d + 64 * u, expand4(w[u]));
        }
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = (d + 64 * u < kFull) ? src[d + 64 * u] : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (d + 64 * u < kFull) out.put(d + 64 * u, expand4(w[u]));
        return;
    }
    for (; d < full; d += 64) out.put(d, expand4(src[d]));
    for (int b = (full << 2) + lane_id(); b < nbytes; b += 64) dst[b] = (int32_t)rows_lds[b];
}

// store_obs_block (64 rows) with `mid()` issued between its first and second half: work that fills the
// wave's store-issue stalls instead of following the whole block (k_step_wso's legal mask).  Plain stores.
template <class Mid>
__device__ __forceinline__ void store_obs_block_mid(const uint8_t *rows_lds, int rows, int32_t *dst, Mid mid) {
    if (rows != 64) {
        mid();
        store_obs_block<64, false>(rows_lds, rows, dst);
        return;
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    const V4Sink<kPlainCpol> out(dst);
    constexpr int U = 5, kFull = 64 * kObsDim / 4, kIters = kFull / (64 * U);  // 4752 = 14 x 320 + 272
    int d = lane_id();
#pragma unroll 1
    for (int it = 0; it < kIters / 2; ++it, d += 64 * U) {
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = src[d + 64 * u];
#pragma unroll
        for (int u = 0; u < U; ++u) out.put(d + 64 * u, expand4(w[u]));
    }
    __asm__ volatile("" ::: "memory");
    mid();
    __asm__ volatile("" ::: "memory");
#pragma unroll 1
    for (int it = kIters / 2; it < kIters; ++it, d += 64 * U) {
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = src[d + 64 * u];
#pragma unroll
        for (int u = 0; u < U; ++u) out.put(d + 64 * u, expand4(w[u]));
    }
    uint32_t w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = (d + 64 * u < kFull) ? src[d + 64 * u] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (d + 64 * u < kFull) out.put(d + 64 * u, expand4(w[u]));
}

// Block store of `rows` compact rows (300 bytes each) staged in LDS to dst (16-byte aligned).
__device__ __forceinline__ void store_obs_u8_block(const uint8_t *rows_lds, int rows, uint8_t *dst) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    const int words = rows * (kObsU8 / 4), chunks = words >> 2;
    v4i *out = reinterpret_cast<v4i *>(dst);
    for (int c = lane_id(); c < chunks; c += 64) {
        const v4i v = {(int)src[4 * c], (int)src[4 * c + 1], (int)src[4 * c + 2], (int)src[4 * c + 3]};
        out[c] = v;
    }
    for (int w = 4 * chunks + lane_id(); w < words; w += 64) reinterpret_cast<uint32_t *>(dst)[w] = src[w];
}

// The compact rows (spl_step_args_t.obs_u8 layout: 297 bytes, move_count >> 8, two zero bytes) of
// the wave's staged 297-byte rows, stored beside their int32 block when a step writes both: 75 dwords
// per row, consecutive lanes on consecutive dwords (256-byte stores); dword j < 74 of row r is the
// staged bytes 297 r + 4 j .. + 3 (one v_alignbyte of the two staged dwords around them), dword 74
// is byte 296, move_count >> 8 (`mhi` of lane r, whose table is row r), 0, 0.  Every lane runs
// every iteration (the row's high byte comes by shuffle), the stores are predicated.  With a 16-byte
// aligned dst each lane builds four consecutive dwords (one 16-byte store; a chunk crosses at most one
// row end, whose dword 74 belongs to the chunk's first row), 19 iterations for 64 rows instead of 75.
__device__ __forceinline__ void store_u8_from_rows(const uint8_t *rows_lds, int rows, uint8_t *dst, uint32_t mhi) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows_lds);
    uint32_t *out = reinterpret_cast<uint32_t *>(dst);
    constexpr int kWords = kObsU8 / 4;  // 75
    const int total = rows * kWords;
    int q_first = 0;
    if (((uintptr_t)dst & 15u) == 0) {
        const int chunks = total >> 2;
        v4i *out4 = reinterpret_cast<v4i *>(dst);
        for (int it = 0; it < (chunks + 63) / 64; ++it) {
            const int c = lane_id() + 64 * it, cc = c < chunks ? c : chunks - 1;
            const int q0 = 4 * cc, r0 = q0 / kWords, j0 = q0 - kWords * r0;
            const uint32_t h = (uint32_t)__shfl((int)mhi, r0);
            v4i v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool next = j0 + i >= kWords;  // past row r0's end: row r0 + 1 from its byte 0
                const int j = next ? j0 + i - kWords : j0 + i;
                const int b = kObsDim * (next ? r0 + 1 : r0) + 4 * j;
                uint32_t w = __builtin_amdgcn_alignbyte(src[(b >> 2) + 1], src[b >> 2], (uint32_t)(b & 3));
                if (j0 + i == kWords - 1) w = (w & 0xFFu) | (h << 8);
                v[i] = (int)w;
            }
            if (c < chunks) out4[c] = v;
        }
        q_first = chunks << 2;
    }
    for (int it = 0; it < (total - q_first + 63) / 64; ++it) {
        const int q = q_first + lane_id() + 64 * it, qq = q < total ? q : total - 1;
        const int r = qq / kWords, j = qq - kWords * r;
        const int b = kObsDim * r + 4 * j;  // staged byte; b / 4 + 1 <= 4 677 < 64 * 300 / 4
        uint32_t v = __builtin_amdgcn_alignbyte(src[(b >> 2) + 1], src[b >> 2], (uint32_t)(b & 3));
        const uint32_t h = (uint32_t)__shfl((int)mhi, r);
        if (j == kWords - 1) v = (v & 0xFFu) | (h << 8);
        if (q < total) out[q] = v;
    }
}

// Block store of this wave's masks: mask[t0 .. t0+rows) as int8 [rows][45].  The 64 x 45 mask
// bits are first laid out as ONE bit stream in LDS (row r at bits 45r..45r+44; each stream
// dword is cut from at most two rows), so every output dword is one nibble of the stream,
// spread to 4 bytes by a multiply: bit i of n moves to bit 8i in n * 0x204081.
template <bool NT = false, int CP = stream_cpol(NT)>
__device__ __forceinline__ void store_mask_block(const uint64_t *mask, uint32_t *mbits, int rows, int8_t *dst) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int w = lane_id() + 64 * k;  // stream dword w: bits 32w .. 32w+31
        if (w < kMaskStreamWords) {
            const int r0 = (32 * w) / 45, c0 = 32 * w - 45 * r0;  // first bit: row r0, column c0
            const uint64_t m0 = mask[r0], m1 = r0 + 1 < 64 ? mask[r0 + 1] : 0ull;
            // columns c0..44 of row r0, then row r0+1 from column 0
            const uint64_t lo = m0 >> c0, hi = (c0 > 13) ? (m1 << (45 - c0)) : 0ull;
            mbits[w] = (uint32_t)(lo | hi);
        }
    }
    wave_lds_sync();
    if ((rows == 64 || rows == 32) && ((uintptr_t)dst & 15u) == 0) {  // 180 (90) x 16 B
        const V4Sink<CP> out4(dst);
        const int nc = rows * 45 / 16;
        for (int c = lane_id(); c < nc; c += 64) {
            const uint32_t half = (mbits[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;  // stream bits 16c..16c+15
            v4i v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (int)((((half >> (4 * q)) & 0xFu) * 0x00204081u) & 0x01010101u);
            out4.put(c, v);
        }
        return;
    }
    const int nbytes = rows * 45;
    const int full = nbytes >> 2;
    uint32_t *out = reinterpret_cast<uint32_t *>(dst);
    for (int d = lane_id(); d < full; d += 64) {
        const uint32_t nib = (mbits[d >> 3] >> (4 * (d & 7))) & 0xFu;
        out[d] = (nib * 0x00204081u) & 0x01010101u;
    }
    for (int b = (full << 2) + lane_id(); b < nbytes; b += 64)
        dst[b] = (int8_t)((mbits[b >> 5] >> (b & 31)) & 1u);
}

}  // namespace spl
