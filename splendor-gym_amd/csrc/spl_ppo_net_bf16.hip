// spl_ppo_net_bf16.hip — spl_ppo_net_forward_bf16 and spl_ppo_net_backward_bf16 (include/splendor_ppo.h):
// the passes of spl_ppo_net_tiled.hip with bf16 operands on v_mfma_f32_32x32x16_bf16, float32 accumulation.
// Same launches, same buffers, same treatment of bad rows (all of it spl_ppo_net_tile.h's, shared with the f32
// source); NOT the same bytes as the f32 pairs.  Here are the bf16 stages and the matrix-instruction loops.
//
// The arithmetic (the header's contract): both operands of every matrix-instruction product are rounded from
// float32 to bf16, to nearest even, as they are staged into LDS (v_cvt_pk_bf16_f32), so LDS holds bf16 and a
// stage covers 64 of k in the room the f32 kernels need for 32.  The accumulators start from the bias (forward)
// or zero and stay float32; everything elementwise, the critic's single unit, its dZ2 and the bias gradients
// are float32 on the VALU from unrounded operands.  The inputs enter exactly: a byte is a bf16, and column
// 295 = byte 295 + 256 * byte 297 is fed as TWO k-positions, byte 295 at k = 295 and 256 * byte 297 at the pad
// position k = 297, both against W1[:, 295]; in dW1 the two positions' sums are added into column 295.
//
// Operand lane map of the 32x32x16 form, lane l, r = l & 31, h = l >> 5: A[i = r][k = 8 h + j] and
// B[k = 8 h + j][n = r], j = 0..7, so a fragment is 8 k-contiguous bf16 = one ds_read_b128, and every LDS
// image here is [row or unit][k].  An operand that lies [k][unit] in memory (W3, W2 in the dZ products; both
// operands of the sums over rows, whose k is the row) is transposed while it is staged: a thread loads one
// column down k, coalesced across threads, and writes its k-run packed.  Rows are 64 bf16 + 8 of pad = 144 B:
// the 16 lanes of a ds_read_b128 group then fall on 16 different 16-byte slots of the 256-byte bank row.
#include "spl_ppo_net_tile.h"

namespace spln {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kStage = 64;                        // k of one stage
constexpr int kLdb = kStage + 8;                  // row stride of an LDS image, in bf16
constexpr int kHiPos = kIn;                       // the pad position that carries 256 * byte 297
constexpr int kHiCol = 295;                       // the column it belongs to
static_assert(kIn == 297 && SPL_PPO_OBS_U8 == 300, "byte 297 is the dword at 296's second byte");

__device__ __forceinline__ bf16x4 pack4(const float *x) {
    bf16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (__bf16)x[e];
    return v;
}

__device__ __forceinline__ bf16x8 pack8(const float *x) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)x[e];
    return v;
}

// input k of a row from the store's bytes, as an integer that bf16 holds exactly: dword `w` holds bytes
// 4 * (k / 4) .. + 3 of the row (k < 300), or anything for k >= 300
__device__ __forceinline__ uint32_t input_at(uint32_t w, int k) {
    const uint32_t b = (w >> (8 * (k & 3))) & 255u;
    return k < kIn ? b : k == kHiPos ? b << 8 : 0u;
}

// grid (row tiles, 2): blockIdx.y 0 the actor, 1 the critic
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_bf16_gemm(Gemm g) {
    using S = Shape<MODE, kStage>;
    const int t = threadIdx.x, net = blockIdx.y;
    const int64_t b0 = (int64_t)blockIdx.x * kTileRows;
    if constexpr (MODE == F3 || MODE == Z2) {
        if (net == 1) {  // a single unit is no matrix product
            if constexpr (MODE == F3) value_rows(g, b0);
            else dz2_critic_rows(g, b0);
            return;
        }
    }
    __shared__ __attribute__((aligned(16))) __bf16 as[kTileRows * kLdb];  // [row][k]
    __shared__ __attribute__((aligned(16))) __bf16 ws[S::kNw * kLdb];     // [unit][k]
    // what this thread stages of a [row or unit][k] operand: k0 + 4 g4 .. + 3 of rows rw + 16 i
    const int g4 = t & 15, rw = t >> 4;
    const int lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int rt0 = S::kTm == 2 ? 0 : 32 * (wave >> 1);   // the wave's rows and units inside the workgroup's
    const int u0 = S::kTm == 2 ? 64 * wave : 32 * (wave & 1);
    const float *__restrict__ A = g.a[net];
    const float *__restrict__ W = g.w[net];

    // The rows this thread stages.  No load sits behind a per-lane branch: a row past B reads row B - 1, a
    // bad row reads position 0 (which every store has), and the value is replaced afterwards; the address of
    // a bad position is never formed.
    int64_t rowc[4];
    const uint8_t *src[4];
    unsigned okm = 0xfu;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t b = b0 + rw + 16 * i;
        rowc[i] = b < g.B ? b : (int64_t)g.B - 1;
    }
    if constexpr (S::kNeedOk) {
        int n_bad = 0;
        okm = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t pos = g.idx[rowc[i]];
            const bool ok = pos >= 0 && pos < g.total;
            okm |= (ok ? 1u : 0u) << i;
            n_bad += (!ok && b0 + rw + 16 * i < g.B) ? 1 : 0;
            if constexpr (S::kBytes) src[i] = g.obs + (ok ? pos : 0) * SPL_PPO_OBS_U8;
        }
        if constexpr (S::kBytes) {
            if (net == 0 && g4 == 0 && n_bad) atomicAdd(g.errors, (unsigned long long)n_bad);  // a row once
        }
    }

    // the next stage as loaded, on its way while this one is summed; what a clamped load brought is replaced
    // when the stage is rounded into LDS
    uint32_t ab[4];
    float an[4][4], wn[S::kWRegs];
    auto fetch = [&](int k0) {
        const int kb = k0 + 4 * g4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (S::kBytes) {  // the row's dword at kb: rows are 300 bytes, the plane 16-byte aligned
                ab[i] = *reinterpret_cast<const uint32_t *>(src[i] + (kb < SPL_PPO_OBS_U8 - 4 ? kb : SPL_PPO_OBS_U8 - 4));
            } else if constexpr (S::kVec) {
                const float4 v = *reinterpret_cast<const float4 *>(A + rowc[i] * S::kK + kb);
                an[i][0] = v.x, an[i][1] = v.y, an[i][2] = v.z, an[i][3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) an[i][e] = A[rowc[i] * S::kK + (kb + e < S::kK ? kb + e : S::kK - 1)];
            }
        }
        if constexpr (S::kKMajor) {  // thread t the unit, 64 rows of k
#pragma unroll
            for (int i = 0; i < S::kWRegs; ++i) {
                const int kk = k0 + i;
                wn[i] = W[(uint32_t)((kk < S::kK ? kk : S::kK - 1) * kH + t)];
            }
        } else {
#pragma unroll
            for (int i = 0; i < S::kWRegs / 4; ++i) {
                const int u = rw + 16 * i, uc = u < S::kUnits ? u : S::kUnits - 1;
                if constexpr (S::kVec) {
                    const float4 v = *reinterpret_cast<const float4 *>(W + (uint32_t)(uc * S::kK + kb));
                    wn[4 * i] = v.x, wn[4 * i + 1] = v.y, wn[4 * i + 2] = v.z, wn[4 * i + 3] = v.w;
                } else {  // layer 1: rows of 297 floats are only dword-aligned; position 297 reads column 295
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = kb + e;
                        wn[4 * i + e] = W[(uint32_t)(uc * S::kK + (k < S::kK ? k : kHiCol))];
                    }
                }
            }
        }
    };
    // the fetched stage, rounded to bf16, into LDS
    auto stage = [&](int k0) {
        const int kb = k0 + 4 * g4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = (okm >> i) & 1u;
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (S::kBytes) x[e] = ok ? (float)input_at(ab[i], kb + e) : 0.f;
                else x[e] = (ok && kb + e < S::kK) ? an[i][e] : 0.f;
            }
            *reinterpret_cast<bf16x4 *>(&as[(rw + 16 * i) * kLdb + 4 * g4]) = pack4(x);
        }
        if constexpr (S::kKMajor) {
#pragma unroll
            for (int c = 0; c < S::kWRegs / 8; ++c) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = k0 + 8 * c + e < S::kK ? wn[8 * c + e] : 0.f;
                *reinterpret_cast<bf16x8 *>(&ws[t * kLdb + 8 * c]) = pack8(x);
            }
        } else {
#pragma unroll
            for (int i = 0; i < S::kWRegs / 4; ++i) {
                const int u = rw + 16 * i;
                float x[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = kb + e;
                    const bool live = u < S::kUnits && (S::kBytes ? k <= kHiPos : k < S::kK);
                    x[e] = live ? wn[4 * i + e] : 0.f;
                }
                *reinterpret_cast<bf16x4 *>(&ws[u * kLdb + 4 * g4]) = pack4(x);
            }
        }
    };
    fetch(0);

    f32x16 acc[S::kTm][S::kTn];
    acc_start<MODE>(g, net, u0, r, acc);

    for (int k0 = 0; k0 < S::kKp; k0 += kStage) {
        __syncthreads();  // the stage's readers are done
        stage(k0);
        __syncthreads();
        if (k0 + kStage < S::kKp) fetch(k0 + kStage);
#pragma unroll
        for (int s = 0; s < kStage / 16; ++s) {
            const int kk = 16 * s + 8 * h;
            bf16x8 av[S::kTm], bv[S::kTn];
#pragma unroll
            for (int i = 0; i < S::kTm; ++i) av[i] = *reinterpret_cast<const bf16x8 *>(&as[(rt0 + 32 * i + r) * kLdb + kk]);
#pragma unroll
            for (int j = 0; j < S::kTn; ++j) bv[j] = *reinterpret_cast<const bf16x8 *>(&ws[(u0 + 32 * j + r) * kLdb + kk]);
#pragma unroll
            for (int i = 0; i < S::kTm; ++i)
#pragma unroll
                for (int j = 0; j < S::kTn; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

    tile_store<MODE, true>(g, net, b0, rt0, u0, r, h, acc);
}

// ---------------------------------------------------------------------------------------------
// the sums over rows: dW and db of every layer, per partial
// ---------------------------------------------------------------------------------------------
// The stages are 64 rows; both operands lie [row][column] in memory and [column][row] in LDS (the blocks:
// spl_ppo_net_tile.h).  In layer 1 the narrow operand's columns are X's positions: position 297 is column 295's
// second half and is added to it in the epilogue.
// The bias gradient, the column against ones, is a float32 sum of the unrounded values down the same rows on
// the VALU: by the thread that stages the column (layers 1 and 2), or by the four threads that stage a
// quarter of the stage's rows each, added in order at the end (layer 3).
//
// A wave stages 16 rows of the narrow operand, a lane a column, so a row's position is the same for the whole
// wave: the sixteen are read by one load, a row a lane, ahead of the first byte that depends on one, and
// broadcast from their lanes.  No load sits behind a per-lane branch.
constexpr int kDwStage = kStage;  // rows of a stage
static_assert(kChunkRows % kDwStage == 0, "a chunk is a whole number of stages");

template <int LAYER>
__device__ __forceinline__ void dw_block(const Bwd &g, const int net, const int n0, const int part, __bf16 *const lds) {
    __bf16 *const wide_s = lds, *const narrow_s = lds + kH * kLdb;
    const int t = threadIdx.x;
    const int n3 = net == 0 ? kA : 1;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
    const int ncol = lane, nq = wave;  // what this thread stages of the narrow operand: rows 16 nq .. + 15
    const float *__restrict__ wide = LAYER == 1   ? g.dz + (int64_t)(net * 2 + 1) * g.B * kH
                                     : LAYER == 2 ? g.dz + (int64_t)(net * 2 + 0) * g.B * kH
                                                  : g.act + (int64_t)(net * 2 + 1) * g.B * kH;
    const float *__restrict__ h1 = g.act + (int64_t)(net * 2 + 0) * g.B * kH;
    const float *__restrict__ dout = g.dout[net];
    const int64_t *__restrict__ idx = g.idx;
    const uint8_t *__restrict__ obs = g.obs;

    float wn[kDwStage], nn[16];
    // A row past `end` reads row end - 1, a column past the matrix its last one, a bad row position 0, and the
    // value is then replaced; the address of a bad position is never formed.
    auto fetch = [&](int64_t s0, int64_t end) {
        const float *wrow = wide + s0 * kH + t;
        // The stage's live rows, >= 1, in a vector register on purpose: as a scalar, the 64 clamped offsets and
        // the 64 masks of the loop below are scalars too, all live at once, and the compiler spilled hundreds of them.
        const int live_s = (int)(end - s0 < kDwStage ? end - s0 : kDwStage);
        int live_rows;
        asm("v_mov_b32 %0, %1" : "=v"(live_rows) : "s"(live_s));
#pragma unroll
        for (int i = 0; i < kDwStage; ++i) {
            const float v = wrow[(uint32_t)((i < live_rows ? i : live_rows - 1) * kH)];
            wn[i] = i < live_rows ? v : 0.f;
        }
        // The sixteen rows' positions: lane l loads row (l & 15)'s and keeps, in three registers, the byte offset of
        // its observation row (0 for a bad one) and whether the row counts (live, at a good position); row i's are
        // broadcast from lane i when its value is loaded.  Sixteen 64-bit positions held as scalars spilled SGPRs.
        const int64_t bl = s0 + 16 * nq + (lane & 15);
        int keepl = bl < end ? 1 : 0;
        uint32_t off_lo = 0, off_hi = 0;
        if constexpr (LAYER != 2) {
            const int64_t p = idx[bl < end ? bl : end - 1];
            const bool ok = p >= 0 && p < g.total;
            keepl = ok ? keepl : 0;
            const uint64_t off = (uint64_t)(ok ? p : 0) * SPL_PPO_OBS_U8;
            off_lo = (uint32_t)off, off_hi = (uint32_t)(off >> 32);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = (int)s0 + 16 * nq + i, bc = b < (int)end ? b : (int)end - 1;  // uniform; B <= 65 536
            const bool keep = __builtin_amdgcn_readlane(keepl, i) != 0;
            float x;
            if constexpr (LAYER == 2) {
                x = h1[(int64_t)bc * kH + n0 + ncol];
            } else if constexpr (LAYER == 1) {
                const int n = n0 + ncol;  // a position of k: < 300 reads its own byte
                const uint64_t off = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_lo, i) |
                                     (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, i) << 32;
                const uint32_t v = obs[off + (n < SPL_PPO_OBS_U8 ? n : SPL_PPO_OBS_U8 - 1)];
                x = (float)(n < kIn ? v : n == kHiPos ? v << 8 : 0u);
            } else {
                x = dout[(int64_t)bc * n3 + (ncol < n3 ? ncol : n3 - 1)];
                x = ncol < n3 ? x : 0.f;
            }
            nn[i] = keep ? x : 0.f;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    const bool wide_bias = LAYER != 3 && n0 == 0;  // uniform
    float bsum = 0.f;
    // The MFMA's A operand is the units (m), its B operand the columns (n): the wide and the narrow stage in
    // layers 1 and 2, the other way round in layer 3.  This lane's fragment of tile 0 at k = 0:
    const __bf16 *const wide_l = wide_s + (64 * wave + r) * kLdb + 8 * h, *const narrow_l = narrow_s + r * kLdb + 8 * h;
    const __bf16 *const a_s = LAYER == 3 ? narrow_l : wide_l, *const b_s = LAYER == 3 ? wide_l : narrow_l;

    // the stages of chunks p, p + parts, ... in row order; the next one is fetched while this one is summed
    int c = part;
    int64_t s0 = (int64_t)c * kChunkRows;
    bool more = c < g.chunks;
    if (more) fetch(s0, end_of(g, c));
    while (more) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kDwStage / 8; ++i) *reinterpret_cast<bf16x8 *>(&wide_s[t * kLdb + 8 * i]) = pack8(wn + 8 * i);
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<bf16x8 *>(&narrow_s[ncol * kLdb + 16 * nq + 8 * i]) = pack8(nn + 8 * i);
        if (wide_bias) {
#pragma unroll
            for (int i = 0; i < kDwStage; ++i) bsum += wn[i];
        } else if constexpr (LAYER == 3) {
#pragma unroll
            for (int i = 0; i < 16; ++i) bsum += nn[i];
        }
        __syncthreads();
        next_stage(g, kDwStage, c, s0);
        more = c < g.chunks;
        if (more) fetch(s0, end_of(g, c));
#pragma unroll
        for (int s = 0; s < kDwStage / 16; ++s) {
            bf16x8 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const bf16x8 *>(a_s + 32 * i * kLdb + 16 * s);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const bf16x8 *>(b_s + 32 * j * kLdb + 16 * s);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

    const DwOut o = dw_out(g, LAYER, net, part);
    if (LAYER == 1 && n0 + kNarrow > kHiPos) {  // uniform: position 297 (lane r + 2 of the same half) into column 295
        static_assert(kHiCol / 32 == kHiPos / 32 && kHiPos - kHiCol == 2, "both in one tile, two lanes apart");
        const int j = (kHiCol - 4 * kNarrow) / 32;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float hi = __shfl(acc[i][j][q], (lane + 2) & 63);
                if (n0 + 32 * j + r == kHiCol) acc[i][j][q] += hi;
            }
    }
    dw_store(LAYER, o, n0, wave, r, h, acc);
    if (wide_bias) {
        o.out[t * o.nc + o.nc - 1] = bsum;
    } else if constexpr (LAYER == 3) {  // the four quarters of a stage's rows, in order
        __syncthreads();
        float *const q4 = reinterpret_cast<float *>(lds);
        q4[nq * kNarrow + ncol] = bsum;
        __syncthreads();
        if (t < o.m_live) o.out[t * o.nc + o.nc - 1] = ((q4[t] + q4[kNarrow + t]) + q4[2 * kNarrow + t]) + q4[3 * kNarrow + t];
    }
}

// grid (2 * kDwBlocks, parts).  The blocks of one partial read the same rows of dZ1 (five of them), dZ2 (four)
// and H1, so they are dealt to ONE of the eight dies and its L2: workgroups go round the dies in launch
// order, and the remap gives each die a run of consecutive (partial, network, block) triples.  It is a
// bijection of the grid, for speed alone; a grid that is no multiple of eight keeps the launch order.
__global__ __launch_bounds__(kBlock) void k_bf16_dw(Bwd g) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[(kH + kNarrow) * kLdb];
    const unsigned nwg = gridDim.x * gridDim.y;
    unsigned bid = blockIdx.x + gridDim.x * blockIdx.y;
    if (nwg % 8 == 0) bid = (bid % 8) * (nwg / 8) + bid / 8;
    const int part = bid / (2 * kDwBlocks), x = bid % (2 * kDwBlocks), net = x / kDwBlocks, y = x % kDwBlocks;
    if (y < 5) dw_block<1>(g, net, kNarrow * y, part, lds);
    else if (y < 9) dw_block<2>(g, net, kNarrow * (y - 5), part, lds);
    else dw_block<3>(g, net, 0, part, lds);
}

}  // namespace spln

using namespace spln;

extern "C" {

int spl_ppo_net_forward_bf16(int32_t B, const spl_ppo_net_fwd_t *a, void *stream) {
    return forward_tiles(B, a, stream, k_bf16_gemm<F1>, k_bf16_gemm<F2>, k_bf16_gemm<F3>, "k_bf16_gemm (forward)");
}

int spl_ppo_net_backward_bf16(int32_t B, const spl_ppo_net_bwd_t *a, void *stream) {
    return backward_tiles(B, a, stream, k_bf16_gemm<Z2>, k_bf16_gemm<Z1>, k_bf16_dw, "k_bf16_gemm (backward)");
}

}  // extern "C"
