// spl_ppo_net_bf16.hip — spl_ppo_net_forward_bf16 and spl_ppo_net_backward_bf16 (include/splendor_ppo.h):
// the passes of spl_ppo_net_tiled.hip with bf16 operands on v_mfma_f32_32x32x16_bf16, float32 accumulation.
// Same launches (forward: layer 1, layer 2, the output layers; backward: dZ2, dZ1, the sums over rows,
// k_net_reduce unchanged), same buffers, same treatment of bad rows; NOT the same bytes as the f32 pairs.
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
// C/D is the f32 form's: D[i = (q & 3) + 8 (q >> 2) + 4 h][j = r] in register q.
#include "spl_ppo_net_common.h"

namespace spln {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kTileRows = SPL_PPO_NET_TILE_ROWS;  // rows of a workgroup of the forward and dZ launches
constexpr int kStage = 64;                        // k of one stage
constexpr int kLdb = kStage + 8;                  // row stride of an LDS image, in bf16
constexpr int kHiPos = kIn;                       // the pad position that carries 256 * byte 297
constexpr int kHiCol = 295;                       // the column it belongs to
static_assert(kTileRows == 64, "a workgroup's four waves cover 64 rows as 2 x 2 or 1 x 1 tiles of 32 x 32");
static_assert(kIn == 297 && SPL_PPO_OBS_U8 == 300, "byte 297 is the dword at 296's second byte");

__device__ __forceinline__ int d_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

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

// ---------------------------------------------------------------------------------------------
// out = epilogue(C0 + A W): forward layers and the two dZ products
// ---------------------------------------------------------------------------------------------
struct Gemm {
    int B;
    int64_t total;
    const int64_t *idx;
    const uint8_t *obs;
    const float *a[2];     // the rows' operand where it is floats: [B][256], or dOut
    const float *w[2];     // the weight
    const float *bias[2];  // forward: where the sums start
    const float *h[2];     // dZ: the activations behind the tanh whose derivative is applied, [B][256]
    float *out[2];
    unsigned long long *errors;
};

enum { F1, F2, F3, Z2, Z1 };

template <int MODE>
struct Shape {
    static constexpr bool kBytes = MODE == F1;                   // A is rebuilt from the store's bytes
    static constexpr bool kKMajor = MODE == Z2 || MODE == Z1;    // W is [k][unit]; otherwise [unit][k]
    static constexpr int kK = MODE == F1 ? kIn : MODE == Z2 ? kA : kH;
    static constexpr int kKp = (kK + kStage - 1) / kStage * kStage;  // whole stages: 320, 256, 64
    static constexpr int kUnits = MODE == F3 ? kA : kH;          // live units
    static constexpr int kNw = MODE == F3 ? 64 : kH;             // units of a workgroup
    static constexpr int kTm = MODE == F3 ? 1 : 2, kTn = kTm;    // a wave's tiles
    static constexpr bool kNeedOk = MODE == F1 || MODE == Z2;    // bad rows are zeros in A
    static constexpr int kWRegs = kNw * kStage / kBlock;         // a thread's elements of a weight stage
    static constexpr bool kVec = kK % 4 == 0;                    // rows of A and of a [unit][k] W are 16-byte aligned
};

// The critic's output layer: row b's value = b3 + SUM_k H2[b][k] w3[k], k ascending, a thread a row; float32.
__device__ __forceinline__ void value_rows(const Gemm &g, int64_t b0) {
    const int t = threadIdx.x;
    if (t >= kTileRows) return;
    const int64_t b = b0 + t, bc = b < g.B ? b : (int64_t)g.B - 1;
    const int64_t pos = g.idx[bc];
    const float4 *hrow = reinterpret_cast<const float4 *>(g.a[1] + bc * kH);
    const float4 *w = reinterpret_cast<const float4 *>(g.w[1]);
    float y = g.bias[1][0];
#pragma unroll 16
    for (int k = 0; k < kH / 4; ++k) {
        const float4 c = w[k], x = hrow[k];
        y = __builtin_fmaf(x.x, c.x, y);
        y = __builtin_fmaf(x.y, c.y, y);
        y = __builtin_fmaf(x.z, c.z, y);
        y = __builtin_fmaf(x.w, c.w, y);
    }
    if (b < g.B) g.out[1][b] = (pos >= 0 && pos < g.total) ? y : 0.f;
}

// The critic's dZ2: one product a row and unit, dvalue * w3[t], times 1 - H2^2; thread t the unit; float32.
__device__ __forceinline__ void dz2_critic_rows(const Gemm &g, int64_t b0) {
    const int t = threadIdx.x;
    const float w = g.w[1][t];
#pragma unroll 8
    for (int r = 0; r < kTileRows; ++r) {
        const int64_t b = b0 + r, bc = b < g.B ? b : (int64_t)g.B - 1;  // uniform
        const int64_t pos = g.idx[bc];
        const float dv = g.a[1][bc], hh = g.h[1][bc * kH + t];
        const float d = (pos >= 0 && pos < g.total) ? dv : 0.f;
        const float z = __builtin_fmaf(d, w, 0.f) * __builtin_fmaf(-hh, hh, 1.f);
        if (b < g.B) g.out[1][b * kH + t] = z;
    }
}

}  // namespace

// grid (row tiles, 2): blockIdx.y 0 the actor, 1 the critic
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_bf16_gemm(Gemm g) {
    using S = Shape<MODE>;
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
#pragma unroll
    for (int j = 0; j < S::kTn; ++j) {
        float c0 = 0.f;
        if constexpr (MODE == F1 || MODE == F2 || MODE == F3) {
            const int u = u0 + 32 * j + r;
            c0 = g.bias[net][u < S::kUnits ? u : S::kUnits - 1];
        }
#pragma unroll
        for (int i = 0; i < S::kTm; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = c0;
    }

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

    // epilogue: register q of tile (i, j) is row rt0 + 32 i + d_row(q, h), unit u0 + 32 j + r
#pragma unroll
    for (int i = 0; i < S::kTm; ++i) {
        // dZ: a tile's activations are all loaded before its first store (the planes may be one allocation, so
        // a load behind a store would wait for it: 32 round trips in a row)
        float hh[16][S::kTn];
        if constexpr (MODE == Z2 || MODE == Z1) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t b = b0 + rt0 + 32 * i + d_row(q, h);
                const int64_t bc = b < g.B ? b : (int64_t)g.B - 1;
#pragma unroll
                for (int j = 0; j < S::kTn; ++j) hh[q][j] = g.h[net][bc * kH + u0 + 32 * j + r];
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t b = b0 + rt0 + 32 * i + d_row(q, h);
            const int64_t bc = b < g.B ? b : (int64_t)g.B - 1;
            bool ok = true;
            if constexpr (MODE == F3) {
                const int64_t pos = g.idx[bc];
                ok = pos >= 0 && pos < g.total;
            }
#pragma unroll
            for (int j = 0; j < S::kTn; ++j) {
                const int u = u0 + 32 * j + r;
                const float y = acc[i][j][q];
                if constexpr (MODE == F1 || MODE == F2) {
                    if (b < g.B) g.out[net][b * kH + u] = tanh_acc(y);
                } else if constexpr (MODE == F3) {
                    if (b < g.B && u < kA) g.out[0][b * kA + u] = ok ? y : 0.f;
                } else {
                    if (b < g.B) g.out[net][b * kH + u] = y * __builtin_fmaf(-hh[q][j], hh[q][j], 1.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the sums over rows: dW and db of every layer, per partial
// ---------------------------------------------------------------------------------------------
// A workgroup sums one block of one dW over the chunks p, p + parts, ... of its partial, 64 rows a stage
// (zeros past a chunk's end), rows the MFMA's k.  Both operands lie [row][column] in memory and [column][row]
// in LDS.  The `wide` one has 256 columns, 64 a wave; the `narrow` one 64, which every wave reads:
//   layer 1: dW1[m][n0 .. n0 + 63]: wide dZ1 (m), narrow X's positions (n), 5 blocks; position 297 is column
//            295's second half and is added to it in the epilogue
//   layer 2: dW2[m][n0 .. n0 + 63]: wide dZ2 (m), narrow H1's columns (n), 4 blocks
//   layer 3: dW3[m < 45 | 1][n]:    wide H2 (n), narrow dOut (m), 1 block
// The bias gradient, the column against ones, is a float32 sum of the unrounded values down the same rows on
// the VALU: by the thread that stages the column (layers 1 and 2), or by the four threads that stage a
// quarter of the stage's rows each, added in order at the end (layer 3).
//
// A wave stages 16 rows of the narrow operand, a lane a column, so a row's position is the same for the whole
// wave: the sixteen are read by one load, a row a lane, ahead of the first byte that depends on one, and
// broadcast from their lanes.  No load sits behind a per-lane branch.
constexpr int kDwBlocks = 5 + 4 + 1;  // a network's
constexpr int kNarrow = 64;
constexpr int kDwStage = kStage;      // rows of a stage
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
    auto end_of = [&](int c) {
        const int64_t e = (int64_t)(c + 1) * kChunkRows;
        return e < g.B ? e : (int64_t)g.B;
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
    if (more) fetch(s0, end_of(c));
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
        s0 += kDwStage;
        if (s0 >= end_of(c)) {
            c += g.parts;
            s0 = (int64_t)c * kChunkRows;
        }
        more = c < g.chunks;
        if (more) fetch(s0, end_of(c));
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

    const int nc = LAYER == 1 ? kC1 : kC2;
    const int m_live = LAYER == 3 ? n3 : kH;
    float *out = g.partial + (int64_t)part * kPartFloats + net * kActorFloats + (LAYER == 1 ? 0 : LAYER == 2 ? kOff2 : kOff3);
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
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = (LAYER == 3 ? 0 : 64 * wave) + 32 * i + d_row(q, h);
                const int n = (LAYER == 3 ? 64 * wave : n0) + 32 * j + r;
                if (m < m_live && n < nc - 1) out[m * nc + n] = acc[i][j][q];
            }
    if (wide_bias) {
        out[t * nc + nc - 1] = bsum;
    } else if constexpr (LAYER == 3) {  // the four quarters of a stage's rows, in order
        __syncthreads();
        float *const q4 = reinterpret_cast<float *>(lds);
        q4[nq * kNarrow + ncol] = bsum;
        __syncthreads();
        if (t < m_live) out[t * nc + nc - 1] = ((q4[t] + q4[kNarrow + t]) + q4[2 * kNarrow + t]) + q4[3 * kNarrow + t];
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
    Fwd f;
    if (const int e = fwd_args(B, a, f)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]
    Gemm g{};
    g.B = B, g.total = f.total, g.idx = f.idx, g.obs = f.obs, g.errors = f.errors;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n) g.a[n] = nullptr, g.w[n] = f.net[n].w1, g.bias[n] = f.net[n].b1, g.out[n] = f.act + (2 * n) * slot;
    hipLaunchKernelGGL(k_bf16_gemm<F1>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = f.act + (2 * n) * slot, g.w[n] = f.net[n].w2, g.bias[n] = f.net[n].b2, g.out[n] = f.act + (2 * n + 1) * slot;
    hipLaunchKernelGGL(k_bf16_gemm<F2>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n) g.a[n] = f.act + (2 * n + 1) * slot, g.w[n] = f.net[n].w3, g.bias[n] = f.net[n].b3;
    g.out[0] = f.logits, g.out[1] = f.value;
    hipLaunchKernelGGL(k_bf16_gemm<F3>, grid, block, 0, s, g);
    return spl_launched("k_bf16_gemm (forward)");
}

int spl_ppo_net_backward_bf16(int32_t B, const spl_ppo_net_bwd_t *a, void *stream) {
    Bwd b;
    if (const int e = bwd_args(B, a, b)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]; dz: [network][dZ2, dZ1][B][256]
    Gemm g{};
    g.B = B, g.total = b.total, g.idx = b.idx, g.obs = b.obs;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dout[n], g.w[n] = b.w3[n], g.h[n] = b.act + (2 * n + 1) * slot, g.out[n] = b.dz + (2 * n) * slot;
    hipLaunchKernelGGL(k_bf16_gemm<Z2>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dz + (2 * n) * slot, g.w[n] = b.w2[n], g.h[n] = b.act + (2 * n) * slot, g.out[n] = b.dz + (2 * n + 1) * slot;
    hipLaunchKernelGGL(k_bf16_gemm<Z1>, grid, block, 0, s, g);
    hipLaunchKernelGGL(k_bf16_dw, dim3(2 * kDwBlocks, b.parts), block, 0, s, b);
    launch_net_reduce(b, s);
    return spl_launched("k_bf16_gemm (backward)");
}

}  // extern "C"
