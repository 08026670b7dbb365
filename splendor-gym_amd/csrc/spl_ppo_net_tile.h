// spl_ppo_net_tile.h — what the two tiled sources of the PPO network passes share (spl_ppo_net_tiled.hip, the
// f32-input MFMA; spl_ppo_net_bf16.hip, bf16 operands): everything about a tile that is not the operand format.
// The products' argument block and shapes, the critic's single unit on the VALU, where an accumulator starts,
// the write-out of the five products and of the dW partials, the walk over a partial's chunks, and the launch
// sequences.  A source keeps what IS its format: how a stage is fetched, rounded and laid out in LDS, the
// fragment loads and the matrix-instruction loop, and the bias-gradient sums.
//
// Launches: forward 3 (layer 1, layer 2, the output layers), backward 4 (dZ2, dZ1, the sums over rows, the
// ordered combination of the partials).  C/D lane map of both 32x32 forms, lane l, r = l & 31, h = l >> 5:
// D[i = (q & 3) + 8 (q >> 2) + 4 h][j = r] in register q.
#pragma once
#include "spl_ppo_net_common.h"

namespace spln {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = SPL_PPO_NET_TILE_ROWS;  // rows of a workgroup of the forward and dZ launches
static_assert(kTileRows == 64, "a workgroup's four waves cover 64 rows as 2 x 2 or 1 x 1 tiles of 32 x 32");

__device__ __forceinline__ int d_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

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

// STAGE: the k of one stage, 32 for f32 operands and 64 for bf16
template <int MODE, int STAGE>
struct Shape {
    static constexpr bool kBytes = MODE == F1;                   // A is rebuilt from the store's bytes
    static constexpr bool kKMajor = MODE == Z2 || MODE == Z1;    // W is [k][unit]; otherwise [unit][k]
    static constexpr int kK = MODE == F1 ? kIn : MODE == Z2 ? kA : kH;
    static constexpr int kKp = (kK + STAGE - 1) / STAGE * STAGE; // whole stages: 320, 256, 64
    static constexpr int kUnits = MODE == F3 ? kA : kH;          // live units
    static constexpr int kNw = MODE == F3 ? 64 : kH;             // units of a workgroup
    static constexpr int kTm = MODE == F3 ? 1 : 2, kTn = kTm;    // a wave's tiles
    static constexpr bool kNeedOk = MODE == F1 || MODE == Z2;    // bad rows are zeros in A
    static constexpr int kWRegs = kNw * STAGE / kBlock;          // a thread's elements of a weight stage
    static constexpr bool kVec = kK % 4 == 0;                    // rows of A and of a [unit][k] W are 16-byte aligned
};
template <int MODE>
using Tiles = Shape<MODE, kTile>;  // for what does not depend on the stage

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

// The critic's dZ2: one product a row and unit, dvalue * w3[t] from zero, times 1 - H2^2; thread t the unit;
// float32.
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

// Where the sums start: the bias of the lane's unit u0 + 32 j + r (forward), or zero (dZ).
template <int MODE>
__device__ __forceinline__ void acc_start(const Gemm &g, int net, int u0, int r, f32x16 (&acc)[Tiles<MODE>::kTm][Tiles<MODE>::kTn]) {
    using S = Tiles<MODE>;
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
}

// The write-out of a wave's tiles: register q of tile (i, j) is row rt0 + 32 i + d_row(q, h), unit u0 + 32 j + r.
// tanh (F1, F2), the logits with a bad row's as zeros (F3), y * (1 - h^2) (Z2, Z1).
// kLoadFirst (dZ alone): a tile's activations are all loaded before its first store.  The planes may be one
// allocation, so a load behind a store waits for it: 32 round trips in a row.  The bf16 kernels load first; the
// f32 kernels do not, and whether they should is an OPEN performance question, to be settled by a measurement of
// its own: the bytes are the same either way.
template <int MODE, bool kLoadFirst>
__device__ __forceinline__ void tile_store(const Gemm &g, int net, int64_t b0, int rt0, int u0, int r, int h,
                                           const f32x16 (&acc)[Tiles<MODE>::kTm][Tiles<MODE>::kTn]) {
    using S = Tiles<MODE>;
    constexpr bool kDz = MODE == Z2 || MODE == Z1;
#pragma unroll
    for (int i = 0; i < S::kTm; ++i) {
        float hh[16][S::kTn];
        if constexpr (kDz && kLoadFirst) {
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
                    if constexpr (!kLoadFirst) hh[q][j] = g.h[net][bc * kH + u];
                    if (b < g.B) g.out[net][b * kH + u] = y * __builtin_fmaf(-hh[q][j], hh[q][j], 1.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the sums over rows: dW and db of every layer, per partial
// ---------------------------------------------------------------------------------------------
// A workgroup sums one block of one dW over the chunks p, p + parts, ... of its partial, a stage of rows at a
// time (zeros past a chunk's end), rows the MFMA's k.  The `wide` operand has 256 columns, 64 a wave; the
// `narrow` one 64, which every wave reads:
//   layer 1: dW1[m][n0 .. n0 + 63]: wide dZ1 (m), narrow X's columns (n), 5 blocks
//   layer 2: dW2[m][n0 .. n0 + 63]: wide dZ2 (m), narrow H1's columns (n), 4 blocks
//   layer 3: dW3[m < 45 | 1][n]:    wide H2 (n), narrow dOut (m), 1 block
constexpr int kDwBlocks = 5 + 4 + 1;  // a network's
constexpr int kNarrow = 64;

// The stages of chunks p, p + parts, ... in row order: chunk c's end, and from stage s0 of chunk c to the next
// (past the last chunk c >= g.chunks).
__device__ __forceinline__ int64_t end_of(const Bwd &g, int c) {
    const int64_t e = (int64_t)(c + 1) * kChunkRows;
    return e < g.B ? e : (int64_t)g.B;
}

__device__ __forceinline__ void next_stage(const Bwd &g, int stage_rows, int &c, int64_t &s0) {
    s0 += stage_rows;
    if (s0 >= end_of(g, c)) {
        c += g.parts;
        s0 = (int64_t)c * kChunkRows;
    }
}

// A dW block's place in partial `part`: the layer's matrix with its bias gradient as the last of nc columns, and
// its live rows
struct DwOut {
    float *out;
    int nc, m_live;
};

__device__ __forceinline__ DwOut dw_out(const Bwd &g, int layer, int net, int64_t part) {
    const int nc = layer == 1 ? kC1 : kC2, m_live = layer == 3 ? (net == 0 ? kA : 1) : kH;
    float *out = g.partial + part * kPartFloats + net * kActorFloats + (layer == 1 ? 0 : layer == 2 ? kOff2 : kOff3);
    return DwOut{out, nc, m_live};
}

// The write-out of a block's four tiles a wave: layers 1 and 2 units 64 wave .. + 63 by columns n0 .. + 63, layer 3
// the outputs by units 64 wave .. + 63
__device__ __forceinline__ void dw_store(int layer, const DwOut o, int n0, int wave, int r, int h, const f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = (layer == 3 ? 0 : 64 * wave) + 32 * i + d_row(q, h);
                const int n = (layer == 3 ? 64 * wave : n0) + 32 * j + r;
                if (m < o.m_live && n < o.nc - 1) o.out[m * o.nc + n] = acc[i][j][q];
            }
}

// ---------------------------------------------------------------------------------------------
// the launch sequences, over a family's kernels; `what` is the name a failed launch is reported under
// ---------------------------------------------------------------------------------------------
using GemmKernel = void (*)(Gemm);
using DwKernel = void (*)(Bwd);

inline int forward_tiles(int32_t B, const spl_ppo_net_fwd_t *a, void *stream, GemmKernel f1, GemmKernel f2, GemmKernel f3,
                         const char *what) {
    Fwd f;
    if (const int e = fwd_args(B, a, f)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]
    Gemm g{};
    g.B = B, g.total = f.total, g.idx = f.idx, g.obs = f.obs, g.errors = f.errors;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n) g.a[n] = nullptr, g.w[n] = f.net[n].w1, g.bias[n] = f.net[n].b1, g.out[n] = f.act + (2 * n) * slot;
    hipLaunchKernelGGL(f1, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = f.act + (2 * n) * slot, g.w[n] = f.net[n].w2, g.bias[n] = f.net[n].b2, g.out[n] = f.act + (2 * n + 1) * slot;
    hipLaunchKernelGGL(f2, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n) g.a[n] = f.act + (2 * n + 1) * slot, g.w[n] = f.net[n].w3, g.bias[n] = f.net[n].b3;
    g.out[0] = f.logits, g.out[1] = f.value;
    hipLaunchKernelGGL(f3, grid, block, 0, s, g);
    return spl_launched(what);
}

inline int backward_tiles(int32_t B, const spl_ppo_net_bwd_t *a, void *stream, GemmKernel z2, GemmKernel z1, DwKernel dw,
                          const char *what) {
    Bwd b;
    if (const int e = bwd_args(B, a, b)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]; dz: [network][dZ2, dZ1][B][256]
    Gemm g{};
    g.B = B, g.total = b.total, g.idx = b.idx, g.obs = b.obs;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dout[n], g.w[n] = b.w3[n], g.h[n] = b.act + (2 * n + 1) * slot, g.out[n] = b.dz + (2 * n) * slot;
    hipLaunchKernelGGL(z2, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dz + (2 * n) * slot, g.w[n] = b.w2[n], g.h[n] = b.act + (2 * n) * slot, g.out[n] = b.dz + (2 * n + 1) * slot;
    hipLaunchKernelGGL(z1, grid, block, 0, s, g);
    hipLaunchKernelGGL(dw, dim3(2 * kDwBlocks, b.parts), block, 0, s, b);
    launch_net_reduce(b, s);
    return spl_launched(what);
}

}  // namespace spln
