// spl_ppo_net_tiled.hip — spl_ppo_net_forward_tiled and spl_ppo_net_backward_tiled (include/splendor_ppo.h):
// the passes of spl_ppo_net.hip for large minibatches, as LDS-tiled GEMMs on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32) with the epilogues fused.  spl_ppo_net.hip takes 8 rows a workgroup through a
// whole network, so every 8 rows stream all the weights out of L2; here rows are blocked too, a workgroup
// takes SPL_PPO_NET_TILE_ROWS = 64 rows through ONE layer, and a weight element fetched once serves 64 rows.
//
// Same bytes as spl_ppo_net.hip.  The MFMA is, bit for bit, a k-ordered chain of fused multiply-adds from its
// C operand, and that is what the VALU kernels compute: every sum here starts where theirs starts (the bias,
// or zero), takes the same products in the same order (k ascending inside an instruction, instructions in k
// order) and is split over the same partials.  Where a tile is padded, the pad product is the one the VALU
// kernels add (+0 * +0 from K = 297 to 320 and past a chunk's last row), or, where they add none (the 45
// outputs up to 64), -0 * +0, which leaves every accumulator, -0 included, as it is.
//
// Launches: forward 3 (layer 1, layer 2, the output layers), backward 4 (dZ2, dZ1, the sums over rows, the
// ordered combination of the partials).  Operand and C/D lane maps of the 32x32x2 form, lane l, r = l & 31,
// h = l >> 5: A[i = r][k = h], B[k = h][j = r], D[i = (q & 3) + 8 (q >> 2) + 4 h][j = r] in register q.
#include "spl_ppo_net_common.h"

namespace spln {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = SPL_PPO_NET_TILE_ROWS;  // rows of a workgroup of the forward and dZ launches
constexpr int kLd = kTile + 1;                    // row stride of a [..][32] stage in LDS: no bank conflict
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

template <int MODE>
struct Shape {
    static constexpr bool kBytes = MODE == F1;                   // A is rebuilt from the store's bytes
    static constexpr bool kKMajor = MODE == Z2 || MODE == Z1;    // W is [k][unit]; otherwise [unit][k]
    static constexpr int kK = MODE == F1 ? kIn : MODE == Z2 ? kA : kH;
    static constexpr int kKp = (kK + kTile - 1) / kTile * kTile; // whole stages: 320, 256, 64
    static constexpr int kUnits = MODE == F3 ? kA : kH;          // live units
    static constexpr int kNw = MODE == F3 ? 64 : kH;             // units of a workgroup
    static constexpr int kTm = MODE == F3 ? 1 : 2, kTn = kTm;    // a wave's tiles
    static constexpr bool kNeedOk = MODE == F1 || MODE == Z2;    // bad rows are zeros in A
    static constexpr int kWRegs = kNw * kTile / kBlock;          // a thread's elements of a weight stage
};

// The critic's output layer: row b's value = b3 + SUM_k H2[b][k] w3[k], k ascending, a thread a row.
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

// The critic's dZ2: one product a row and unit, dvalue * w3[t] from zero, times 1 - H2^2; thread t the unit.
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

// grid (row tiles, 2): blockIdx.y 0 the actor, 1 the critic
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_tiled_gemm(Gemm g) {
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
    __shared__ float as[kTileRows * kLd];                                        // [row][k]
    __shared__ float ws[S::kKMajor ? kTile * kH : S::kNw * kLd];                 // [unit][k] or [k][unit]
    const int col = t & 31, rw = t >> 5;        // what this thread stages: column k0 + col of rows rw + 8 i
    const int lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int rt0 = S::kTm == 2 ? 0 : 32 * (wave >> 1);   // the wave's rows and units inside the workgroup's
    const int u0 = S::kTm == 2 ? 64 * wave : 32 * (wave & 1);
    const float *__restrict__ A = g.a[net];
    const float *__restrict__ W = g.w[net];

    // The rows this thread stages.  No load sits behind a per-lane branch: a row past B reads row B - 1, a
    // bad row reads position 0 (which every store has), and the value is replaced afterwards; the address of
    // a bad position is never formed.
    int64_t rowc[8];
    const uint8_t *src[8];
    uint32_t hi[8];
    unsigned okm = 0xffu;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t b = b0 + rw + 8 * i;
        rowc[i] = b < g.B ? b : (int64_t)g.B - 1;
    }
    if constexpr (S::kNeedOk) {
        int n_bad = 0;
        okm = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t pos = g.idx[rowc[i]];
            const bool ok = pos >= 0 && pos < g.total;
            okm |= (ok ? 1u : 0u) << i;
            n_bad += (!ok && b0 + rw + 8 * i < g.B) ? 1 : 0;
            if constexpr (S::kBytes) src[i] = g.obs + (ok ? pos : 0) * SPL_PPO_OBS_U8;
        }
        if constexpr (S::kBytes) {
#pragma unroll
            for (int i = 0; i < 8; ++i) hi[i] = src[i][297];
            if (net == 0 && col == 0 && n_bad) atomicAdd(g.errors, (unsigned long long)n_bad);  // a row once
        }
    }

    float an[8], wn[S::kWRegs];  // the next stage, on its way while this one is summed
    auto fetch = [&](int k0) {
        const int k = k0 + col, kc = k < S::kK ? k : S::kK - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = (okm >> i) & 1u;
            if constexpr (S::kBytes) {
                const uint32_t v = src[i][kc];
                const uint32_t x = v + (k == 295 ? hi[i] << 8 : 0u);
                an[i] = (ok && k < S::kK) ? (float)x : 0.f;
            } else {
                const float v = A[rowc[i] * S::kK + kc];
                // past K (the 45 outputs alone): -0, whose product with the weight stage's +0 changes no sum
                an[i] = k < S::kK ? (ok ? v : 0.f) : -0.f;
            }
        }
        if constexpr (S::kKMajor) {  // thread t the unit, 32 rows of k
#pragma unroll
            for (int i = 0; i < S::kWRegs; ++i) {
                const int kk = k0 + i;
                const float v = W[(uint32_t)((kk < S::kK ? kk : S::kK - 1) * kH + t)];
                wn[i] = kk < S::kK ? v : 0.f;
            }
        } else {  // lanes along k: rows are only dword-aligned
#pragma unroll
            for (int i = 0; i < S::kWRegs; ++i) {
                const int u = rw + 8 * i;
                const float v = W[(uint32_t)((u < S::kUnits ? u : S::kUnits - 1) * S::kK + kc)];
                wn[i] = (k < S::kK && u < S::kUnits) ? v : 0.f;
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

    for (int k0 = 0; k0 < S::kKp; k0 += kTile) {
        __syncthreads();  // the stage's readers are done
#pragma unroll
        for (int i = 0; i < 8; ++i) as[(rw + 8 * i) * kLd + col] = an[i];
#pragma unroll
        for (int i = 0; i < S::kWRegs; ++i) {
            if constexpr (S::kKMajor) ws[i * kH + t] = wn[i];
            else ws[(rw + 8 * i) * kLd + col] = wn[i];
        }
        __syncthreads();
        if (k0 + kTile < S::kKp) fetch(k0 + kTile);
        auto step = [&](int s) {
            const int kk = 2 * s + h;
            float av[S::kTm], bv[S::kTn];
#pragma unroll
            for (int i = 0; i < S::kTm; ++i) av[i] = as[(rt0 + 32 * i + r) * kLd + kk];
#pragma unroll
            for (int j = 0; j < S::kTn; ++j)
                bv[j] = S::kKMajor ? ws[kk * kH + u0 + 32 * j + r] : ws[(u0 + 32 * j + r) * kLd + kk];
#pragma unroll
            for (int i = 0; i < S::kTm; ++i)
#pragma unroll
                for (int j = 0; j < S::kTn; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        };
#pragma unroll 4
        for (int s = 0; s < kTile / 2; ++s) step(s);
    }

    // epilogue: register q of tile (i, j) is row rt0 + 32 i + d_row(q, h), unit u0 + 32 j + r
#pragma unroll
    for (int i = 0; i < S::kTm; ++i) {
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
                    const float hh = g.h[net][bc * kH + u];
                    if (b < g.B) g.out[net][b * kH + u] = y * __builtin_fmaf(-hh, hh, 1.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the sums over rows: dW and db of every layer, per partial
// ---------------------------------------------------------------------------------------------
// A workgroup sums one block of one dW over the chunks p, p + parts, ... of its partial, 32 rows a stage as
// k_net_dw does (zeros past a chunk's end), rows the MFMA's k.  Both operands lie [row][column] in memory and
// in LDS.  The `wide` one has 256 columns, 64 a wave; the `narrow` one 64, which every wave reads:
//   layer 1: dW1[m][n0 .. n0 + 63]: wide dZ1 (m), narrow X's columns (n), 5 blocks
//   layer 2: dW2[m][n0 .. n0 + 63]: wide dZ2 (m), narrow H1's columns (n), 4 blocks
//   layer 3: dW3[m < 45 | 1][n]:    wide H2 (n), narrow dOut (m), 1 block
// The bias gradient, the column against ones, is fma(a, 1, sum) down the same rows on the VALU: the same bits.
constexpr int kDwBlocks = 5 + 4 + 1;  // a network's
constexpr int kNarrow = 64;

__global__ __launch_bounds__(kBlock) void k_tiled_dw(Bwd g) {
    __shared__ float lds[kTile * (kH + kNarrow)];
    float *const wide_s = lds, *const narrow_s = lds + kTile * kH;
    const int t = threadIdx.x, net = blockIdx.x / kDwBlocks, y = blockIdx.x % kDwBlocks;
    const int layer = y < 5 ? 1 : y < 9 ? 2 : 3;
    const int n0 = layer == 1 ? kNarrow * y : layer == 2 ? kNarrow * (y - 5) : 0;
    const int n3 = net == 0 ? kA : 1;
    const int lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int ncol = t & 63, nrow = t >> 6;  // what this thread stages of the narrow operand: rows nrow + 4 i
    const float *wide = layer == 1   ? g.dz + (int64_t)(net * 2 + 1) * g.B * kH
                        : layer == 2 ? g.dz + (int64_t)(net * 2 + 0) * g.B * kH
                                     : g.act + (int64_t)(net * 2 + 1) * g.B * kH;
    const float *h1 = g.act + (int64_t)(net * 2 + 0) * g.B * kH;
    const float *dout = g.dout[net];

    float wn[kTile], nn[8];
    // No load sits behind a per-lane branch (the layer is uniform over the workgroup): a row past `end` reads
    // row end - 1, a column past the matrix its last one, a bad row position 0, and the value is then
    // replaced; the address of a bad position is never formed.
    auto fetch = [&](int64_t s0, int64_t end) {
        const float *wrow = wide + s0 * kH + t;
        const int live_rows = (int)(end - s0);  // >= 1
#pragma unroll
        for (int i = 0; i < kTile; ++i) {
            const float v = wrow[(i < live_rows ? i : live_rows - 1) * kH];
            wn[i] = i < live_rows ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t b = s0 + nrow + 4 * i;
            const bool live = b < end;
            const int64_t bc = live ? b : end - 1;
            float x;
            if (layer == 2) {
                x = h1[bc * kH + n0 + ncol];
            } else {
                int64_t pos = g.idx[bc];
                const bool ok = pos >= 0 && pos < g.total;
                pos = ok ? pos : 0;
                if (layer == 1) {
                    const int n = n0 + ncol;
                    const uint8_t *row = g.obs + pos * SPL_PPO_OBS_U8;
                    const uint32_t v = row[n < kIn ? n : kIn - 1], hi = row[297];
                    x = (float)(v + (n == 295 ? hi << 8 : 0u));
                    x = (ok && n < kIn) ? x : 0.f;
                } else {
                    x = dout[bc * n3 + (ncol < n3 ? ncol : n3 - 1)];
                    x = (ok && ncol < n3) ? x : 0.f;
                }
            }
            nn[i] = live ? x : 0.f;
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
    // the bias gradient's unit: layers 1 and 2 the wide column t (the block at n0 = 0 alone), layer 3 the
    // narrow column t < 64
    const bool has_bias = layer == 3 ? t < kNarrow : n0 == 0;
    const float *bias_s = layer == 3 ? narrow_s + (t & 63) : wide_s + t;
    const int bias_ld = layer == 3 ? kNarrow : kH;
    float bsum = 0.f;
    // The MFMA's A operand is the units (m), its B operand the columns (n): the wide and the narrow stage in
    // layers 1 and 2, the other way round in layer 3.  This lane's element of tile 0 at k = 0, and the stride of k:
    const float *const wide_l = wide_s + 64 * wave + r, *const narrow_l = narrow_s + r;
    const float *const a_s = layer == 3 ? narrow_l : wide_l, *const b_s = layer == 3 ? wide_l : narrow_l;
    const int a_ld = layer == 3 ? kNarrow : kH, b_ld = layer == 3 ? kH : kNarrow;

    // the stages of chunks p, p + parts, ... in row order; the next one is fetched while this one is summed
    int c = blockIdx.y;
    int64_t s0 = (int64_t)c * kChunkRows;
    bool more = c < g.chunks;
    if (more) fetch(s0, end_of(c));
    while (more) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kTile; ++i) wide_s[i * kH + t] = wn[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) narrow_s[(nrow + 4 * i) * kNarrow + ncol] = nn[i];
        __syncthreads();
        s0 += kTile;
        if (s0 >= end_of(c)) {
            c += g.parts;
            s0 = (int64_t)c * kChunkRows;
        }
        more = c < g.chunks;
        if (more) fetch(s0, end_of(c));
#pragma unroll 4
        for (int s = 0; s < kTile / 2; ++s) {
            const int kk = 2 * s + h;
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = a_s[kk * a_ld + 32 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = b_s[kk * b_ld + 32 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (has_bias) {
#pragma unroll 8
            for (int rr = 0; rr < kTile; ++rr) bsum = __builtin_fmaf(bias_s[rr * bias_ld], 1.f, bsum);
        }
    }

    const int nc = layer == 1 ? kC1 : kC2;
    const int m_live = layer == 3 ? n3 : kH;
    float *out = g.partial + (int64_t)blockIdx.y * kPartFloats + net * kActorFloats + (layer == 1 ? 0 : layer == 2 ? kOff2 : kOff3);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = (layer == 3 ? 0 : 64 * wave) + 32 * i + d_row(q, h);
                const int n = (layer == 3 ? 64 * wave : n0) + 32 * j + r;
                if (m < m_live && n < nc - 1) out[m * nc + n] = acc[i][j][q];
            }
    if (has_bias && t < m_live) out[t * nc + nc - 1] = bsum;
}

}  // namespace spln

using namespace spln;

extern "C" {

int spl_ppo_net_forward_tiled(int32_t B, const spl_ppo_net_fwd_t *a, void *stream) {
    Fwd f;
    if (const int e = fwd_args(B, a, f)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]
    Gemm g{};
    g.B = B, g.total = f.total, g.idx = f.idx, g.obs = f.obs, g.errors = f.errors;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n) g.a[n] = nullptr, g.w[n] = f.net[n].w1, g.bias[n] = f.net[n].b1, g.out[n] = f.act + (2 * n) * slot;
    hipLaunchKernelGGL(k_tiled_gemm<F1>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = f.act + (2 * n) * slot, g.w[n] = f.net[n].w2, g.bias[n] = f.net[n].b2, g.out[n] = f.act + (2 * n + 1) * slot;
    hipLaunchKernelGGL(k_tiled_gemm<F2>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n) g.a[n] = f.act + (2 * n + 1) * slot, g.w[n] = f.net[n].w3, g.bias[n] = f.net[n].b3;
    g.out[0] = f.logits, g.out[1] = f.value;
    hipLaunchKernelGGL(k_tiled_gemm<F3>, grid, block, 0, s, g);
    return spl_launched("k_tiled_gemm (forward)");
}

int spl_ppo_net_backward_tiled(int32_t B, const spl_ppo_net_bwd_t *a, void *stream) {
    Bwd b;
    if (const int e = bwd_args(B, a, b)) return e;
    const int64_t slot = (int64_t)B * kH;  // act: [network][layer][B][256]; dz: [network][dZ2, dZ1][B][256]
    Gemm g{};
    g.B = B, g.total = b.total, g.idx = b.idx, g.obs = b.obs;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kTileRows - 1) / kTileRows), 2), block(kBlock);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dout[n], g.w[n] = b.w3[n], g.h[n] = b.act + (2 * n + 1) * slot, g.out[n] = b.dz + (2 * n) * slot;
    hipLaunchKernelGGL(k_tiled_gemm<Z2>, grid, block, 0, s, g);
    for (int n = 0; n < 2; ++n)
        g.a[n] = b.dz + (2 * n) * slot, g.w[n] = b.w2[n], g.h[n] = b.act + (2 * n) * slot, g.out[n] = b.dz + (2 * n + 1) * slot;
    hipLaunchKernelGGL(k_tiled_gemm<Z1>, grid, block, 0, s, g);
    hipLaunchKernelGGL(k_tiled_dw, dim3(2 * kDwBlocks, b.parts), block, 0, s, b);
    launch_net_reduce(b, s);
    return spl_launched("k_tiled_gemm (backward)");
}

}  // extern "C"
