// spl_ppo_net_tiled.hip — spl_ppo_net_forward_tiled and spl_ppo_net_backward_tiled (include/splendor_ppo.h):
// the passes of spl_ppo_net.hip for large minibatches, as LDS-tiled GEMMs on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32) with the epilogues fused.  spl_ppo_net.hip takes 8 rows a workgroup through a
// whole network, so every 8 rows stream all the weights out of L2; here rows are blocked too, a workgroup
// takes SPL_PPO_NET_TILE_ROWS = 64 rows through ONE layer, and a weight element fetched once serves 64 rows.
// What a tile is apart from its operands (shapes, epilogues, the partials' write-out, the launches) is
// spl_ppo_net_tile.h's, shared with the bf16 source; here are the f32 stages and the matrix-instruction loops.
//
// Same bytes as spl_ppo_net.hip.  The MFMA is, bit for bit, a k-ordered chain of fused multiply-adds from its
// C operand, and that is what the VALU kernels compute: every sum here starts where theirs starts (the bias,
// or zero), takes the same products in the same order (k ascending inside an instruction, instructions in k
// order) and is split over the same partials.  Where a tile is padded, the pad product is the one the VALU
// kernels add (+0 * +0 from K = 297 to 320 and past a chunk's last row), or, where they add none (the 45
// outputs up to 64), -0 * +0, which leaves every accumulator, -0 included, as it is.
//
// Operand lane map of the 32x32x2 form, lane l, r = l & 31, h = l >> 5: A[i = r][k = h], B[k = h][j = r].
#include "spl_ppo_net_tile.h"

namespace spln {

constexpr int kLd = kTile + 1;  // row stride of a [..][32] stage in LDS: no bank conflict

// grid (row tiles, 2): blockIdx.y 0 the actor, 1 the critic
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_tiled_gemm(Gemm g) {
    using S = Shape<MODE, kTile>;
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
    acc_start<MODE>(g, net, u0, r, acc);

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

    tile_store<MODE, false>(g, net, b0, rt0, u0, r, h, acc);
}

// ---------------------------------------------------------------------------------------------
// the sums over rows: dW and db of every layer, per partial
// ---------------------------------------------------------------------------------------------
// The stages are 32 rows as k_net_dw's are; both operands lie [row][column] in memory and in LDS (the blocks:
// spl_ppo_net_tile.h).  The bias gradient, the column against ones, is fma(a, 1, sum) down the same rows on the
// VALU: the same bits.
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
    if (more) fetch(s0, end_of(g, c));
    while (more) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kTile; ++i) wide_s[i * kH + t] = wn[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) narrow_s[(nrow + 4 * i) * kNarrow + ncol] = nn[i];
        __syncthreads();
        next_stage(g, kTile, c, s0);
        more = c < g.chunks;
        if (more) fetch(s0, end_of(g, c));
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

    const DwOut o = dw_out(g, layer, net, blockIdx.y);
    dw_store(layer, o, n0, wave, r, h, acc);
    if (has_bias && t < o.m_live) o.out[t * o.nc + o.nc - 1] = bsum;
}

}  // namespace spln

using namespace spln;

extern "C" {

int spl_ppo_net_forward_tiled(int32_t B, const spl_ppo_net_fwd_t *a, void *stream) {
    return forward_tiles(B, a, stream, k_tiled_gemm<F1>, k_tiled_gemm<F2>, k_tiled_gemm<F3>, "k_tiled_gemm (forward)");
}

int spl_ppo_net_backward_tiled(int32_t B, const spl_ppo_net_bwd_t *a, void *stream) {
    return backward_tiles(B, a, stream, k_tiled_gemm<Z2>, k_tiled_gemm<Z1>, k_tiled_dw, "k_tiled_gemm (backward)");
}

}  // extern "C"
