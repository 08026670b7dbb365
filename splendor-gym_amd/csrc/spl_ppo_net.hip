// spl_ppo_net.hip — the two networks of the PPO update (include/splendor_ppo.h): spl_ppo_net_forward and
// spl_ppo_net_backward, the actor's and the critic's 297 -> 256 -> 256 -> (45 | 1) tanh MLPs around the loss
// head, float32 throughout.
//
// Arithmetic: plain fused multiply-adds on the VALU (__builtin_fmaf chains in a fixed order), not the
// f32-input MFMA.  Both run at the same rate on this chip and give the same bits for a k-ordered chain; a
// minibatch of 256 is 0.5 GFLOP forward and backward, microseconds either way, and what bounds the calls
// is their launches and the 1.18 MB of weights every workgroup streams out of L2.  The VALU form needs no
// operand layout, so the same loops serve the 45- and the 1-unit output layers and every ragged edge.
//
// Launches: forward 1, backward 3 (dZ, the tiled sums over rows, the ordered combination of the partials).
#include "spl_ppo_net_common.h"

namespace spln {

constexpr int kRows = SPL_PPO_NET_FWD_ROWS;
constexpr int kXStride = 320;              // an input row in LDS: 297 columns and zeros up to 10 stages of 32
static_assert(kRows % 2 == 0 && (kRows / 2) * kA <= kBlock, "the output layer is one pass of row pairs");

// tiles of launch 2 of the backward (a dW tile is 32 x 32, a weight stage 256 x 32), per network: layer 1,
// layer 2, layer 3
constexpr int kNt1 = (kC1 + kTile - 1) / kTile, kNt2 = (kC2 + kTile - 1) / kTile;  // 10, 9
constexpr int kT1 = (kH / kTile) * kNt1, kT2 = (kH / kTile) * kNt2;                 // 80, 72
constexpr int kT3a = ((kA + kTile - 1) / kTile) * kNt2, kT3c = kNt2;                // 18, 9
constexpr int kActorTiles = kT1 + kT2 + kT3a, kTiles = kActorTiles + kT1 + kT2 + kT3c;  // 170, 331

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// acc[r] = bias[t] + SUM_k in[r][k] W[t][k], k ascending, for the workgroup's kRows rows and thread t's unit.
// W [256][KD] is only dword-aligned per row, so it comes in 256 x 32 stages through LDS: lanes along k for
// the load (128-byte runs), a row stride of 33 so that the stage is written and read without a bank conflict.
// `in` rows hold zeros from KD up to the next multiple of 32 and the stage holds zeros there too.
// The stage after the one being summed is already on its way into registers (`next`), so a workgroup,
// alone on its CU at B = 256, waits for L2 once per layer, not once per stage.
constexpr int kStageRegs = kH / 8;  // a thread's 32 elements of a stage: rows t / 32 + 8 i, column t % 32

template <int KD>
__device__ __forceinline__ void load_stage(const float *__restrict__ W, int k0, float (&next)[kStageRegs]) {
    // every load is issued whatever k is (a column past the row's end reads the row's last element, and
    // dense() puts a zero in its place): a branch here would make the 32 loads wait for one another
    const int k = k0 + (threadIdx.x & 31);
    const uint32_t at = (threadIdx.x >> 5) * KD + (k < KD ? k : KD - 1);  // unsigned: one 32-bit add a load
#pragma unroll
    for (int i = 0; i < kStageRegs; ++i) next[i] = W[at + (uint32_t)(8 * i * KD)];
}

// `next` holds stage 0 on entry (the caller loads it as early as it can)
template <int KD, int STRIDE>
__device__ __forceinline__ void dense(const float *__restrict__ W, const float *__restrict__ bias, const float *in,
                                      float (*wt)[kTile + 1], float (&next)[kStageRegs], float (&acc)[kRows]) {
    const int t = threadIdx.x, col = t & 31, row0 = t >> 5;
    const float bj = bias[t];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = bj;
    for (int k0 = 0; k0 < KD; k0 += kTile) {
        __syncthreads();  // the stage's readers are done (first pass: `in` is written)
#pragma unroll
        for (int i = 0; i < kStageRegs; ++i) wt[row0 + 8 * i][col] = k0 + col < KD ? next[i] : 0.f;
        __syncthreads();
        if (k0 + kTile < KD) load_stage<KD>(W, k0 + kTile, next);
#pragma unroll
        for (int kk = 0; kk < kTile; kk += 4) {
            const float w0 = wt[t][kk], w1 = wt[t][kk + 1], w2 = wt[t][kk + 2], w3 = wt[t][kk + 3];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const float4 x = *reinterpret_cast<const float4 *>(in + r * STRIDE + k0 + kk);
                acc[r] = __builtin_fmaf(x.x, w0, acc[r]);
                acc[r] = __builtin_fmaf(x.y, w1, acc[r]);
                acc[r] = __builtin_fmaf(x.z, w2, acc[r]);
                acc[r] = __builtin_fmaf(x.w, w3, acc[r]);
            }
        }
    }
}

// grid (row tiles, 2): blockIdx.y 0 the actor, 1 the critic
__global__ __launch_bounds__(kBlock) void k_net_forward(Fwd f) {
    __shared__ __align__(16) float xs[kRows][kXStride];  // the inputs, later the second hidden layer
    __shared__ __align__(16) float hs[kRows][kH];        // the first hidden layer
    __shared__ float wt[kH][kTile + 1];
    __shared__ int bad[kRows];
    const int t = threadIdx.x, net = blockIdx.y;
    const int64_t b0 = (int64_t)blockIdx.x * kRows;
    const Mlp m = f.net[net];
    int n_bad = 0;
    float next[kStageRegs];
    load_stage<kIn>(m.w1, 0, next);
    // The rows' bytes: every load is issued before any is waited for, so none sits behind a branch.  A row
    // past B reads row B - 1's position and a bad row reads position 0 (which every store has) in its place;
    // both are then replaced by zeros, and the address of a bad position is never formed.
    const uint8_t *src[kRows];
    bool ok[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int64_t b = b0 + r;
        const int64_t pos = f.idx[b < f.B ? b : (int64_t)f.B - 1];
        ok[r] = b < f.B && pos >= 0 && pos < f.total;  // uniform over the workgroup
        src[r] = f.obs + (ok[r] ? pos : 0) * SPL_PPO_OBS_U8;
        n_bad += (b < f.B && !ok[r]) ? 1 : 0;
    }
    const int c1 = t + kBlock < kIn ? t + kBlock : kIn - 1;  // t < 256 <= 296 needs no clamp
    uint32_t v0[kRows], v1[kRows], hi[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        v0[r] = src[r][t];
        v1[r] = src[r][c1];
        hi[r] = src[r][297];
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        if (t == 0) bad[r] = ok[r] ? 0 : 1;
        xs[r][t] = ok[r] ? (float)v0[r] : 0.f;
        if (t < kXStride - kBlock) {
            const int c = t + kBlock;  // 256 .. 319: column 295 is here
            const uint32_t x = v1[r] + (c == 295 ? hi[r] << 8 : 0u);
            xs[r][c] = (ok[r] && c < kIn) ? (float)x : 0.f;
        }
    }
    if (net == 0 && t == 0 && n_bad) atomicAdd(f.errors, (unsigned long long)n_bad);

    float acc[kRows];
    dense<kIn, kXStride>(m.w1, m.b1, &xs[0][0], wt, next, acc);
    load_stage<kH>(m.w2, 0, next);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const float h = tanh_acc(acc[r]);
        hs[r][t] = h;
        if (b0 + r < f.B) f.act[((int64_t)(net * 2 + 0) * f.B + b0 + r) * kH + t] = h;
    }
    dense<kH, kH>(m.w2, m.b2, &hs[0][0], wt, next, acc);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const float h = tanh_acc(acc[r]);
        xs[r][t] = h;  // the inputs were last read in layer 1, barriers ago
        if (b0 + r < f.B) f.act[((int64_t)(net * 2 + 1) * f.B + b0 + r) * kH + t] = h;
    }
    __syncthreads();
    // the output layer: a thread takes unit o for rows 2 rp and 2 rp + 1 (180 threads for the actor), each a
    // 256-long chain from b3[o] over one pass through W3's row o (1 KiB, 16-byte aligned), 16 loads in flight
    const int n3 = net == 0 ? kA : 1;
    if (t < (kRows / 2) * n3) {
        const int rp = t / n3, o = t - rp * n3;
        const float4 *w = reinterpret_cast<const float4 *>(m.w3 + o * kH);
        const float4 *h0 = reinterpret_cast<const float4 *>(&xs[2 * rp][0]);
        const float4 *h1 = reinterpret_cast<const float4 *>(&xs[2 * rp + 1][0]);
        float y0 = m.b3[o], y1 = y0;
#pragma unroll 16
        for (int k = 0; k < kH / 4; ++k) {
            const float4 c = w[k], a0 = h0[k], a1 = h1[k];
            y0 = __builtin_fmaf(a0.x, c.x, y0);
            y1 = __builtin_fmaf(a1.x, c.x, y1);
            y0 = __builtin_fmaf(a0.y, c.y, y0);
            y1 = __builtin_fmaf(a1.y, c.y, y1);
            y0 = __builtin_fmaf(a0.z, c.z, y0);
            y1 = __builtin_fmaf(a1.z, c.z, y1);
            y0 = __builtin_fmaf(a0.w, c.w, y0);
            y1 = __builtin_fmaf(a1.w, c.w, y1);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = 2 * rp + i;
            const int64_t b = b0 + r;
            if (b >= f.B) continue;
            const float y = bad[r] ? 0.f : (i ? y1 : y0);
            if (net == 0) f.logits[b * kA + o] = y;
            else f.value[b] = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool good_row(const Bwd &g, int64_t b, int64_t &pos) {
    if (b >= g.B) return false;
    pos = g.idx[b];
    return pos >= 0 && pos < g.total;
}

// Launch 1, grid (row tiles, 2): dZ2 and dZ1 of kRows rows, thread t the hidden unit.  Both products walk
// the weight's rows, so lanes read 1 KiB runs of W3 and W2 as they lie; a bad row's dOut counts as zeros.
__global__ __launch_bounds__(kBlock) void k_net_dz(Bwd g) {
    __shared__ float ds[kRows][48];
    __shared__ __align__(16) float z2[kRows][kH];
    const int t = threadIdx.x, net = blockIdx.y, n3 = net == 0 ? kA : 1;
    const int64_t b0 = (int64_t)blockIdx.x * kRows;
    for (int e = t; e < kRows * 48; e += kBlock) {
        const int r = e / 48, o = e - r * 48;
        int64_t pos;
        ds[r][o] = (o < n3 && good_row(g, b0 + r, pos)) ? g.dout[net][(b0 + r) * n3 + o] : 0.f;
    }
    __syncthreads();
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
    const float *w3 = g.w3[net];
    for (int o = 0; o < n3; ++o) {
        const float w = w3[o * kH + t];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = __builtin_fmaf(ds[r][o], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        float z = 0.f;
        if (b0 + r < g.B) {
            const float h = g.act[((int64_t)(net * 2 + 1) * g.B + b0 + r) * kH + t];
            z = acc[r] * __builtin_fmaf(-h, h, 1.f);
            g.dz[((int64_t)(net * 2 + 0) * g.B + b0 + r) * kH + t] = z;
        }
        z2[r][t] = z;
        acc[r] = 0.f;
    }
    __syncthreads();
    const float *w2 = g.w2[net];
#pragma unroll 2
    for (int j = 0; j < kH; j += 4) {
        const float w0 = w2[(j + 0) * kH + t], w1 = w2[(j + 1) * kH + t], w2_ = w2[(j + 2) * kH + t], w3_ = w2[(j + 3) * kH + t];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const float4 z = *reinterpret_cast<const float4 *>(&z2[r][j]);
            acc[r] = __builtin_fmaf(z.x, w0, acc[r]);
            acc[r] = __builtin_fmaf(z.y, w1, acc[r]);
            acc[r] = __builtin_fmaf(z.z, w2_, acc[r]);
            acc[r] = __builtin_fmaf(z.w, w3_, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        if (b0 + r < g.B) {
            const float h = g.act[((int64_t)(net * 2 + 0) * g.B + b0 + r) * kH + t];
            g.dz[((int64_t)(net * 2 + 1) * g.B + b0 + r) * kH + t] = acc[r] * __builtin_fmaf(-h, h, 1.f);
        }
    }
}

// which tile of which matrix blockIdx.x is
struct TileOf {
    int net, layer, m0, n0;  // layer 1..3
    int M, NC;               // rows of dW (units), augmented columns
    int off;                 // the matrix inside a partial
};

__device__ __forceinline__ TileOf tile_of(int x) {
    TileOf q;
    q.net = x >= kActorTiles ? 1 : 0;
    int y = x - q.net * kActorTiles;
    const int base = q.net * kActorFloats;
    if (y < kT1) {
        q.layer = 1, q.M = kH, q.NC = kC1, q.off = base;
        q.m0 = (y / kNt1) * kTile, q.n0 = (y % kNt1) * kTile;
    } else if (y < kT1 + kT2) {
        y -= kT1;
        q.layer = 2, q.M = kH, q.NC = kC2, q.off = base + kOff2;
        q.m0 = (y / kNt2) * kTile, q.n0 = (y % kNt2) * kTile;
    } else {
        y -= kT1 + kT2;
        q.layer = 3, q.M = q.net == 0 ? kA : 1, q.NC = kC2, q.off = base + kOff3;
        q.m0 = (y / kNt2) * kTile, q.n0 = (y % kNt2) * kTile;
    }
    return q;
}

// Launch 2, grid (kTiles, parts): one 32 x 32 tile of one dW (its last column the bias gradient) over the
// chunks p, p + parts, ... of kChunkRows rows, row by row.  32 rows at a time go through LDS: thread
// (t / 32, t % 32) keeps units 4 (t / 32) .. + 3 against column t % 32.
__global__ __launch_bounds__(kBlock) void k_net_dw(Bwd g) {
    __shared__ __align__(16) float a_s[kTile][kTile];  // [row][unit]: dOut, dZ2 or dZ1
    __shared__ float c_s[kTile][kTile];                // [row][column]: H2, H1 or X, and the ones
    const TileOf q = tile_of(blockIdx.x);
    const int t = threadIdx.x, col = t & 31, mg = t >> 5, net = q.net;
    const int m = q.m0 + col, n = q.n0 + col;  // what this thread stages
    const int n3 = net == 0 ? kA : 1;
    const float *zsrc = q.layer == 3 ? nullptr : g.dz + (int64_t)(net * 2 + (q.layer == 2 ? 0 : 1)) * g.B * kH;
    const float *hsrc = q.layer == 1 ? nullptr : g.act + (int64_t)(net * 2 + (q.layer == 3 ? 1 : 0)) * g.B * kH;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    // this thread's four elements of each side of the stage at rows s0 .. s0 + 31 (below `end`); zeros elsewhere
    float a_n[kTile / 8], x_n[kTile / 8];
    auto fetch = [&](int64_t s0, int64_t end) {
#pragma unroll
        // No load sits behind a per-lane branch (the layer is uniform over the workgroup): a row past `end`
        // reads row end - 1, a unit or column past the matrix its last one, a bad row position 0, and the
        // value is then replaced; the address of a bad position is never formed.
        for (int i = 0; i < kTile / 8; ++i) {
            const int64_t b = s0 + mg + 8 * i;
            const bool live = b < end;
            const int64_t bc = live ? b : end - 1;
            bool ok = true;
            int64_t pos = 0;
            if (q.layer != 2) {  // layer 2 reads scratch and activations alone
                pos = g.idx[bc];
                ok = pos >= 0 && pos < g.total;
                pos = ok ? pos : 0;
            }
            float a, x;
            if (q.layer == 3) {
                a = g.dout[net][bc * n3 + (m < q.M ? m : q.M - 1)];
                a = (live && ok && m < q.M) ? a : 0.f;
            } else {
                a = zsrc[bc * kH + m];  // m < 256 = M
                a = live ? a : 0.f;
            }
            if (q.layer == 1) {
                const uint8_t *row = g.obs + pos * SPL_PPO_OBS_U8;
                const uint32_t v = row[n < kIn ? n : kIn - 1], hi = row[297];
                x = (float)(v + (n == 295 ? hi << 8 : 0u));
                x = ok ? x : 0.f;
            } else {
                x = hsrc[bc * kH + (n < kH ? n : kH - 1)];
            }
            x = n < q.NC - 1 ? x : n == q.NC - 1 ? 1.f : 0.f;
            a_n[i] = a;
            x_n[i] = live ? x : 0.f;
        }
    };
    auto end_of = [&](int c) {
        const int64_t e = (int64_t)(c + 1) * kChunkRows;
        return e < g.B ? e : (int64_t)g.B;
    };
    // the stages of chunks p, p + parts, ... in row order; the next one is fetched while this one is summed
    int c = blockIdx.y;
    int64_t s0 = (int64_t)c * kChunkRows;
    bool more = c < g.chunks;
    if (more) fetch(s0, end_of(c));
    while (more) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kTile / 8; ++i) {
            a_s[mg + 8 * i][col] = a_n[i];
            c_s[mg + 8 * i][col] = x_n[i];
        }
        __syncthreads();
        s0 += kTile;
        if (s0 >= end_of(c)) {
            c += g.parts;
            s0 = (int64_t)c * kChunkRows;
        }
        more = c < g.chunks;
        if (more) fetch(s0, end_of(c));
#pragma unroll 8
        for (int r = 0; r < kTile; ++r) {
            const float4 a = *reinterpret_cast<const float4 *>(&a_s[r][4 * mg]);
            const float x = c_s[r][col];
            acc[0] = __builtin_fmaf(a.x, x, acc[0]);
            acc[1] = __builtin_fmaf(a.y, x, acc[1]);
            acc[2] = __builtin_fmaf(a.z, x, acc[2]);
            acc[3] = __builtin_fmaf(a.w, x, acc[3]);
        }
    }
    float *out = g.partial + (int64_t)blockIdx.y * kPartFloats + q.off;
    if (n < q.NC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mm = q.m0 + 4 * mg + i;
            if (mm < q.M) out[mm * q.NC + n] = acc[i];
        }
    }
}

// Launch 3: element e of the partials' layout, partials 0, 1, ... in that order, into its gradient
__global__ __launch_bounds__(kBlock) void k_net_reduce(Bwd g) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= kGradFloats) return;
    float s = g.partial[e];
    for (int p = 1; p < g.parts; ++p) s += g.partial[(int64_t)p * kPartFloats + e];
    const int net = e >= kActorFloats ? 1 : 0;
    int y = e - net * kActorFloats;
    if (y < kOff2) {
        const int mm = y / kC1, n = y - mm * kC1;
        if (n < kIn) g.gw1[net][mm * kIn + n] = s;
        else g.gb1[net][mm] = s;
    } else if (y < kOff3) {
        y -= kOff2;
        const int mm = y / kC2, n = y - mm * kC2;
        if (n < kH) g.gw2[net][mm * kH + n] = s;
        else g.gb2[net][mm] = s;
    } else {
        y -= kOff3;
        const int mm = y / kC2, n = y - mm * kC2;
        if (n < kH) g.gw3[net][mm * kH + n] = s;
        else g.gb3[net][mm] = s;
    }
}

// the same launch for spl_ppo_net_tiled.hip, whose partials have this layout
void launch_net_reduce(const Bwd &g, hipStream_t s) {
    hipLaunchKernelGGL(k_net_reduce, dim3((kGradFloats + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g);
}

}  // namespace spln

using namespace spln;

extern "C" {

int64_t spl_ppo_net_act_bytes(int32_t B) {
    if (const int e = rows_ok(B)) return e;
    return dz_floats(B) * (int64_t)sizeof(float);
}

int64_t spl_ppo_net_scratch_bytes(int32_t B) {
    if (const int e = rows_ok(B)) return e;
    return (dz_floats(B) + (int64_t)parts_of(B) * kPartFloats) * (int64_t)sizeof(float);
}

int spl_ppo_net_forward(int32_t B, const spl_ppo_net_fwd_t *a, void *stream) {
    Fwd f;
    if (const int e = fwd_args(B, a, f)) return e;
    hipLaunchKernelGGL(k_net_forward, dim3((unsigned)((B + kRows - 1) / kRows), 2), dim3(kBlock), 0, (hipStream_t)stream, f);
    return spl_launched("k_net_forward");
}

int spl_ppo_net_backward(int32_t B, const spl_ppo_net_bwd_t *a, void *stream) {
    Bwd g;
    if (const int e = bwd_args(B, a, g)) return e;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_net_dz, dim3((unsigned)((B + kRows - 1) / kRows), 2), dim3(kBlock), 0, s, g);
    hipLaunchKernelGGL(k_net_dw, dim3(kTiles, g.parts), dim3(kBlock), 0, s, g);
    launch_net_reduce(g, s);
    return spl_launched("k_net_backward");
}

}  // extern "C"
