// spl_ppo.hip — the PPO rollout store (include/splendor_ppo.h): record one step's rows, the GAE
// reverse scan of ppo_splendor.py:304-314 with the advantage statistics of :325, and the minibatch
// gather that expands the compact rows into ActorCritic.get_action_and_value's inputs, and the loss head
// of the update (loss, statistics and the gradients with respect to the logits and the value), and the
// optimiser step behind the backward pass (global-norm clip, Adam, target-KL gate).
//
// The GAE scan must be bit-equal to numpy, which never fuses a multiply with an add, while HIP device
// code contracts a*b+c into an FMA by default.  Contraction is switched off for this whole file by
// the pragma below (not by a Makefile flag: the requirement then travels with the source, whatever
// builds it).
#pragma clang fp contract(off)

#include "../../include/splendor_ppo.h"
#include "spl_common.h"
#include "spl_rng.h"

#include <float.h>

namespace splp {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------
// record
// ---------------------------------------------------------------------------------------------
struct Rec {
    const uint32_t *obs;
    uint32_t *dst_obs;
    int64_t quads, tail;  // the rows as `quads` 16-byte pieces, then `tail` dwords
    const int8_t *mask;
    uint64_t *dst_mask;
    const float *reward;
    float *dst_reward;
    const uint8_t *done;
    uint8_t *dst_done;
};

// One launch for all four groups.  Rows: thread q moves 16-byte piece q (both sides 16-byte aligned;
// else quads = 0 and every dword is a `tail` dword).  Masks: a wave owns 64 tables = 2 880 mask bytes,
// read as 45 coalesced 64-byte loads; the ballot of "byte != 0" of load a is bits 64a..64a+63 of the
// wave's 2 880-bit string, of which table L's word is bits 45L..45L+44.  The 45 ballots go through LDS
// (lane a keeps ballot a) so that each lane can pick the two words its bits straddle.
__global__ __launch_bounds__(kBlock) void k_record(int n, Rec r) {
    __shared__ uint64_t words[kBlock / 64][64];
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r.obs) {
        if (q < r.quads) {
            reinterpret_cast<uint4 *>(r.dst_obs)[q] = reinterpret_cast<const uint4 *>(r.obs)[q];
        } else if (q < r.quads + r.tail) {
            const int64_t e = 4 * r.quads + (q - r.quads);
            r.dst_obs[e] = r.obs[e];
        }
    }
    if ((int64_t)blockIdx.x * kBlock >= n) return;  // uniform over the workgroup
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (r.mask) {
        const int64_t base = ((int64_t)blockIdx.x * kBlock + wave * 64) * 45, end = (int64_t)n * 45;
        uint64_t mine = 0;
#pragma unroll 5
        for (int a = 0; a < 45; ++a) {
            const int64_t off = base + a * 64 + lane;
            const int8_t m = off < end ? r.mask[off] : (int8_t)0;
            const uint64_t b = __ballot(m != 0);
            if (lane == a) mine = b;
        }
        words[wave][lane] = lane < 45 ? mine : 0;
        __syncthreads();
        if (q < n) {
            const int bit = 45 * lane, w = bit >> 6, s = bit & 63;  // w + 1 <= 45
            const uint64_t lo = words[wave][w] >> s, hi = s ? words[wave][w + 1] << (64 - s) : 0;
            r.dst_mask[q] = (lo | hi) & ((1ull << 45) - 1);
        }
    }
    if (q < n) {
        if (r.reward) r.dst_reward[q] = r.reward[q];
        if (r.done) r.dst_done[q] = r.done[q];
    }
}

// ---------------------------------------------------------------------------------------------
// GAE
// ---------------------------------------------------------------------------------------------
// One lane per table, K dependent steps per lane.  At 65 536 tables there are four waves per CU, one
// per SIMD, so nothing but the lane's own earlier loads can hide a load's latency: an HBM miss is
// ~900 cycles (MI355X, idle chip), one step's dependent chain (a float multiply, five float64
// operations, two conversions) is of the order of 60-100 cycles, so about a dozen steps have to be in
// flight.  The scan therefore runs in chunks of kAhead = 8 steps with two register buffers: the loads of
// the chunk after next are issued before the current chunk's chain starts, which keeps 8 to 16 steps
// (24 to 48 loads, 48 VGPRs) ahead of the chain.
constexpr int kAhead = 8;

struct Chunk {
    float r[kAhead], v[kAhead];
    uint32_t d[kAhead];
};

struct Gae {
    const float *reward, *value;
    const uint8_t *done;
    const float *last_value;
    float *adv, *ret;
    double gl;      // gamma * lambda, multiplied once on the host in double
    float gamma_f;  // fp32(gamma)
};

// steps t0, t0 - 1, ... : `live` of them (kAhead in the pipelined loop; K % kAhead in the first, partial chunk)
template <bool kFull>
__device__ __forceinline__ void load_chunk(Chunk &c, const Gae &g, int t0, int live, int64_t T, int64_t i) {
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
        if (kFull || j < live) {
            const int64_t e = (int64_t)(t0 - j) * T + i;
            c.r[j] = g.reward[e];
            c.v[j] = g.value[e];
            c.d[j] = g.done[e];
        }
    }
}

struct Scan {
    double last, sum, sumsq;
    float v_next;
};

template <bool kFull>
__device__ __forceinline__ void scan_chunk(const Chunk &c, const Gae &g, int t0, int live, int64_t T, int64_t i, Scan &s) {
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
        const int t = t0 - j;
        if (kFull || j < live) {
            const double nnt = c.d[j] ? 0.0 : 1.0;
            const float gv = g.gamma_f * s.v_next;
            const double v = (double)c.v[j];
            const double delta = ((double)c.r[j] + (double)gv * nnt) - v;
            s.last = delta + (g.gl * nnt) * s.last;
            const float a = (float)s.last;
            const int64_t e = (int64_t)t * T + i;
            g.adv[e] = a;
            g.ret[e] = (float)(s.last + v);
            s.sum += (double)a;
            s.sumsq += (double)a * (double)a;
            s.v_next = c.v[j];
        }
    }
}

// sum of x over the workgroup in a fixed order (a binary tree over the lane index); result in lane 0
__device__ __forceinline__ double block_sum(double x, double *lds) {
    lds[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void k_gae(int K, int T, Gae g, double *__restrict__ partial) {
    __shared__ double lds[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Scan s{0.0, 0.0, 0.0, 0.f};
    if (i < T) {
        s.v_next = g.last_value[i];
        // the K % kAhead newest steps as one partial chunk, then whole chunks only: chunk c (1-based)
        // holds steps kAhead * c - 1 down to kAhead * (c - 1)
        Chunk a, b;
        const int rem = K % kAhead;
        int c = K / kAhead;
        if (rem) load_chunk<false>(b, g, K - 1, rem, T, i);
        if (c >= 1) load_chunk<true>(a, g, kAhead * c - 1, kAhead, T, i);
        if (rem) scan_chunk<false>(b, g, K - 1, rem, T, i, s);
        for (; c >= 2; c -= 2) {
            load_chunk<true>(b, g, kAhead * (c - 1) - 1, kAhead, T, i);
            scan_chunk<true>(a, g, kAhead * c - 1, kAhead, T, i, s);
            if (c >= 3) load_chunk<true>(a, g, kAhead * (c - 2) - 1, kAhead, T, i);
            scan_chunk<true>(b, g, kAhead * (c - 1) - 1, kAhead, T, i, s);
        }
        if (c == 1) scan_chunk<true>(a, g, kAhead - 1, kAhead, T, i, s);
    }
    const double sum = block_sum(s.sum, lds), sumsq = block_sum(s.sumsq, lds);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sum;
        partial[2 * blockIdx.x + 1] = sumsq;
    }
}

// one workgroup: lane j adds partials j, j + 256, ... in that order, then the same tree
__global__ __launch_bounds__(kBlock) void k_gae_finish(int blocks, uint64_t count, const double *__restrict__ partial,
                                                       spl_ppo_stats_t *__restrict__ st) {
    __shared__ double lds[kBlock];
    double s = 0.0, ss = 0.0;
    for (int p = threadIdx.x; p < blocks; p += kBlock) {
        s += partial[2 * p];
        ss += partial[2 * p + 1];
    }
    const double sum = block_sum(s, lds), sumsq = block_sum(ss, lds);
    if (threadIdx.x == 0) {
        const double n = (double)count;
        const double mean = sum / n;
        double var = (sumsq - sum * mean) / (n - 1.0);
        if (var < 0.0) var = 0.0;  // a NaN (count = 1) stays a NaN
        const double sd = sqrt(var);
        st->count = count;
        st->sum = sum;
        st->sumsq = sumsq;
        st->mean = mean;
        st->std = sd;
        st->mean32 = (float)mean;
        st->std32 = (float)sd;
    }
}

// ---------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup.  In: the row's 75 dwords as two coalesced dword loads
// (lanes 0..63, then lanes 0..10) into LDS.  Out: lane j converts bytes j, j + 64, ... so that every
// store instruction of the wave writes 64 consecutive floats (297 floats in five stores, the 45 mask
// floats in one); rows of 297 floats are only 4-byte aligned, so dwords are the widest store.
__global__ __launch_bounds__(kBlock) void k_gather(int B, int64_t total, spl_ppo_gather_t g) {
    __shared__ uint32_t rows[kBlock / 64][76];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    const int64_t pos = b < B ? g.idx[b] : -1;
    const bool ok = b < B && pos >= 0 && pos < total;  // the address is formed only under `ok`
    if (ok) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(g.obs_u8 + pos * SPL_PPO_OBS_U8);
        rows[wave][lane] = src[lane];
        if (lane < 75 - 64) rows[wave][64 + lane] = src[64 + lane];
    }
    __syncthreads();
    if (!ok) {
        if (b < B && lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(g.errors), 1ull);
        return;
    }
    const uint8_t *rb = reinterpret_cast<const uint8_t *>(rows[wave]);
    const uint32_t hi = rb[297];
    float *o = g.out_obs + b * 297;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        const int c = lane + 64 * m;
        if (c < 297) {
            uint32_t x = rb[c];
            if (c == 295) x += hi << 8;  // move_count
            o[c] = (float)x;
        }
    }
    const uint64_t bits = g.mask_bits[pos];
    if (lane < 45) g.out_mask[b * 45 + lane] = ((bits >> lane) & 1) ? 1.f : 0.f;
    if (lane == 0) g.out_action[b] = (int64_t)g.action[pos];
    if (lane == 1) g.out_logprob[b] = g.logprob[pos];
    if (lane == 2) g.out_value[b] = g.value[pos];
    if (lane == 3) g.out_ret[b] = g.ret[pos];
    if (lane == 4) {
        float a = g.adv[pos];
        if (g.normalize) {
            // float32 subtract and add are single IEEE operations; the quotient is taken in float64
            // and rounded once more, which for float32 operands equals the correctly rounded float32
            // quotient (53 >= 2 * 24 + 2)
            const float num = a - g.stats->mean32, den = g.stats->std32 + 1e-8f;
            a = (float)((double)num / (double)den);
        }
        g.out_adv[b] = a;
    }
}

// ---------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------
// A wave owns 64 rows = 2 880 contiguous logits: in as 45 coalesced 64-lane loads into its LDS tile,
// then lane l works on row l out of the tile (a stride of 45 dwords is odd, so the 64 lanes fall on
// different banks), puts the row's gradient back in place, and the tile goes out as 45 coalesced
// stores.  The row's recorded scalars are gathered by idx, one lane per row.  The waves of a workgroup
// share nothing but the partial sums at the end.
constexpr int kLossSums = 6;  // policy, value, entropy, lp_old - lp, clipped rows, bad rows
constexpr uint64_t kAllActions = (1ull << spl::kActions) - 1;

// sum of x over the wave in a fixed order (a butterfly over the lane index); every lane gets it
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) x += __shfl_xor(x, h, 64);
    return x;
}

// the workgroup's sums of q[0], ... in a fixed order (the butterfly inside each wave, then the waves in
// order), in every thread
__device__ __forceinline__ void block_sums(double (&q)[kLossSums], double (*lds)[kLossSums]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kLossSums; ++k) {
        q[k] = wave_sum(q[k]);
        if (lane == k) lds[wave][k] = q[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLossSums; ++k) {
        q[k] = lds[0][k];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) q[k] += lds[w][k];
    }
}

// kDev: the four coefficients come from device memory (spl_ppo_loss_dev) and are checked here, since the
// host could not: one that spl_ppo_loss refuses makes every row of the call a bad row.  Otherwise they are
// the argument block's, which the host has checked.
struct LossCoef {
    float clip, vclip, vf, ent;
    bool valid;
};

template <bool kDev>
__device__ __forceinline__ LossCoef loss_coef(const spl_ppo_loss_t &g, const float *__restrict__ coef) {
    if (!kDev) return LossCoef{g.clip_coef, g.vclip, g.vf_coef, g.ent_coef, true};
    const float4 c = *reinterpret_cast<const float4 *>(coef);
    return LossCoef{c.x, c.y, c.z, c.w, c.x >= 0.f && c.y >= 0.f && c.z >= 0.f && c.w == c.w};
}

template <bool kDev>
__global__ __launch_bounds__(kBlock) void k_loss(int B, int64_t total, float inv_b, spl_ppo_loss_t g,
                                                 const float *__restrict__ coef, double *__restrict__ partial) {
    constexpr int kA = spl::kActions;
    const LossCoef cf = loss_coef<kDev>(g, coef);
    __shared__ float tile[kBlock / 64][64 * kA];
    __shared__ double sums[kBlock / 64][kLossSums];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * (kBlock / 64) + wave) * 64, b = row0 + lane;
    const int64_t base = row0 * kA, end = (int64_t)B * kA;
    const bool whole = base + 64 * kA <= end;  // all 64 rows exist: no bound to test per load and store
    float *t = tile[wave];
    const int64_t pos = b < B ? g.idx[b] : -1;
    const bool in = b < B && pos >= 0 && pos < total;  // an address is formed only under `in`
    uint64_t legal = 0;
    int act = -1;
    float lp_old = 0.f, v_old = 0.f, adv = 0.f, ret = 0.f, v = 0.f;
    if (in) {
        legal = g.mask_bits[pos] & kAllActions;
        act = g.action[pos];
        lp_old = g.logprob[pos];
        v_old = g.value[pos];
        adv = g.adv[pos];
        ret = g.ret[pos];
        v = g.new_value[b];
    }
    // the tile: with all 45 loads in flight at once (and the gathers above beside them) the wave waits
    // for memory once
    if (whole) {
        float in_flight[kA];
#pragma unroll
        for (int a = 0; a < kA; ++a) in_flight[a] = g.logits[base + a * 64 + lane];
#pragma unroll
        for (int a = 0; a < kA; ++a) t[a * 64 + lane] = in_flight[a];
    } else {
#pragma unroll 9
        for (int a = 0; a < kA; ++a) {
            const int64_t off = base + a * 64 + lane;
            if (off < end) t[a * 64 + lane] = g.logits[off];
        }
    }
    if (in && g.normalize) {  // as k_gather
        const float num = adv - g.stats->mean32, den = g.stats->std32 + 1e-8f;
        adv = (float)((double)num / (double)den);
    }
    if (!legal) legal = kAllActions;
    const bool ok = in && cf.valid && act >= 0 && act < kA && ((legal >> act) & 1);
    spl::wave_lds_sync();

    float *row = t + lane * kA;
    float dv = 0.f;
    double q[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0, (b < B && !ok) ? 1.0 : 0.0};
    if (ok) {
        // x[j]: the logit, then logit - max, then log p_j; -inf for an illegal j until log p_j is clamped
        // to -FLT_MAX, and its p_j = exp(-inf) is an exact 0: every product with it below is a zero, so
        // the loops need no branch on legality
        float x[kA];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kA; ++j) {
            x[j] = ((legal >> j) & 1) ? row[j] : -INFINITY;
            m = fmaxf(m, x[j]);
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kA; ++j) {
            x[j] -= m;
            s += expf(x[j]);
        }
        const float logz = logf(s);
        float H = 0.f, lp = 0.f;
#pragma unroll
        for (int j = 0; j < kA; ++j) {
            const float p = expf(x[j] - logz);
            const float l = fmaxf(x[j] - logz, -FLT_MAX);  // keeps 0 * log 0 at 0, as torch's entropy() does
            x[j] = l;
            row[j] = p;
            H -= p * l;
            lp = j == act ? l : lp;
        }
        const float c = cf.clip, lo = 1.f - c, hi = 1.f + c;
        const float r = expf(lp - lp_old), rc = fminf(fmaxf(r, lo), hi);
        const float s1 = r * adv, s2 = rc * adv;
        const float g_lp = ((r >= lo && r <= hi) || s1 < s2) ? -(adv * r) * inv_b : 0.f;
        const float g_ent = cf.ent * inv_b;
#pragma unroll
        for (int j = 0; j < kA; ++j) {
            const float p = row[j];
            row[j] = (g_lp * ((j == act ? 1.f : 0.f) - p) - g_ent * p * (x[j] + H)) + 0.f;  // -0 + 0 = +0
        }
        const float vclip = cf.vclip, dlt = v - v_old;
        const float v_c = v_old + fminf(fmaxf(dlt, -vclip), vclip);
        const float e1 = v - ret, e2 = v_c - ret, q1 = e1 * e1, q2 = e2 * e2;
        const float w1 = q1 > q2 ? 1.f : q1 < q2 ? 0.f : 0.5f;
        const float through = (dlt >= -vclip && dlt <= vclip) ? (1.f - w1) * e2 : 0.f;
        dv = cf.vf * inv_b * (w1 * e1 + through);
        q[0] = -(double)fminf(s1, s2);
        q[1] = (double)(0.5f * fmaxf(q1, q2));
        q[2] = (double)H;
        q[3] = (double)(lp_old - lp);
        q[4] = fabsf(r - 1.f) > c ? 1.0 : 0.0;
    } else {
#pragma unroll
        for (int j = 0; j < kA; ++j) row[j] = 0.f;  // a bad row; past B the tile row is never stored
    }
    if (b < B) g.dvalue[b] = dv;
    spl::wave_lds_sync();
    if (whole) {
#pragma unroll
        for (int a = 0; a < kA; ++a) g.dlogits[base + a * 64 + lane] = t[a * 64 + lane];
    } else {
#pragma unroll 9
        for (int a = 0; a < kA; ++a) {
            const int64_t off = base + a * 64 + lane;
            if (off < end) g.dlogits[off] = t[a * 64 + lane];
        }
    }

    block_sums(q, sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kLossSums; ++k) partial[(int64_t)blockIdx.x * kLossSums + k] = q[k];
        if (q[kLossSums - 1] > 0.0)
            atomicAdd(reinterpret_cast<unsigned long long *>(g.errors), (unsigned long long)q[kLossSums - 1]);
    }
}

// one workgroup: lane j adds partials j, j + 256, ... in that order, then block_sums
// (coef: the device block of spl_ppo_loss_dev, whose vf_coef and ent_coef then replace the arguments)
__global__ __launch_bounds__(kBlock) void k_loss_finish(int blocks, int B, float vf_coef, float ent_coef,
                                                        const float *__restrict__ coef,
                                                        const double *__restrict__ partial,
                                                        spl_ppo_loss_out_t *__restrict__ o) {
    __shared__ double sums[kBlock / 64][kLossSums];
    if (coef) vf_coef = coef[2], ent_coef = coef[3];
    double q[kLossSums] = {};
    for (int p = threadIdx.x; p < blocks; p += kBlock) {
#pragma unroll
        for (int k = 0; k < kLossSums; ++k) q[k] += partial[(int64_t)p * kLossSums + k];
    }
    block_sums(q, sums);
    if (threadIdx.x == 0) {
        const double n = (double)B;
        o->policy_loss = q[0] / n;
        o->value_loss = q[1] / n;
        o->entropy = q[2] / n;
        o->approx_kl = q[3] / n;
        o->clipfrac = q[4] / n;
        const double loss = (o->policy_loss + (double)vf_coef * o->value_loss) + (double)ent_coef * o->entropy;
        o->loss = loss;
        o->loss32 = (float)loss;
        o->bad = (uint32_t)q[5];
    }
}

// ---------------------------------------------------------------------------------------------
// adam
// ---------------------------------------------------------------------------------------------
// The segments are cut into chunks of kChunk floats (a segment starts a new chunk), a workgroup takes
// chunks blockIdx.x, blockIdx.x + kParts, ... and thread t of it the 16-byte pieces t and t + 256 of each:
// wave instructions of 1 KiB when the segment is 16-byte aligned throughout, the same elements a dword at
// a time when it is not.  Both launches walk the chunks alike.  The agent's 295 982 floats are 150 chunks:
// 8 MB through L2 in two launches, so the call is bound by its launches, not by the memory behind them.
constexpr int kChunk = SPL_PPO_ADAM_CHUNK, kParts = SPL_PPO_ADAM_PARTS, kSegs = SPL_PPO_ADAM_MAX_TENSORS;
constexpr int kPieces = kChunk / 4 / kBlock;  // 16-byte pieces of a chunk per thread
static_assert(kPieces * 4 * kBlock == kChunk, "a chunk is a whole number of 16-byte pieces per thread");

struct Adam {
    float *p[kSegs];
    const float *g[kSegs];
    int64_t numel[kSegs];
    int64_t at[kSegs];          // the segment's first float in the arenas
    int32_t chunk0[kSegs + 1];  // the segment's first chunk; chunk0[n] = all chunks
    int32_t n;
    uint32_t wide;              // bit i: segment i moves 16 bytes a lane
    float *m, *v;
    spl_ppo_adam_state_t *st;
    const double *kl;
    const spl_ppo_loss_out_t *lo;
    double *partial;
};

// floats e .. e + 3 of a segment of `numel` floats (e < numel; past the end: 0)
__device__ __forceinline__ void load4(const float *src, int64_t e, int64_t numel, bool wide, float (&x)[4]) {
    if (wide && e + 4 <= numel) {
        const float4 q = *reinterpret_cast<const float4 *>(src + e);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = e + j < numel ? src[e + j] : 0.f;
    }
}

__device__ __forceinline__ void store4(float *dst, int64_t e, int64_t numel, bool wide, const float (&x)[4]) {
    if (wide && e + 4 <= numel) {
        *reinterpret_cast<float4 *>(dst + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < numel) dst[e + j] = x[j];
    }
}

// the segment of chunk c (uniform over the workgroup)
__device__ __forceinline__ int segment_of(const Adam &a, int c) {
    int s = 0;
    while (s + 1 < a.n && c >= a.chunk0[s + 1]) ++s;
    return s;
}

// Launch 1.  partial[b] = the squares of chunks b, b + kParts, ...: per thread in element order, then
// block_sum's tree.  Thread 0 of workgroup 0 is the only reader of the latch and the only writer of the
// words launch 2's workgroups all read.
__global__ __launch_bounds__(kBlock) void k_adam_norm(Adam a) {
    __shared__ double lds[kBlock];
    const int chunks = a.chunk0[a.n];
    double acc = 0.0;
    for (int c = blockIdx.x; c < chunks; c += kParts) {
        const int s = segment_of(a, c);
        const int64_t numel = a.numel[s], base = (int64_t)(c - a.chunk0[s]) * kChunk;
        const float *g = a.g[s];
        const bool wide = (a.wide >> s) & 1;
#pragma unroll
        for (int k = 0; k < kPieces; ++k) {
            const int64_t e = base + 4 * (int64_t)(threadIdx.x + k * kBlock);
            if (e < numel) {
                float x[4];
                load4(g, e, numel, wide, x);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sq = x[j] * x[j];
                    acc += (double)sq;
                }
            }
        }
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        a.partial[blockIdx.x] = sum;
        if (blockIdx.x == 0) {
            spl_ppo_adam_state_t *st = a.st;
            st->armed = st->stopped ? 0 : 1;
            st->step_in = st->step;
            const double target = st->target_kl;
            if (target > 0.0 && (a.kl || a.lo)) {
                const double kl = a.kl ? *a.kl : a.lo->approx_kl;
                if (kl > target) st->stopped = 1;
            }
        }
    }
}

struct AdamScalars {
    float coef, w1, b2, w2, step_size, bc2_sqrt, eps;
    int active;
};

// Launch 2.  Every workgroup adds the partial sums in one order (lane j takes j, j + 256, ..., then
// block_sum's tree), so all decide alike; workgroup 0 writes the outcome to words this launch never reads.
__global__ __launch_bounds__(kBlock) void k_adam_step(Adam a, int parts) {
    __shared__ double lds[kBlock];
    __shared__ AdamScalars shared;
    double acc = 0.0;
    for (int p = threadIdx.x; p < parts; p += kBlock) acc += a.partial[p];
    const double sumsq = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        spl_ppo_adam_state_t *st = a.st;
        const double norm = sqrt(sumsq);
        const bool finite = norm - norm == 0.0;
        const bool armed = st->armed != 0, active = armed && finite;
        const double mx = st->max_norm, cn = mx / (norm + 1e-6);
        const float coef = mx < 0.0 ? 1.f : (float)(cn < 1.0 ? cn : 1.0);
        const double step = (double)(st->step_in + 1), b1 = st->beta1, b2 = st->beta2;
        const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
        shared = AdamScalars{coef, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)(st->lr / bc1),
                             (float)sqrt(bc2), (float)st->eps, active ? 1 : 0};
        if (blockIdx.x == 0) {
            st->active = active ? 1 : 0;
            st->grad_norm = norm;
            st->clip_coef = (double)coef;
            if (!armed) {
                st->gated += 1;
            } else if (!finite) {
                st->nonfinite += 1;
            } else {
                st->step = st->step_in + 1;
                if (a.lo) {
                    st->last = *a.lo;
                    if (st->applied == 0) st->first = *a.lo;
                }
                st->applied += 1;
            }
        }
    }
    __syncthreads();
    const AdamScalars sc = shared;
    if (!sc.active) return;
    const int chunks = a.chunk0[a.n];
    for (int c = blockIdx.x; c < chunks; c += kParts) {
        const int s = segment_of(a, c);
        const int64_t numel = a.numel[s], base = (int64_t)(c - a.chunk0[s]) * kChunk;
        float *p = a.p[s], *m = a.m + a.at[s], *v = a.v + a.at[s];
        const float *g = a.g[s];
        const bool wide = (a.wide >> s) & 1;
#pragma unroll
        for (int k = 0; k < kPieces; ++k) {
            const int64_t e = base + 4 * (int64_t)(threadIdx.x + k * kBlock);
            if (e < numel) {
                float xp[4], xg[4], xm[4], xv[4];
                load4(p, e, numel, wide, xp);
                load4(g, e, numel, wide, xg);
                load4(m, e, numel, wide, xm);
                load4(v, e, numel, wide, xv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gc = xg[j] * sc.coef;
                    xm[j] = xm[j] + (gc - xm[j]) * sc.w1;
                    xv[j] = xv[j] * sc.b2 + sc.w2 * (gc * gc);
                    xp[j] = xp[j] - sc.step_size * (xm[j] / (sqrtf(xv[j]) / sc.bc2_sqrt + sc.eps));
                }
                store4(p, e, numel, wide, xp);
                store4(m, e, numel, wide, xm);
                store4(v, e, numel, wide, xv);
            }
        }
    }
}

__global__ void k_adam_begin(spl_ppo_adam_state_t *st, int update) {
    st->stopped = 0;
    if (update) {
        st->applied = st->gated = st->nonfinite = 0;
        st->first = spl_ppo_loss_out_t{};
    }
}

// ---------------------------------------------------------------------------------------------
// permute
// ---------------------------------------------------------------------------------------------
// One thread per output word, pads included, so the -1 words need no launch of their own.  Element i is
// computed from (seed, draw, i) alone: a pass is eight rounds of an alternating Feistel network over the
// `wa + wb` bits that hold n - 1, Philox4x32-10 as the round function, and passes are repeated until the
// value falls below n (cycle walking; a pass is a bijection of [0, 2^bits), so the walk from i < n ends).
// Nothing here writes *state: k_permute_advance does, one thread, behind this launch.
struct Perm {
    uint32_t n, B, stride;
    int wa, wb;     // a = bits / 2, b = bits - a
    int64_t slots;  // ceil(n / B) * stride
    const spl_ppo_perm_state_t *state;
    int64_t *out;
};

__device__ __forceinline__ uint32_t permute_pass(uint32_t x, int wa, int wb, uint2 key, uint32_t d_lo, uint32_t d_hi) {
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const int wl = (r & 1) ? wa : wb, wr = (r & 1) ? wb : wa;
        const uint32_t L = x >> wr, R = x & ((1u << wr) - 1u);
        const uint32_t f = spl::philox4x32(make_uint4(R, r, d_lo, d_hi), key).x;
        x = (R << wl) | ((L ^ f) & ((1u << wl) - 1u));
    }
    return x;
}

__global__ __launch_bounds__(kBlock) void k_permute(Perm p) {
    const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= p.slots) return;
    const uint64_t seed = p.state->seed, draw = p.state->draw;
    const uint32_t row = (uint32_t)(slot / p.stride), col = (uint32_t)(slot - (int64_t)row * p.stride);
    const uint64_t i = (uint64_t)row * p.B + col;  // below 2^32 + 2^31
    int64_t v = -1;
    if (col < p.B && i < p.n) {
        uint32_t x = (uint32_t)i;
        if (p.n > 1) {
            const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
            do x = permute_pass(x, p.wa, p.wb, key, (uint32_t)draw, (uint32_t)(draw >> 32));
            while (x >= p.n);
        }
        v = (int64_t)x;
    }
    p.out[slot] = v;
}

__global__ void k_permute_advance(spl_ppo_perm_state_t *st) { st->draw += 1; }

}  // namespace splp

using namespace splp;

extern "C" {

int spl_ppo_record(int32_t n, const spl_ppo_record_t *a, void *stream) {
    if (n <= 0) return spl_fail(SPL_E_ARG, "n must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null record arguments");
    if (!a->obs_u8 != !a->dst_obs_u8 || !a->mask != !a->dst_mask_bits || !a->reward != !a->dst_reward ||
        !a->done != !a->dst_done)
        return spl_fail(SPL_E_ARG, "null buffer: a record group needs its source and its destination");
    if (!a->obs_u8 && !a->mask && !a->reward && !a->done) return spl_fail(SPL_E_ARG, "null buffer: nothing to record");
    if (spl_misaligned(a->obs_u8, 4) || spl_misaligned(a->dst_obs_u8, 4))
        return spl_fail(SPL_E_ARG, "obs_u8 rows must be 4-byte aligned");
    if (spl_misaligned(a->dst_mask_bits, 8)) return spl_fail(SPL_E_ARG, "mask_bits must be 8-byte aligned");
    if (spl_misaligned(a->reward, 4) || spl_misaligned(a->dst_reward, 4))
        return spl_fail(SPL_E_ARG, "reward rows must be 4-byte aligned");
    Rec r{};
    const int64_t dwords = (int64_t)n * (SPL_PPO_OBS_U8 / 4);
    if (a->obs_u8) {
        r.obs = reinterpret_cast<const uint32_t *>(a->obs_u8);
        r.dst_obs = reinterpret_cast<uint32_t *>(a->dst_obs_u8);
        const bool wide = !spl_misaligned(a->obs_u8, 16) && !spl_misaligned(a->dst_obs_u8, 16);
        r.quads = wide ? dwords / 4 : 0;
        r.tail = dwords - 4 * r.quads;
    }
    r.mask = a->mask;
    r.dst_mask = a->dst_mask_bits;
    r.reward = a->reward;
    r.dst_reward = a->dst_reward;
    r.done = a->done;
    r.dst_done = a->dst_done;
    const int64_t items = r.quads + r.tail, threads = items > n ? items : (int64_t)n;
    hipLaunchKernelGGL(k_record, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       n, r);
    return spl_launched("k_record");
}

int64_t spl_ppo_gae_scratch_bytes(int32_t T) {
    if (T < 1) return spl_fail(SPL_E_ARG, "T must be positive");
    return (int64_t)((T + kBlock - 1) / kBlock) * 2 * (int64_t)sizeof(double);
}

int spl_ppo_gae(int32_t K, int32_t T, const spl_ppo_gae_t *a, void *stream) {
    if (K < 1 || T < 1) return spl_fail(SPL_E_ARG, "K and T must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null gae arguments");
    if (!a->reward || !a->value || !a->done || !a->last_value || !a->adv || !a->ret || !a->stats || !a->scratch)
        return spl_fail(SPL_E_ARG, "null buffer");
    if (!(a->gamma >= 0.0 && a->gamma <= 1.0) || !(a->lambda >= 0.0 && a->lambda <= 1.0))
        return spl_fail(SPL_E_ARG, "gamma and lambda must be in [0, 1]");
    if (spl_misaligned(a->reward, 4) || spl_misaligned(a->value, 4) || spl_misaligned(a->last_value, 4) || spl_misaligned(a->adv, 4) ||
        spl_misaligned(a->ret, 4) || spl_misaligned(a->stats, 8) || spl_misaligned(a->scratch, 8))
        return spl_fail(SPL_E_ARG, "float planes must be 4-byte aligned, stats and scratch 8-byte aligned");
    const Gae g{a->reward, a->value, a->done, a->last_value, a->adv, a->ret, a->gamma * a->lambda, (float)a->gamma};
    const int blocks = (T + kBlock - 1) / kBlock;
    const hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(a->scratch);
    hipLaunchKernelGGL(k_gae, dim3(blocks), dim3(kBlock), 0, s, K, T, g, partial);
    hipLaunchKernelGGL(k_gae_finish, dim3(1), dim3(kBlock), 0, s, blocks, (uint64_t)K * (uint64_t)T, partial, a->stats);
    return spl_launched("k_gae");
}

int spl_ppo_gather(int32_t B, const spl_ppo_gather_t *a, void *stream) {
    if (B <= 0) return spl_fail(SPL_E_ARG, "B must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null gather arguments");
    if (a->K < 1 || a->T < 1) return spl_fail(SPL_E_ARG, "K and T must be positive");
    if (!a->idx || !a->obs_u8 || !a->mask_bits || !a->action || !a->logprob || !a->value || !a->adv || !a->ret ||
        !a->out_obs || !a->out_mask || !a->out_action || !a->out_logprob || !a->out_value || !a->out_adv ||
        !a->out_ret || !a->errors || (a->normalize && !a->stats))
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->obs_u8, 4)) return spl_fail(SPL_E_ARG, "obs_u8 rows must be 4-byte aligned");
    if (spl_misaligned(a->idx, 8) || spl_misaligned(a->mask_bits, 8) || spl_misaligned(a->out_action, 8) ||
        spl_misaligned(a->errors, 8) || spl_misaligned(a->stats, 8))
        return spl_fail(SPL_E_ARG, "idx, mask_bits, out_action, errors and stats must be 8-byte aligned");
    if (spl_misaligned(a->out_obs, 4) || spl_misaligned(a->out_mask, 4))
        return spl_fail(SPL_E_ARG, "float outputs must be 4-byte aligned");
    const int rows = kBlock / 64;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((B + rows - 1) / rows)), dim3(kBlock), 0, (hipStream_t)stream, B,
                       (int64_t)a->K * a->T, *a);
    return spl_launched("k_gather");
}

int64_t spl_ppo_loss_scratch_bytes(int32_t B) {
    if (B < 1) return spl_fail(SPL_E_ARG, "B must be positive");
    return (((int64_t)B + kBlock - 1) / kBlock) * kLossSums * (int64_t)sizeof(double);
}

// what spl_ppo_loss and spl_ppo_loss_dev check alike; coef: NULL for the argument block's coefficients
static int loss_call(int32_t B, const spl_ppo_loss_t *a, const float *coef, bool dev, void *stream) {
    if (B < 1) return spl_fail(SPL_E_ARG, "B must be positive");
    if (!a) return spl_fail(SPL_E_ARG, "null loss arguments");
    if (a->K < 1 || a->T < 1) return spl_fail(SPL_E_ARG, "K and T must be positive");
    if (!a->idx || !a->mask_bits || !a->action || !a->logprob || !a->value || !a->adv || !a->ret || !a->logits ||
        !a->new_value || !a->dlogits || !a->dvalue || !a->out || !a->errors || !a->scratch || (a->normalize && !a->stats))
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->idx, 8) || spl_misaligned(a->mask_bits, 8) || spl_misaligned(a->stats, 8) ||
        spl_misaligned(a->out, 8) || spl_misaligned(a->errors, 8) || spl_misaligned(a->scratch, 8))
        return spl_fail(SPL_E_ARG, "idx, mask_bits, stats, out, errors and scratch must be 8-byte aligned");
    if (spl_misaligned(a->action, 4) || spl_misaligned(a->logprob, 4) || spl_misaligned(a->value, 4) ||
        spl_misaligned(a->adv, 4) || spl_misaligned(a->ret, 4) || spl_misaligned(a->logits, 4) ||
        spl_misaligned(a->new_value, 4) || spl_misaligned(a->dlogits, 4) || spl_misaligned(a->dvalue, 4))
        return spl_fail(SPL_E_ARG, "action and the float planes must be 4-byte aligned");
    if (dev) {
        if (!coef) return spl_fail(SPL_E_ARG, "null buffer");
        if (spl_misaligned(coef, 16)) return spl_fail(SPL_E_ARG, "coef must be 16-byte aligned");
    } else {
        if (a->clip_coef != a->clip_coef || a->vclip != a->vclip || a->vf_coef != a->vf_coef || a->ent_coef != a->ent_coef)
            return spl_fail(SPL_E_ARG, "a coefficient is NaN");
        if (a->clip_coef < 0.f || a->vclip < 0.f || a->vf_coef < 0.f)
            return spl_fail(SPL_E_ARG, "clip_coef, vclip and vf_coef must not be negative");
    }
    const int blocks = (int)(((int64_t)B + kBlock - 1) / kBlock);
    const hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(a->scratch);
    const int64_t total = (int64_t)a->K * a->T;
    if (dev)
        hipLaunchKernelGGL(k_loss<true>, dim3(blocks), dim3(kBlock), 0, s, B, total, 1.f / (float)B, *a, coef, partial);
    else
        hipLaunchKernelGGL(k_loss<false>, dim3(blocks), dim3(kBlock), 0, s, B, total, 1.f / (float)B, *a, coef, partial);
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kBlock), 0, s, blocks, B, a->vf_coef, a->ent_coef, coef, partial, a->out);
    return spl_launched("k_loss");
}

int spl_ppo_loss(int32_t B, const spl_ppo_loss_t *a, void *stream) { return loss_call(B, a, nullptr, false, stream); }

int spl_ppo_loss_dev(int32_t B, const spl_ppo_loss_t *a, const float *coef, void *stream) {
    return loss_call(B, a, coef, true, stream);
}

int spl_ppo_permute(const spl_ppo_permute_t *a, void *stream) {
    if (!a) return spl_fail(SPL_E_ARG, "null permute arguments");
    if (a->reserved != 0) return spl_fail(SPL_E_ARG, "reserved must be 0");
    if (!a->state || !a->out) return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->state, 8)) return spl_fail(SPL_E_ARG, "state must be 8-byte aligned");
    if (spl_misaligned(a->out, 16)) return spl_fail(SPL_E_ARG, "out must be 16-byte aligned");
    if (a->n < 1 || a->n > (int64_t)INT32_MAX) return spl_fail(SPL_E_RANGE, "n must be in 1 .. 2^31 - 1");
    if (a->B < 1 || (int64_t)a->B > a->n) return spl_fail(SPL_E_RANGE, "B must be in 1 .. n");
    Perm p{};
    p.n = (uint32_t)a->n;
    p.B = (uint32_t)a->B;
    p.stride = (p.B + 1u) & ~1u;
    p.slots = ((a->n + a->B - 1) / a->B) * (int64_t)p.stride;  // at most 2^32: B = 1, stride 2
    int bits = 0;
    while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)a->n) ++bits;  // bit_length(n - 1)
    if (bits < 2) bits = 2;
    p.wa = bits / 2;
    p.wb = bits - p.wa;
    p.state = a->state;
    p.out = a->out;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_permute, dim3((unsigned)((p.slots + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(k_permute_advance, dim3(1), dim3(1), 0, s, a->state);
    return spl_launched("k_permute");
}

static int64_t adam_chunks(int64_t numel) { return (numel + kChunk - 1) / kChunk; }

int64_t spl_ppo_adam_scratch_bytes(int64_t total_numel) {
    if (total_numel < 1) return spl_fail(SPL_E_ARG, "total_numel must be positive");
    if (total_numel > (int64_t)1 << 31) return spl_fail(SPL_E_ARG, "total_numel must not exceed 2^31");
    const int64_t chunks = adam_chunks(total_numel) + (kSegs - 1);
    return (chunks < kParts ? chunks : kParts) * (int64_t)sizeof(double);
}

int spl_ppo_adam_begin(spl_ppo_adam_state_t *state, int32_t what, void *stream) {
    if (!state) return spl_fail(SPL_E_ARG, "null state");
    if (spl_misaligned(state, 8)) return spl_fail(SPL_E_ARG, "state must be 8-byte aligned");
    if (what != SPL_PPO_ADAM_EPOCH && what != SPL_PPO_ADAM_UPDATE)
        return spl_fail(SPL_E_ARG, "what must be SPL_PPO_ADAM_EPOCH or SPL_PPO_ADAM_UPDATE");
    hipLaunchKernelGGL(k_adam_begin, dim3(1), dim3(1), 0, (hipStream_t)stream, state, what == SPL_PPO_ADAM_UPDATE ? 1 : 0);
    return spl_launched("k_adam_begin");
}

int spl_ppo_adam(const spl_ppo_adam_t *a, void *stream) {
    if (!a) return spl_fail(SPL_E_ARG, "null adam arguments");
    if (a->n < 1 || a->n > kSegs) return spl_fail(SPL_E_ARG, "n must be in 1..SPL_PPO_ADAM_MAX_TENSORS");
    if (a->reserved != 0) return spl_fail(SPL_E_ARG, "reserved must be 0");
    if (!a->exp_avg || !a->exp_avg_sq || !a->state || !a->scratch) return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->exp_avg, 4) || spl_misaligned(a->exp_avg_sq, 4))
        return spl_fail(SPL_E_ARG, "the moment arenas must be 4-byte aligned");
    if (spl_misaligned(a->state, 8) || spl_misaligned(a->scratch, 8) || spl_misaligned(a->approx_kl, 8) ||
        spl_misaligned(a->loss_out, 8))
        return spl_fail(SPL_E_ARG, "state, scratch, approx_kl and loss_out must be 8-byte aligned");
    Adam k{};
    int64_t total = 0, at = 0, chunks = 0;
    for (int i = 0; i < a->n; ++i) {
        if (!a->param[i] || !a->grad[i]) return spl_fail(SPL_E_ARG, "null buffer: a segment needs its parameter and its gradient");
        if (spl_misaligned(a->param[i], 4) || spl_misaligned(a->grad[i], 4))
            return spl_fail(SPL_E_ARG, "parameters and gradients must be 4-byte aligned");
        if (a->numel[i] < 1) return spl_fail(SPL_E_ARG, "numel must be positive");
        if (a->numel[i] > ((int64_t)1 << 31) - total) return spl_fail(SPL_E_ARG, "the segments together must not exceed 2^31 floats");
        total += a->numel[i];
        k.p[i] = a->param[i];
        k.g[i] = a->grad[i];
        k.numel[i] = a->numel[i];
        k.at[i] = at;
        k.chunk0[i] = (int32_t)chunks;
        if (!spl_misaligned(a->param[i], 16) && !spl_misaligned(a->grad[i], 16) && !spl_misaligned(a->exp_avg + at, 16) &&
            !spl_misaligned(a->exp_avg_sq + at, 16))
            k.wide |= 1u << i;
        at += (a->numel[i] + 3) / 4 * 4;
        chunks += adam_chunks(a->numel[i]);
    }
    k.chunk0[a->n] = (int32_t)chunks;
    k.n = a->n;
    k.m = a->exp_avg;
    k.v = a->exp_avg_sq;
    k.st = a->state;
    k.kl = a->approx_kl;
    k.lo = a->loss_out;
    k.partial = static_cast<double *>(a->scratch);
    const int parts = (int)(chunks < kParts ? chunks : kParts);  // <= spl_ppo_adam_scratch_bytes(total) / 8
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_norm, dim3(parts), dim3(kBlock), 0, s, k);
    hipLaunchKernelGGL(k_adam_step, dim3(parts), dim3(kBlock), 0, s, k, parts);
    return spl_launched("k_adam");
}

}  // extern "C"
