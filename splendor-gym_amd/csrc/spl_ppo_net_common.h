// spl_ppo_net_common.h — what the sources of the PPO network passes share (spl_ppo_net.hip, the
// 8-rows-a-workgroup VALU kernels; spl_ppo_net_tiled.hip, the LDS-tiled f32-MFMA kernels; spl_ppo_net_bf16.hip,
// the same tiles with bf16 operands): the sizes, the layout of the partial sums in `scratch`, tanh_acc, the
// kernels' argument blocks and the host-side checks that fill them.  The two f32 sources give the same bytes,
// so everything that fixes a summation order is here; the bf16 source keeps the split of the sums over rows.
// What only the two tiled sources share, the tile apart from its operand format, is spl_ppo_net_tile.h.
#pragma once
#include "../../include/splendor_ppo.h"
#include "spl_common.h"

namespace spln {

constexpr int kBlock = 256;
constexpr int kH = SPL_PPO_NET_HIDDEN;     // hidden units = threads of a workgroup
constexpr int kIn = spl::kObsDim;          // 297
constexpr int kA = spl::kActions;          // 45
constexpr int kChunkRows = SPL_PPO_NET_BWD_ROWS;
constexpr int kParts = SPL_PPO_NET_BWD_PARTS;
constexpr int kTile = 32;                  // a stage of the sums over rows is 32 rows (zeros past a chunk's end)
static_assert(kH == kBlock, "a thread is a hidden unit");
static_assert(kChunkRows % kTile == 0, "a chunk is a whole number of 32-row stages");

// The partial sums of the backward's second launch, per network: dW1 with db1 as column 297, dW2 with db2 as
// column 256, dW3 with db3 as column 256; the actor's block, then the critic's.
constexpr int kC1 = kIn + 1, kC2 = kH + 1;                         // augmented column counts
constexpr int kOff2 = kH * kC1, kOff3 = kOff2 + kH * kC2;          // inside a network's block
constexpr int kActorFloats = kOff3 + kA * kC2, kCriticFloats = kOff3 + 1 * kC2;
constexpr int kGradFloats = kActorFloats + kCriticFloats;          // 295 982: every parameter once
constexpr int kPartFloats = (kGradFloats + 3) / 4 * 4;             // a partial's stride

struct Mlp {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
};

// tanh to a few ulp (0.73 ulp measured over tests/crafted_nets.py's arguments, 4 allowed; spl_policy32.hip's tanh_acc, kept as a copy so that the actors' code does not move): an odd
// polynomial below 0.625, 1 - 2 / (exp(2|x|) + 1) above
__device__ __forceinline__ float tanh_acc(float x) {
    const float ax = __builtin_fabsf(x);
    const float z = ax * ax;
    float p = -0.005718891508877277f;
    p = __builtin_fmaf(p, z, 0.02065306343138218f);
    p = __builtin_fmaf(p, z, -0.053744640201330185f);
    p = __builtin_fmaf(p, z, 0.13331513106822968f);
    p = __builtin_fmaf(p, z, -0.3333328664302826f);
    const float small = __builtin_fmaf(ax * z, p, ax);
    const float e = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);  // exp(2|x|)
    const float big = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
    return __builtin_copysignf(ax < 0.625f ? small : big, x);
}

// the forward kernels' arguments
struct Fwd {
    int B;
    int64_t total;
    const int64_t *idx;
    const uint8_t *obs;
    Mlp net[2];
    float *logits, *value, *act;
    unsigned long long *errors;
};

// the backward kernels' arguments
struct Bwd {
    int B, parts, chunks;
    int64_t total;
    const int64_t *idx;
    const uint8_t *obs;
    const float *w2[2], *w3[2];
    const float *dout[2];  // dlogits, dvalue
    const float *act;
    float *dz;             // scratch: [net][dZ2, dZ1][B][256]
    float *partial;        // scratch: [parts][kPartFloats]
    float *gw1[2], *gb1[2], *gw2[2], *gb2[2], *gw3[2], *gb3[2];
};

inline int chunks_of(int B) { return (B + kChunkRows - 1) / kChunkRows; }
inline int parts_of(int B) { return chunks_of(B) < kParts ? chunks_of(B) : kParts; }
inline int64_t dz_floats(int B) { return (int64_t)4 * B * kH; }

inline int rows_ok(int32_t B) {
    if (B < 1) return spl_fail(SPL_E_ARG, "B must be positive");
    if (B > SPL_PPO_NET_MAX_ROWS) return spl_fail(SPL_E_RANGE, "B must not exceed SPL_PPO_NET_MAX_ROWS (65536)");
    return SPL_OK;
}

inline bool mlp_null(const spl_ppo_mlp_t &m) { return !m.w1 || !m.b1 || !m.w2 || !m.b2 || !m.w3 || !m.b3; }
inline bool mlp_misaligned(const spl_ppo_mlp_t &m) {
    return spl_misaligned(m.w1, 16) || spl_misaligned(m.b1, 16) || spl_misaligned(m.w2, 16) || spl_misaligned(m.b2, 16) ||
           spl_misaligned(m.w3, 16) || spl_misaligned(m.b3, 16);
}
inline bool grad_null(const spl_ppo_mlp_grad_t &m) { return !m.w1 || !m.b1 || !m.w2 || !m.b2 || !m.w3 || !m.b3; }
inline bool grad_misaligned(const spl_ppo_mlp_grad_t &m) {
    return spl_misaligned(m.w1, 16) || spl_misaligned(m.b1, 16) || spl_misaligned(m.w2, 16) || spl_misaligned(m.b2, 16) ||
           spl_misaligned(m.w3, 16) || spl_misaligned(m.b3, 16);
}

// the checks of a forward call and its kernels' arguments: SPL_OK, or the error already reported
inline int fwd_args(int32_t B, const spl_ppo_net_fwd_t *a, Fwd &f) {
    if (const int e = rows_ok(B)) return e;
    if (!a) return spl_fail(SPL_E_ARG, "null forward arguments");
    if (a->K < 1 || a->T < 1) return spl_fail(SPL_E_ARG, "K and T must be positive");
    if (a->reserved != 0) return spl_fail(SPL_E_ARG, "reserved must be 0");
    if (!a->idx || !a->obs_u8 || mlp_null(a->actor) || mlp_null(a->critic) || !a->logits || !a->new_value || !a->act ||
        !a->errors)
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->idx, 16) || spl_misaligned(a->obs_u8, 16) || mlp_misaligned(a->actor) || mlp_misaligned(a->critic) ||
        spl_misaligned(a->logits, 16) || spl_misaligned(a->new_value, 16) || spl_misaligned(a->act, 16) ||
        spl_misaligned(a->errors, 16))
        return spl_fail(SPL_E_ARG, "every pointer must be 16-byte aligned");
    f = Fwd{};
    f.B = B;
    f.total = (int64_t)a->K * a->T;
    f.idx = a->idx;
    f.obs = a->obs_u8;
    f.net[0] = Mlp{a->actor.w1, a->actor.b1, a->actor.w2, a->actor.b2, a->actor.w3, a->actor.b3};
    f.net[1] = Mlp{a->critic.w1, a->critic.b1, a->critic.w2, a->critic.b2, a->critic.w3, a->critic.b3};
    f.logits = a->logits;
    f.value = a->new_value;
    f.act = static_cast<float *>(a->act);
    f.errors = reinterpret_cast<unsigned long long *>(a->errors);
    return SPL_OK;
}

// the same for a backward call
inline int bwd_args(int32_t B, const spl_ppo_net_bwd_t *a, Bwd &g) {
    if (const int e = rows_ok(B)) return e;
    if (!a) return spl_fail(SPL_E_ARG, "null backward arguments");
    if (a->K < 1 || a->T < 1) return spl_fail(SPL_E_ARG, "K and T must be positive");
    if (a->reserved != 0) return spl_fail(SPL_E_ARG, "reserved must be 0");
    if (!a->idx || !a->obs_u8 || mlp_null(a->actor) || mlp_null(a->critic) || !a->dlogits || !a->dvalue || !a->act ||
        grad_null(a->actor_grad) || grad_null(a->critic_grad) || !a->scratch)
        return spl_fail(SPL_E_ARG, "null buffer");
    if (spl_misaligned(a->idx, 16) || spl_misaligned(a->obs_u8, 16) || mlp_misaligned(a->actor) || mlp_misaligned(a->critic) ||
        spl_misaligned(a->dlogits, 16) || spl_misaligned(a->dvalue, 16) || spl_misaligned(a->act, 16) ||
        grad_misaligned(a->actor_grad) || grad_misaligned(a->critic_grad) || spl_misaligned(a->scratch, 16))
        return spl_fail(SPL_E_ARG, "every pointer must be 16-byte aligned");
    g = Bwd{};
    g.B = B;
    g.chunks = chunks_of(B);
    g.parts = parts_of(B);
    g.total = (int64_t)a->K * a->T;
    g.idx = a->idx;
    g.obs = a->obs_u8;
    g.w2[0] = a->actor.w2, g.w2[1] = a->critic.w2;
    g.w3[0] = a->actor.w3, g.w3[1] = a->critic.w3;
    g.dout[0] = a->dlogits, g.dout[1] = a->dvalue;
    g.act = static_cast<const float *>(a->act);
    g.dz = static_cast<float *>(a->scratch);
    g.partial = g.dz + dz_floats(B);
    const spl_ppo_mlp_grad_t *gr[2] = {&a->actor_grad, &a->critic_grad};
    for (int n = 0; n < 2; ++n) {
        g.gw1[n] = gr[n]->w1, g.gb1[n] = gr[n]->b1;
        g.gw2[n] = gr[n]->w2, g.gb2[n] = gr[n]->b2;
        g.gw3[n] = gr[n]->w3, g.gb3[n] = gr[n]->b3;
    }
    return SPL_OK;
}

// The backward's last launch in both sources, k_net_reduce (spl_ppo_net.hip): element e of the partials' layout,
// partials 0, 1, ... in that order, into its gradient
void launch_net_reduce(const Bwd &g, hipStream_t s);

}  // namespace spln
