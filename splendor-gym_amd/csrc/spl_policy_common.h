// spl_policy_common.h — what the two actor translation units (spl_policy.hip: bf16, spl_policy32.hip:
// the fp32 formats) share: the network a pack kernel reads, the wave-level LDS hand-off, the action
// draw of the sampling epilogues, and the entry points spl_policy.hip forwards the fp32 images to.
#pragma once
#include "../../include/splendor_policy.h"
#include "spl_common.h"
#include "spl_rng.h"

namespace splpol {

// one MLP as a pack kernel takes it: Linear(297,256)-Tanh-Linear(256,256)-Tanh-Linear(256,out)
struct PackNet {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int out;
};
inline PackNet pack_net(const spl_mlp_t *m, int out) { return PackNet{m->w1, m->b1, m->w2, m->b2, m->w3, m->b3, out}; }

using spl::kActions;
using spl::kObsDim;
using spl::wave_lds_sync;

typedef __attribute__((address_space(3))) void lds_void;

// The sampling epilogues' draw for one table at one ply: uniform in [0, 1) with 24 bits, from the
// Philox block keyed (table, ply | seed ^ the actors' stream constant).  One function for every
// precision, so that the same (seed, ply, table) gives the bf16 and the fp32 actors the same draw.
__device__ __forceinline__ float action_uniform(uint64_t seed, uint64_t ply, int64_t table) {
    const uint4 rnd = spl::philox4x32(make_uint4((uint32_t)table, (uint32_t)((uint64_t)table >> 32), (uint32_t)ply,
                                                 (uint32_t)(ply >> 32)),
                                      make_uint2((uint32_t)seed, (uint32_t)(seed >> 32) ^ 0xA5C3E1F7u));
    return (float)(rnd.x >> 8) * (1.f / 16777216.f);
}

}  // namespace splpol

// ---- spl_policy32.hip: the fp32 images; fmt 0 = exact three bf16 planes (SPL_PREC_FP32), 1 = two fp16
// planes (SPL_PREC_FP32_F16X2)
int64_t splp32_bytes(int with_critic, int fmt);
int splp32_pack(const spl_mlp_t *actor, const spl_mlp_t *critic, void *packed, void *stream, int fmt);
// image: a packed image of format `fmt` (full when has_critic); critic: evaluate the critic (SAMPLE
// with value, or alone when !sample); groups > 0: `groups` actor-only images image_stride apart, table i
// served by image group_of[i], scratch of splp32_group_scratch(n, groups) bytes
int splp32_act(const uint8_t *img, bool has_critic, bool critic, bool sample, int32_t n, const spl_act_args_t *args,
               void *stream, int fmt, int groups = 0, int64_t image_stride = 0, const int32_t *group_of = nullptr,
               void *scratch = nullptr);
int64_t splp32_group_scratch(int32_t n, int32_t groups);
