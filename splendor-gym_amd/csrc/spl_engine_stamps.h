#pragma once
// spl_engine_stamps.h — the SPL_STAMPS diagnostics (tools/stamps.py, tools/wsstamps.py): STAMP / STAMPV / RSTAMP /
// WSHWID and WsStamps, which record s_memrealtime at phase boundaries of the step and rollout kernels, and the
// empty versions the product build compiles them to.
#include "spl_engine_args.h"

namespace spl {

// Phase stamps for the diagnostic build only (-DSPL_STAMPS, tools/stamps.py): lane 0 of every
// wave records s_memrealtime (100 MHz) at phase boundaries of step_ws.  Never in the product build.
#ifdef SPL_STAMPS
__device__ uint64_t *g_stamps;
#define STAMP(i)                                                                                 \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if ((threadIdx.x & 63) == 0 && g_stamps) g_stamps[((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                       \
    } while (0)
// a value instead of a time in stamp slot i (e.g. a wave's terminal-row count)
#define STAMPV(i, v)                                                                             \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0 && g_stamps) g_stamps[((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (i)] = (uint64_t)(v); \
    } while (0)
// k_rollout keeps its stamps in registers (lane k holds step k's) so that stamping never waits
// on the stores in flight; they are written to g_rstamps[wave][step][kRStamps] at the end.
constexpr int kRStamps = 6;
__device__ uint64_t *g_rstamps;
#define RSTAMP(i, k)                                                                             \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        const uint64_t tt_ = __builtin_amdgcn_s_memrealtime();                                   \
        rst_lo[i] = lane_id() == (k) ? (int)(uint32_t)tt_ : rst_lo[i];                           \
        rst_hi[i] = lane_id() == (k) ? (int)(uint32_t)(tt_ >> 32) : rst_hi[i];                   \
        __builtin_amdgcn_sched_barrier(0);                                                       \
    } while (0)
// rollout_ws (k_rollout_store_*, k_rollout_inplace_*): both waves keep kWsStamps stamps per step in registers (lane k = step k, K <= 64),
// written to g_wsstamps[workgroup][wave][step][kWsStamps] at the end.
constexpr int kWsStamps = 11;  // 0-3 per step; 4-10 sub-phases of the rules wave
__device__ uint64_t *g_wsstamps;
__device__ uint32_t *g_wshwid;  // [workgroup][wave][2]: HW_ID (SIMD, CU, SE) and XCC_ID of each wave
__device__ uint64_t *g_wsclk;   // [workgroup][4]: s_memtime / s_memrealtime at the rules wave's start and end
__device__ uint64_t *g_wsend;   // [workgroup][2]: s_memrealtime at the output wave's last step and at its end
#define WSHWID(sid, wave)                                                                        \
    do {                                                                                         \
        if (g_wshwid && lane_id() == 0) {                                                        \
            g_wshwid[((size_t)(sid) * 2 + (wave)) * 2 + 0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  \
            g_wshwid[((size_t)(sid) * 2 + (wave)) * 2 + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20); \
        }                                                                                        \
    } while (0)
// a rules / output wave's stamps of one launch (rules_wave, output_wave): at(i, k) is stamp i of step k
struct WsStamps {
    int rst_lo[kWsStamps] = {0}, rst_hi[kWsStamps] = {0};
    uint64_t clk0 = 0, rt0 = 0;
    struct Sub {  // step_rules' sub-phase hook
        WsStamps &st;
        int k;
        __device__ __forceinline__ void operator()(int i) const { st.at(i, k); }
    };
    __device__ __forceinline__ void at(int i, int k) { RSTAMP(i, k); }
    __device__ __forceinline__ Sub sub(int k) { return Sub{*this, k}; }
    __device__ __forceinline__ void start() {
        clk0 = __builtin_amdgcn_s_memtime();
        rt0 = __builtin_amdgcn_s_memrealtime();
    }
    // the rules wave's clocks from start() to now -> g_wsclk[sid]
    __device__ __forceinline__ void flush_clocks(int sid) const {
        const uint64_t clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
        if (g_wsclk && lane_id() == 0) {
            g_wsclk[sid * 4 + 0] = clk0;
            g_wsclk[sid * 4 + 1] = rt0;
            g_wsclk[sid * 4 + 2] = clk1;
            g_wsclk[sid * 4 + 3] = rt1;
        }
    }
    // the per-step stamps -> g_wsstamps[sid][wave]
    __device__ __forceinline__ void flush(int sid, int wave, int K) const {
        if (g_wsstamps && lane_id() < K)
            for (int i = 0; i < kWsStamps; ++i)
                g_wsstamps[(((size_t)sid * 2 + wave) * 64 + lane_id()) * kWsStamps + i] =
                    ((uint64_t)(uint32_t)rst_hi[i] << 32) | (uint32_t)rst_lo[i];
    }
    // now -> g_wsend[sid][i]; `drained`: once this wave's stores have completed
    __device__ __forceinline__ void end(int sid, int i, bool drained) const {
        if (!g_wsend) return;
        if (drained) __builtin_amdgcn_s_waitcnt(0);
        if (lane_id() == 0) g_wsend[sid * 2 + i] = __builtin_amdgcn_s_memrealtime();
    }
};
#else
#define WSHWID(sid, wave) \
    do {                  \
    } while (0)
struct WsStamps {
    __device__ __forceinline__ void at(int, int) {}
    __device__ __forceinline__ NoStamp sub(int) { return NoStamp(); }
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void flush_clocks(int) const {}
    __device__ __forceinline__ void flush(int, int, int) const {}
    __device__ __forceinline__ void end(int, int, bool) const {}
};
#define STAMP(i) \
    do {         \
    } while (0)
#define STAMPV(i, v) \
    do {             \
    } while (0)
#define RSTAMP(i, k) \
    do {             \
    } while (0)
#endif

}  // namespace spl
