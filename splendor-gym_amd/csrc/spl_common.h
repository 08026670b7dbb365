// spl_common.h — what every translation unit of the library shares: the error channel behind
// spl_last_error(), the check behind a kernel launch, pointer alignment, the observation and action
// sizes, and the wave-level LDS hand-off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/splendor_amd.h"

int spl_fail(int code, const std::string &msg);  // spl_engine.hip: sets spl_last_error(), returns code

// behind a kernel launch: SPL_OK, or SPL_E_HIP with "<what>: <the HIP error's text>"
inline int spl_launched(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SPL_OK : spl_fail(SPL_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// p is not a multiple of a (a power of two)
inline bool spl_misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

namespace spl {

constexpr int kObsDim = SPL_OBS_DIM;
constexpr int kObsU8 = 300;  // compact observation row (spl_step_args_t.obs_u8): 297 bytes + move_count >> 8 + 2 zero
constexpr int kActions = SPL_NUM_ACTIONS;

// Cross-lane LDS hand-off inside ONE wave: this wave's LDS writes are visible to its own lanes' reads
// behind this.  __syncthreads() would also emit s_waitcnt vmcnt(0): the wave would stall until its
// pending global stores drain behind every other wave's observation traffic.  LDS executes one wave's
// operations in order, so ordering the compiler (wavefront fence) and the LDS counter suffices.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
    __builtin_amdgcn_wave_barrier();
}

}  // namespace spl
