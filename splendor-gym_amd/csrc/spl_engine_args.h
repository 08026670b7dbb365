#pragma once
// spl_engine_args.h — the engine's bottom layer, part 1: what a kernel is handed and how a build is switched.
// The kernel argument blocks (KArena / KTables / KStep), SPL_ABL for profiling builds, SPL_CHECK and the BC_* bits
// for the bounds-check build, lane_id, and the empty stamp hook of the product build.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spl {

// ------------------------------------------------------------------------------------------
// kernel parameter blocks
// ------------------------------------------------------------------------------------------
struct KArena {
    uint32_t *planes;  // [num_words(P)][n] table state
    uint32_t *pool;    // [PL_COUNT][n] pool deal's board / noble words
    uint8_t *slots;    // [n][2][128] deck records
    uint8_t *pcg;      // [n][64] engine-seed streams
    int n;
    uint8_t *deleg;    // [n/128][kDelegTasks][num_words(P) x 64] u32 staged state words (rollout-store delegation)
    uint32_t *dflags;  // [n/128][kDelegFlagWords] its flags
    uint32_t *legal;   // [2][n] legal-mask cache of the stored state (spl_layout.h)
};

struct KTables {
    const uint4 *cards;   // [90] {1,tier,points,oh_w | oh_b..oh_k | cost w,b,g,r | cost k,colour,0,0}
    const uint2 *nobles;  // [10] {1,req w,b,g | req r,k,points,0}
    const uint4 *lut;     // [kLutEntries] token-return MT outputs (top 3 bits, 10 per word)
    uint32_t mtag;        // this context's legal-mask cache tag (bits 0-15: 1..65535) | kTagFreeCard
};
// Bit 31 of KTables::mtag: the card table has a card of total cost 0, so a fresh deal may allow a purchase and
// reset lanes evaluate legal_moves instead of taking kFreshDealMask.  Set at context creation; a kernel argument,
// so the branch on it is wave-uniform, and it rides in the tag's word, so it costs the kernels no register.
constexpr uint32_t kTagFreeCard = 1u << 31;
__device__ __forceinline__ bool has_free_card(const KTables &Tb) { return (Tb.mtag & kTagFreeCard) != 0u; }

struct KStep {
    const int32_t *actions;
    int32_t *obs;
    int8_t *mask;
    float *reward;
    uint8_t *terminated;
    uint8_t *flags;
    int8_t *winner;
    int32_t *final_obs;
    int32_t *next_actions;
    float *ep_return;
    uint32_t *ep_count;
    uint8_t *info;             // nullable: [4][n] info planes + truncated (spl_step)
    uint8_t *obs_u8;           // nullable: [n][300] compact observation instead of obs (k_step_ws)
    const uint8_t *gate_terminated, *gate_flags;  // nullable: the dual step's gate (spl_step_args_t)
    unsigned long long *errors;  // nullable: running count of tables with an error flag (spl_step)
    const uint64_t *ply_base;  // nullable: device counter added to `ply` (graph replays)
    uint64_t *fault;           // nullable: the context's host-mapped fault word (spl_ctx_faults)
    uint64_t fault_tag;        // what a faulting launch writes there (the context's launch serial)
    uint64_t policy_seed;
    uint64_t ply;
    int64_t table0;
    int autoreset;
    int policy;
};

// Ablation switches for profiling builds only (tools/ablate.py); the product build defines none.
#ifndef SPL_ABL
#define SPL_ABL 0
#endif
// (bits 16, 64, 512 and 2048 belonged to the one-wave step kernel; the others keep the values past profiles quote)
constexpr int ABL_LEGAL_PRE = 1, ABL_APPLY = 2, ABL_LEGAL_POST = 4, ABL_FINAL = 8, ABL_ENCODE = 32,
              ABL_MASK_STORE = 128, ABL_SMALL_OUT = 256, ABL_OBS_STORE = 1024,
              ABL_TOKLIM = 4096, ABL_NOBLE = 8192, ABL_DECK_GATHER = 16384, ABL_LUT_GATHER = 32768;
__device__ __forceinline__ bool abl(int bit) { return (SPL_ABL & bit) != 0; }

// Bounds-check build (-DSPL_BOUNDS_CHECK; libsplendor_amd_checked.so, tests/test_gpu_bounds_check.py):
// index and range invariants are tested at run time and violations recorded as bits of
// g_bounds_flags (an atomic OR: a checked run never faults, it reports).  The product build
// compiles every check out.
#ifdef SPL_BOUNDS_CHECK
__device__ uint32_t g_bounds_flags;
#define SPL_CHECK(cond, bit)                                              \
    do {                                                                  \
        if (!(cond)) atomicOr(&g_bounds_flags, (uint32_t)(bit));          \
    } while (0)
#else
#define SPL_CHECK(cond, bit) \
    do {                     \
    } while (0)
#endif
enum : uint32_t {
    BC_TABLE = 1, BC_SLOT = 2, BC_DECK = 4, BC_LUT = 8, BC_SCRATCH = 16, BC_BYTE = 32, BC_ROWS = 64, BC_CARD = 128,
    BC_SPIN = 256,  // a wave gave up waiting for an LDS hand-off (dealer rollout)
    BC_BARRIER = 512  // a wave of a multi-team workgroup made another number of s_barriers than 1 + K
};

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
// sub-phase stamp hook of step_rules (diagnostic builds pass a stamping one)
struct NoStamp {
    __device__ __forceinline__ void operator()(int) const {}
};

}  // namespace spl
