// Shared helpers of libtipk (gfx950 only: 64-wide wavefronts are hard-coded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tipk.h"

#define TIPK_WAVE 64

static inline int tipk_hip_status(hipError_t e) {
    return e == hipSuccess ? TIPK_OK : TIPK_EHIP_BASE - (int)e;
}

// Launch-error check that does not synchronise (safe under stream capture).
#define TIPK_RETURN_LAUNCH()                          \
    do {                                              \
        hipError_t e__ = hipGetLastError();           \
        return tipk_hip_status(e__);                  \
    } while (0)

static inline int64_t tipk_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Host-side options of the library (tipk_api.cpp; include/tipk.h section 0): set explicitly through
// tipk_set_option -- no launch path reads the environment.  The *_DEBUG ids skip parts of a kernel's
// work (timing decompositions, tools/bench_*.py): they exist only in -DTIPK_DEBUG builds, a release
// library refuses them and its kernels carry no skip code.
enum {
    TIPK_OPT_GEMM_NO_STREAM = 0,      // every product through the LDS-tiled kernel
    TIPK_OPT_GEMM_THIN_K_NARROW = 1,  // dword body of the Y = att.XB streaming kernel
    TIPK_OPT_GEMM_STREAM_KK = 2,      // lane-per-row streaming body for d att
    TIPK_OPT_RG_DEBUG = 3,            // debug builds only
    TIPK_OPT_DP_DEBUG = 4,            // debug builds only
    TIPK_OPT_RG_OCCUPANCY = 5,        // tipk_rel_gather: workgroups per CU to aim for (0 = default, 1, 2)
    TIPK_OPT_DM_DEBUG = 6,            // debug builds only (decoder kernels)
    TIPK_OPT_DM_TASK_KERNEL = 7,      // fused objective through distmult_task_kernel (k / 4 lanes per position) -- A/B runs
    TIPK_OPT_SCREEN_SEARCH = 8,       // tipk_distmult_screen: known-pair filter by binary search even where the LDS bitmap fits
    TIPK_OPT_PAIR_TOPK_STREAM = 9,    // tipk_distmult_pair_topk: rel_w streamed through LDS in tiles even where all of it fits
    TIPK_OPT_REGIMEN_GLOBAL = 10,     // tipk_distmult_regimen_topk: rel_w rows read from global memory even where the LDS image fits
    TIPK_OPT_PAIR_RANK_STREAM = 11,   // tipk_distmult_pair_rank: rel_w rows read from global memory even where the LDS image fits
    TIPK_OPT_PARTNER_RANK_GLOBAL = 12, // tipk_distmult_partner_rank: z rows read from global memory even where the LDS image fits
    TIPK_OPT_ADDON_GLOBAL = 13,       // tipk_distmult_addon_burden: rel_w rows read from global memory even where the LDS image fits
    TIPK_OPT_ATTRIBUTION_GLOBAL = 14, // tipk_rgcn_attribution: the per-query table in the caller's workspace even where it fits in LDS
    TIPK_OPT_PARTNER_SUM_GLOBAL = 15, // tipk_distmult_partner_sum: z rows read from global memory even where the LDS image fits
    TIPK_OPT_COMBO_NO_PREFIX = 16,    // tipk_*_combo_burden: every combination sums all its levels (no prefix kept while the last slot advances)
    TIPK_OPT_COMBO_RUN = 17,          // tipk_*_combo_burden: combinations per wavefront run (0 = chosen from the call's size; at most 64)
    TIPK_OPT_COUNT = 18
};
int tipk_option(int id);
#ifdef TIPK_DEBUG
#define TIPK_DBG(expr) (expr)
#else
#define TIPK_DBG(expr) 0
#endif

#ifdef __HIPCC__
__device__ __forceinline__ float4 tipk_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void tipk_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// 16-byte store that does NOT stay in the XCD's L2 (`sc1`, MI355X_MICROARCH.md "stores of each flavour"): for write-once
// output nobody on this XCD reads back -- the 10 GB stream of config 5's transposed pass (kept in L2 it evicts the 5 MB
// table every gathered row comes from), and the pair cells and d att slabs of the stream gathers, which left dirty in
// the write-back L2 drain at the END of their launch, in front of the dependent one.  Written through, scattered
// 128-byte rows leave at well under 1 TB/s: only for a launch whose other work lasts longer than that (DESIGN.md
// section 5, profiles/store_drain.md).  16 bytes per lane only: a dword `sc1` store is one fabric write each, ~6x the
// time per byte.  The compiler pads nothing behind an asm statement: the `s_nop 1` keeps the next VALU write of the data
// registers off a store that is still reading them.
typedef float tipk_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st4_stream(float* p, float4 v) {
    tipk_f4 q = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(q) : "memory");
}
__device__ __forceinline__ int tipk_lane() { return threadIdx.x & (TIPK_WAVE - 1); }
// THE total order of every ranking and selection kernel: score descending, id ascending (a NaN score is better than nothing)
__device__ __forceinline__ bool better(float sa, int ka, float sb, int kb) {
    return sa > sb || (sa == sb && ka < kb);
}
#endif
