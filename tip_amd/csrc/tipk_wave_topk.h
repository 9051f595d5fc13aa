// What the wave-per-row kernels share (tipk_pair_topk.hip, tipk_regimen_topk.hip, tipk_pair_rank.hip, tipk_partner_rank.hip;
// include/tipk.h sections 4d, 4e, 4f, 4g):
// the wavefront-local LDS fence, the total order, the 64-ary key search, the bitonic cut of a wave's candidate buffer and
// the bank-spreading row stride of the rel_w image.
#pragma once
#include "tipk_common.h"
#include <math.h>

constexpr int WT_REL_PAD = 0x7fffffff;      // relation id of a buffer slot that holds no candidate (sorts last)

// LDS row stride of the rel_w image: dim or dim + 4 floats, whichever has stride / 4 odd, so the 16 lanes of a
// ds_read_b128 group start on 16 different groups of 4 banks
static inline int wt_stride(int dim) { return ((dim >> 2) & 1) ? dim : dim + 4; }

static inline int wt_cu_count() {
    int dev = 0, n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    return n_cu;
}

#ifdef __HIPCC__
__device__ __forceinline__ void wave_sync() {                  // LDS written by this wave is visible to this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool better(float sa, int ra, float sb, int rb) {
    return sa > sb || (sa == sb && ra < rb);
}

// index of `key` in the strictly ascending keys [0, n), or -1: every lane calls it with the same arguments and gets the
// same answer; the 64 lanes probe 64 keys per step
static __device__ int64_t find_key(const int64_t* keys, int64_t n, int64_t key, int lane) {
    const int64_t big = 0x7fffffffffffffffLL;
    int64_t lo = 0, hi = n;
    while (hi - lo > TIPK_WAVE) {
        const int64_t step = (hi - lo + TIPK_WAVE - 1) / TIPK_WAVE;
        const int64_t idx = lo + (int64_t)lane * step;
        const int64_t v = idx < hi ? keys[idx] : big;
        const int c = __popcll(__ballot(v <= key));              // the probes ascend: the lanes with v <= key are a prefix
        if (c == 0) return -1;
        lo += (int64_t)(c - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    const int64_t idx = lo + lane;
    const int64_t v = idx < hi ? keys[idx] : big;
    const unsigned long long m = __ballot(idx < hi && v == key);
    return m ? lo + (__ffsll((long long)m) - 1) : -1;
}

// sort the wave's c buffer entries best first and keep k of them (the whole wave, uniform); TAG: every entry carries a
// 16-bit tag in bt that moves with it
template <bool TAG>
static __device__ void flush(float* bs, int* br, uint16_t* bt, int& c, float& thr, int k, int lane) {
    int p = TIPK_WAVE;
    while (p < c) p <<= 1;
    wave_sync();
    for (int i = c + lane; i < p; i += TIPK_WAVE) { bs[i] = -INFINITY; br[i] = WT_REL_PAD; }
    wave_sync();
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = lane; x < (p >> 1); x += TIPK_WAVE) {
                const int i = 2 * stride * (x / stride) + (x % stride), j = i + stride;
                const float si = bs[i], sj = bs[j];
                const int ri = br[i], rj = br[j];
                const bool up = (i & size) == 0;
                if (up ? better(sj, rj, si, ri) : better(si, ri, sj, rj)) {
                    bs[i] = sj; br[i] = rj; bs[j] = si; br[j] = ri;
                    if (TAG) { const uint16_t ti = bt[i]; bt[i] = bt[j]; bt[j] = ti; }
                }
            }
            wave_sync();
        }
    }
    c = c < k ? c : k;
    thr = c == k ? bs[k - 1] : -INFINITY;
}
#endif
