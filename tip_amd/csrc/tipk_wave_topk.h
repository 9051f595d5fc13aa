// The one home of what the wave-per-row kernels share (tipk_pair_topk.hip, tipk_regimen_topk.hip, tipk_pair_rank.hip,
// tipk_partner_rank.hip, tipk_addon_burden.hip; include/tipk.h sections 4d, 4e, 4f, 4g, 4i).  A workgroup of WT_NT threads
// takes blocks of WT_NW rows (pairs, regimens, queries, tasks), ONE WAVEFRONT PER ROW.  The kernels must agree to the bit, so each piece exists once:
//   logits     wt_stage_rows (LDS image, bank-spreading stride wt_stride), wt_write_row / wt_row16 (the wave's product row
//              and its dim-16 register copy), wt_dot (THE fma chain, k ascending), wt_softplus (the noisy-or term)
//   known      find_key, wt_lower_bound (64-ary searches), wt_merge_window (ids of a window -> bits), wt_bit
//   rank       wt_target_range, wt_count_beaten, wt_write_rank, under the total order `better` (tipk_common.h)
//   top-k      wt_flush_at, flush (bitonic cut to k); the ballot append and the padded write-out stay written out in the two
//              top-k kernels, where as helpers (and with wt_bit) they cost the table variants 1 % (see
//              profiles/wave_rows_refactor.md)
//   host       the WT_* limits and modes, wt_distmult_shape / wt_table_shape, wt_known_ok, wt_fits_lds, wt_grid, wt_launch
// A file keeps its argument struct, the loop structure of its kernel, its fixed-LDS formula and its extern "C" entries.
// Fences: a helper's comment names the wave_sync() it contains; every other one is the caller's and is written there.
#pragma once
#include "tipk_common.h"
#include <math.h>

constexpr int WT_NT = 1024;                 // threads per workgroup
constexpr int WT_NW = WT_NT / TIPK_WAVE;    // rows per block (one per wavefront)
constexpr int WT_CAP = 256;                 // top-k buffer entries per wave
constexpr int WT_KMAX = 128;
constexpr int WT_DIM_MAX = 256;
constexpr int64_t WT_NMAX = 46340;          // n^2 < 2^31
constexpr int64_t WT_RMAX = 65536;
constexpr int WT_WIN = 2048;                // ids per bitmap window (64 words: lane l clears word l)
constexpr int WT_LDS_BYTES = 152 * 1024;    // dynamic LDS a workgroup may ask for
constexpr int WT_REL_PAD = 0x7fffffff;      // id of a slot that holds nothing (sorts last, lies in no window)

enum { WT_DISTMULT = 0, WT_DISTMULT16 = 1, WT_TABLE = 2 };

// LDS row stride of the image: dim or dim + 4 floats, whichever has stride / 4 odd, so the 16 lanes of a
// ds_read_b128 group start on 16 different groups of 4 banks
static inline int wt_stride(int dim) { return ((dim >> 2) & 1) ? dim : dim + 4; }

static inline int wt_cu_count() {
    int dev = 0, n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    return n_cu;
}

// the shapes the table and the DistMult entries take (an axis a route does not depend on is passed as 1)
static inline bool wt_table_shape(int64_t n_nodes, int64_t n_rel) {
    return n_nodes >= 1 && n_nodes <= WT_NMAX && n_rel >= 1 && n_rel <= WT_RMAX;
}
static inline bool wt_distmult_shape(int64_t n_nodes, int dim, int64_t n_rel) {
    return wt_table_shape(n_nodes, n_rel) && dim >= 4 && dim <= WT_DIM_MAX && dim % 4 == 0;
}

// a pair-major known list comes whole or not at all
static inline bool wt_known_ok(const int64_t* keys, const int64_t* kptr, const int32_t* krel) {
    const int given = (keys != nullptr) + (kptr != nullptr) + (krel != nullptr);
    return given == 0 || given == 3;
}

// an image of `rows` rows fits beside `fixed` bytes of per-wave state
static inline bool wt_fits_lds(int64_t rows, int dim, int64_t fixed) {
    return rows * wt_stride(dim) * 4 + fixed <= WT_LDS_BYTES;
}

// persistent grid: a workgroup per block of WT_NW rows, at most per_cu on every CU
static inline int wt_grid(int64_t n_rows, int per_cu) {
    const int64_t n_blocks = (n_rows + WT_NW - 1) / WT_NW, most = (int64_t)per_cu * wt_cu_count();
    return (int)(n_blocks < most ? n_blocks : most);
}

#ifdef __HIPCC__
template <auto KERNEL, class Args>
static int wt_launch(const Args& a, int grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(WT_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

__device__ __forceinline__ void wave_sync() {                  // LDS written by this wave is visible to this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows [row0, row0 + rows) of src [. x dim] into the LDS image Ws (row stride `stride` floats), by the whole workgroup of
// NT threads.  No fence inside: the caller's __syncthreads() follows (and, where the image is reused, precedes).
template <int NT>
__device__ __forceinline__ void wt_stage_rows(float* Ws, const float* src, int row0, int rows, int dim, int stride) {
    const int q4 = dim >> 2;
    for (int idx = threadIdx.x; idx < rows * q4; idx += NT) {
        const int row = idx / q4, q = idx - row * q4;
        tipk_st4(Ws + row * stride + 4 * q, tipk_ld4(src + (int64_t)(row0 + row) * dim + 4 * q));
    }
}

// the wave's product row hs[k] = x[k] * y[k], rounded once.  No fence inside: the caller issues wave_sync() before (the
// row's previous readers are done) and after (before wt_row16 or wt_dot read it).
__device__ __forceinline__ void wt_write_row(float* hs, const float* x, const float* y, int dim, int lane) {
    for (int kk = lane; kk < dim; kk += TIPK_WAVE) hs[kk] = x[kk] * y[kk];
}

// dim 16: the product row as registers.  Reads hs: the caller has issued wave_sync() since wt_write_row.
template <int MODE>
__device__ __forceinline__ void wt_row16(float4* hq, const float* hs) {
    if (MODE == WT_DISTMULT16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const float4*>(hs + 4 * q);
    }
}

// THE logit: acc = fmaf(h[k], w[k], acc), k ascending; wr = the candidate's row (LDS image or global), h = the wave's
// product row, hq (dim 16) or hs (general, read from LDS: wave_sync() issued since wt_write_row).  No fence inside.
template <int MODE>
__device__ __forceinline__ float wt_dot(const float* wr, const float* hs, const float4* hq, int dim) {
    float s = 0.f;
    if (MODE == WT_DISTMULT16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 w4 = *reinterpret_cast<const float4*>(wr + 4 * q);
            s = fmaf(hq[q].x, w4.x, s);
            s = fmaf(hq[q].y, w4.y, s);
            s = fmaf(hq[q].z, w4.z, s);
            s = fmaf(hq[q].w, w4.w, s);
        }
    } else {
        for (int k0 = 0; k0 < dim; k0 += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wr + k0);
            const float4 h4 = *reinterpret_cast<const float4*>(hs + k0);
            s = fmaf(h4.x, w4.x, s);
            s = fmaf(h4.y, w4.y, s);
            s = fmaf(h4.z, w4.z, s);
            s = fmaf(h4.w, w4.w, s);
        }
    }
    return s;
}

// the noisy-or term of a logit (sections 4e, 4i): -log(1 - sigma(s))
__device__ __forceinline__ float wt_softplus(float s) { return fmaxf(s, 0.f) + log1pf(expf(-fabsf(s))); }

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

// first index in [lo, hi) whose ascending a[] is >= x (hi if none): every lane calls it with the same arguments and gets
// the same answer; the 64 lanes probe 64 entries per step
template <class T>
static __device__ int64_t wt_lower_bound(const T* a, int64_t lo, int64_t hi, T x, int lane) {
    while (hi - lo > TIPK_WAVE) {
        const int64_t step = (hi - lo + TIPK_WAVE - 1) / TIPK_WAVE;
        const int64_t idx = lo + (int64_t)lane * step;
        const int c = __popcll(__ballot(idx < hi && a[idx] < x));   // the probes ascend: the lanes below x are a prefix
        if (c == 0) return lo;
        const int64_t top = lo + (int64_t)c * step;
        lo += (int64_t)(c - 1) * step + 1;                           // a[lo - 1] < x <= a[top] (or top is past the end)
        hi = top < hi ? top : hi;
    }
    const int64_t idx = lo + lane;
    return lo + __popcll(__ballot(idx < hi && a[idx] < x));
}

// the listed ids of the window [c0, c1) as bits of km; id_at(idx) is the ascending id at list position idx, the list ends
// at kend, and the cursor kc only moves forward: it passes every id below c1.  WORDS = bitmap words of a window (at most
// 64, a lane each).  Contains ONE wave_sync(), between the clear and the ORs.  The caller issues the fence BEFORE (the
// previous window's bits have been read) unless one is already there, and the fence AFTER, before the first wt_bit.
template <int WORDS, class IdAt>
__device__ __forceinline__ void wt_merge_window(uint32_t* km, int64_t& kc, int64_t kend, int c0, int c1, int lane,
                                                IdAt id_at) {
    if (WORDS == TIPK_WAVE || lane < WORDS) km[lane] = 0u;
    wave_sync();
    for (;;) {
        const int64_t idx = kc + lane;
        const auto x = idx < kend ? id_at(idx) : WT_REL_PAD;
        const bool below = x < c1;
        if (below && x >= c0) atomicOr(&km[(int)(x - c0) >> 5], 1u << ((int)(x - c0) & 31));
        const int nb = __popcll(__ballot(below));
        kc += nb;
        if (nb < TIPK_WAVE) break;
    }
}

// bit `bit` of the window's bitmap (wave_sync() issued since wt_merge_window)
__device__ __forceinline__ bool wt_bit(const uint32_t* km, int bit) { return (km[bit >> 5] >> (bit & 31)) & 1u; }

// the targets [tb, te) of `row`, cut to [0, n_tgt): device lists cannot be validated on the host, and nothing outside
// [0, n_tgt) is read or written.  false: no targets.
__device__ __forceinline__ bool wt_target_range(const int64_t* tptr, int64_t row, int64_t n_tgt, int64_t& tb, int64_t& te) {
    tb = tptr[row];
    te = tptr[row + 1];
    tb = tb < 0 ? 0 : tb;
    te = te > n_tgt ? n_tgt : te;
    return tb < te;
}

// one window of 64 candidates (s, id: one per lane, NaN beats nothing) against the chunk's nt targets (ts, tid: target j in
// lane j): the number of candidates that beat target j is added to lane j's cnt.  No LDS traffic, no fence.
__device__ __forceinline__ void wt_count_beaten(int& cnt, float s, int id, float ts, int tid, int nt, int lane) {
    for (int j = 0; j < nt; ++j) {
        const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ts), j));
        const int tj = __builtin_amdgcn_readlane(tid, j);
        const int beat = __popcll(__ballot(better(s, id, sj, tj)));
        cnt += lane == j ? beat : 0;
    }
}

// lane j < nt writes target j of the chunk at `ch`: (1 + cnt, ts), or (0, NaN) when it is not ranked (not ok, or a NaN
// logit); out_logit nullable
__device__ __forceinline__ void wt_write_rank(int32_t* out_rank, float* out_logit, int64_t ch, int nt, bool ok, int cnt,
                                              float ts, int lane) {
    if (lane < nt) {
        const bool ranked = ok && ts == ts;
        out_rank[ch + lane] = ranked ? 1 + cnt : 0;
        if (out_logit) out_logit[ch + lane] = ranked ? ts : NAN;
    }
}

// sort the wave's c buffer entries best first and keep k of them (the whole wave, uniform); TAG: every entry carries a
// 16-bit tag in bt that moves with it.  Fenced on both sides of every LDS pass: the caller needs none.
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

// buffer fill at which the wave cuts back to k: max(64, 2k), at most WT_CAP - 64, so k < flush_at <= 192
__device__ __forceinline__ int wt_flush_at(int k) { return k > 32 ? (2 * k < WT_CAP - 64 ? 2 * k : WT_CAP - 64) : 64; }
#endif
