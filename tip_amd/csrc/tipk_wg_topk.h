// The one home of what the workgroup-per-query selection kernels share (tipk_screen.hip, tipk_screen_rank.hip,
// tipk_attribution.hip; include/tipk.h sections 4c, 4h, 4j) -- the sibling of tipk_wave_topk.h.  A workgroup of WG_NT
// threads works on ONE QUERY (or one part of it) with its state in LDS.  The screen and the screen rank must agree to the
// bit, and the attribution selects as the screen does, so each piece exists once:
//   known      key_in (binary search in a relation's sorted keys), WgKnown (LDS bitmap of n^2 bits or the key range; build,
//              known)
//   deal       WgDeal (a part's share of the 64 x 64 tiles of the upper triangle, row-major), wg_tiles / wg_splits (host)
//   logits     wg_score_tile (staging of A = z[u rows] * w and Z = z[v rows] transposed, 32 columns at a time, and THE fma
//              loop of a tile, 4 x 4 per thread, k ascending)
//   top-k      WgSel (running threshold, ballot append on three rotating counters, end_round, pad + bitonic cut to k),
//              wg_bitonic (the network over (score, key) under the total order `better` of tipk_common.h; optionally a
//              third array travels along)
// A file keeps its argument struct, the loop structure of its kernel and its LDS declarations, what only it does (the
// screen: the drug blocks, the merge kernel and the workspace layout; the screen rank: target_logit, the histogram and its
// prefix sum; the attribution: stages 1, 2 and 4) and its extern "C" entries.  The selection knows no filter: a caller asks
// WgSel::wants, then WgKnown::known, then appends.
// Barriers: a helper's comment names each __syncthreads() it contains; every other one is the caller's and is written there.
#pragma once
#include "tipk_common.h"
#include <math.h>

constexpr int WG_NT = 256;                 // threads per workgroup
constexpr int WG_TILE = 64;                // rows of the A and Z tiles of a relation query
constexpr int WG_KC = 32;                  // columns of z per staged chunk
constexpr int WG_LD = WG_TILE + 4;         // LDS row stride of the transposed tiles (floats; keeps float4 alignment)
constexpr int WG_SPLIT_MAX = 64;
constexpr int WG_TARGET_WG = 4096;
constexpr int WG_KEY_PAD = 0x7fffffff;     // key of a slot that holds nothing (sorts last)

static inline int64_t wg_tiles(int64_t n) {
    const int64_t nb = (n + WG_TILE - 1) / WG_TILE;
    return nb * (nb + 1) / 2;
}

// parts per query: enough workgroups to fill the chip for few queries, one part per query for thousands of them
static inline int wg_splits(int64_t n, int64_t n_q) {
    int64_t s = n_q > 0 ? WG_TARGET_WG / n_q : 1;
    if (s < 1) s = 1;
    if (s > WG_SPLIT_MAX) s = WG_SPLIT_MAX;
    const int64_t tiles = wg_tiles(n);
    if (s > tiles) s = tiles;
    return (int)s;
}

#ifdef __HIPCC__
__device__ __forceinline__ bool key_in(const int64_t* keys, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t v = keys[mid];
        if (v == x) return true;
        if (v < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

// the known-pair filter of relation r: the LDS bitmap (both directions of every key set) or the relation's range of the
// sorted keys for the search route; neither when there is no list
struct WgKnown {
    const uint32_t* bm;        // LDS bitmap or nullptr
    const int64_t* keys;       // search route, else nullptr
    int64_t klo, khi;
    int n;

    // by the whole workgroup of NT threads; lds: n^2 bits, written on the bitmap route only.  Contains ONE __syncthreads(),
    // between the clear and the ORs (the bitmap route is uniform).  The barrier AFTER, before the first known(), is the
    // caller's.
    template <int NT>
    __device__ __forceinline__ void build(uint32_t* lds, const int64_t* all_keys, const int64_t* kptr, int r, int n_nodes,
                                          int bitmap) {
        const int t = threadIdx.x;
        bm = nullptr; keys = nullptr; klo = khi = 0;
        n = n_nodes;
        if (all_keys) {
            klo = kptr[r];
            khi = kptr[r + 1];
            if (bitmap) {
                const int words = (int)(((int64_t)n * n + 31) / 32);
                for (int i = t; i < words; i += NT) lds[i] = 0u;
                __syncthreads();                                   // cleared before any bit is set
                const int64_t nn = (int64_t)n * n;
                for (int64_t e = klo + t; e < khi; e += NT) {
                    const int64_t key = all_keys[e];
                    if (key < 0 || key >= nn) continue;
                    const int x = (int)(key / n), y = (int)(key % n);
                    const uint32_t b0 = (uint32_t)(x * n + y), b1 = (uint32_t)(y * n + x);
                    atomicOr(&lds[b0 >> 5], 1u << (b0 & 31));
                    atomicOr(&lds[b1 >> 5], 1u << (b1 & 31));
                }
                bm = lds;
            } else {
                keys = all_keys;
            }
        }
    }

    // the pair (u, v), u != v, both in [0, n), is listed in either direction
    __device__ __forceinline__ bool known(int u, int v) const {
        if (bm) {
            const uint32_t b = (uint32_t)(u * n + v);
            return (bm[b >> 5] >> (b & 31)) & 1u;
        }
        if (keys) return key_in(keys, klo, khi, (int64_t)u * n + v) || key_in(keys, klo, khi, (int64_t)v * n + u);
        return false;
    }
};

// part `part` of `splits` of the tiles (bu <= bv) of the upper triangle in row-major order: tiles [t0, t1), the first one
// at (bu, bv)
struct WgDeal {
    int64_t t0, t1;
    int nb, bu, bv;

    __device__ __forceinline__ WgDeal(int n, int part, int splits) {
        nb = (n + WG_TILE - 1) / WG_TILE;
        const int64_t n_tiles = (int64_t)nb * (nb + 1) / 2;
        t0 = n_tiles * part / splits;
        t1 = n_tiles * (part + 1) / splits;
        bu = 0;
        int64_t row_start = 0;                                  // linear index of tile (bu, bu)
        while (t0 < t1 && t0 >= row_start + (nb - bu)) { row_start += nb - bu; ++bu; }
        bv = bu + (int)(t0 - row_start);
    }
    __device__ __forceinline__ void next() { if (++bv == nb) { ++bu; bv = bu; } }
};

// One tile by the WG_NT threads: onto acc[i][j], which the caller has cleared (in the header the clear costs both kernels
// 40 instructions), comes the logit of (u, v) = (bu * 64 + 4 * ty + i, bv * 64 + 4 * tx + j), ty = t >> 4, tx = t & 15:
// x = z[u][k] * wl[k] rounded once, acc = fmaf(x, z[v][k], acc), k ascending (rows past n count as zero).
// Contains TWO __syncthreads() per chunk of WG_KC columns: one before the staging (the previous chunk, or tile, has been
// read) and one after it.  None follows the last fma loop: acc is in registers, and the next tile's first barrier guards
// As and Zs.
__device__ __forceinline__ void wg_score_tile(float* As, float* Zs, const float* z, const float* wl, int n, int dim, int bu,
                                              int bv, float (&acc)[4][4]) {
    const int t = threadIdx.x;
    const int ty = t >> 4, tx = t & 15;
    for (int k0 = 0; k0 < dim; k0 += WG_KC) {
        const int kc = dim - k0 < WG_KC ? dim - k0 : WG_KC;
        __syncthreads();                                         // the previous chunk has been read
        for (int idx = t; idx < 2 * WG_TILE * (WG_KC / 4); idx += WG_NT) {
            const int which = idx / (WG_TILE * (WG_KC / 4));
            const int rem = idx % (WG_TILE * (WG_KC / 4));
            const int row = rem >> 3, qd = rem & 7;
            if (4 * qd >= kc) continue;
            const int node = (which == 0 ? bu : bv) * WG_TILE + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (node < n) v = tipk_ld4(z + (int64_t)node * dim + k0 + 4 * qd);
            float* dst = which == 0 ? As : Zs;
            if (which == 0) {
                const int kk = k0 + 4 * qd;
                v.x *= wl[kk]; v.y *= wl[kk + 1]; v.z *= wl[kk + 2]; v.w *= wl[kk + 3];
            }
            dst[(4 * qd + 0) * WG_LD + row] = v.x;
            dst[(4 * qd + 1) * WG_LD + row] = v.y;
            dst[(4 * qd + 2) * WG_LD + row] = v.z;
            dst[(4 * qd + 3) * WG_LD + row] = v.w;
        }
        __syncthreads();                                         // the chunk is staged
        for (int kk = 0; kk < kc; ++kk) {
            const float4 av = *reinterpret_cast<const float4*>(&As[kk * WG_LD + 4 * ty]);
            const float4 zv = *reinterpret_cast<const float4*>(&Zs[kk * WG_LD + 4 * tx]);
            const float ar[4] = {av.x, av.y, av.z, av.w}, zr[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], zr[j], acc[i][j]);
        }
    }
}

// The bitonic network: the p entries (p a power of two >= 2) of (s, k) in LDS best first under `better`, by the whole
// workgroup of NT threads; TAG: every entry carries an int in tag that moves with it.  Contains ONE __syncthreads() after
// every pass (log2(p) * (log2(p) + 1) / 2 of them).  The barrier BEFORE (the entries are written) is the caller's.
template <int NT, bool TAG>
__device__ __forceinline__ void wg_bitonic(float* s, int* k, int* tag, int p) {
    const int t = threadIdx.x;
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = t; x < (p >> 1); x += NT) {
                const int i = 2 * stride * (x / stride) + (x % stride), j = i + stride;
                const float si = s[i], sj = s[j];
                const int ki = k[i], kj = k[j];
                const bool up = (i & size) == 0;
                if (up ? better(sj, kj, si, ki) : better(si, ki, sj, kj)) {
                    s[i] = sj; k[i] = kj; s[j] = si; k[j] = ki;
                    if (TAG) { const int ii = tag[i]; tag[i] = tag[j]; tag[j] = ii; }
                }
            }
            __syncthreads();
        }
    }
}

// The selection of a workgroup of NT threads: the k best (score, key) of everything appended, in an LDS buffer of CAP
// entries (a power of two >= k + ROUND; ROUND = most appends between two end_round()).  A candidate below the running
// threshold (the k-th best kept so far) is dropped before it is appended, which is exact: k kept entries are better.  The
// result is a set defined by the total order, so it does not depend on the order of the appends.  The caller clears
// ctr[0..2] and has a barrier between that and the first append.
template <int NT, int CAP, int ROUND>
struct WgSel {
    float* bs;
    int* bk;
    unsigned* ctr;             // [3] rotating append counters (one barrier per round)
    int k;
    int c;                     // entries in the buffer (uniform)
    int rr;                    // round number (uniform)
    float thr;

    __device__ __forceinline__ void init(float* s, int* keys, unsigned* counters, int k_) {
        bs = s; bk = keys; ctr = counters; k = k_; c = 0; rr = 0; thr = -INFINITY;
    }

    // a candidate worth appending: not below the threshold; NaN never passes
    __device__ __forceinline__ bool wants(bool ok, float s) const { return ok && s >= thr; }

    // every lane calls this (uniform control flow): append (s, key) where pass.  No barrier.
    __device__ __forceinline__ void append(bool pass, float s, int key) {
        const unsigned long long mask = __ballot(pass);
        if (mask == 0ull) return;
        const int lane = tipk_lane();
        const int leader = __ffsll((long long)mask) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&ctr[rr % 3], (unsigned)__popcll(mask));
        base = __shfl(base, leader);
        if (pass) {
            const unsigned pos = (unsigned)c + base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            bs[pos] = s;
            bk[pos] = key;
        }
    }

    // sort the c entries best first and keep k of them (every thread, uniform).  Contains ONE __syncthreads() after the pad
    // fill and those of wg_bitonic, the last of them after the last pass.  The barrier BEFORE (the appends are visible) is
    // end_round()'s.
    __device__ void flush() {
        int p = 2;
        while (p < c) p <<= 1;
        for (int i = c + (int)threadIdx.x; i < p; i += NT) { bs[i] = -INFINITY; bk[i] = WG_KEY_PAD; }
        __syncthreads();
        wg_bitonic<NT, false>(bs, bk, nullptr, p);
        c = c < k ? c : k;
        thr = c == k ? bs[k - 1] : -INFINITY;
    }

    // end of a round: ONE __syncthreads() (everything appended is visible), c moves on, the counter of round rr - 1 is
    // cleared for rr + 2; then flush() when the next round could overflow the buffer
    __device__ __forceinline__ void end_round() {
        __syncthreads();
        c += (int)ctr[rr % 3];
        if (threadIdx.x == 0) ctr[(rr + 2) % 3] = 0u;
        ++rr;
        if (c > CAP - ROUND) flush();
    }
};
#endif
