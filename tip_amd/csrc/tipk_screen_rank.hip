// Screen rank: the filtered rank of given drug pairs (held-out pairs) among all unordered pairs, per relation query
// (include/tipk.h section 4h) -- the evaluation of what the screen's relation queries (4c) serve.
//
// Two launches, nothing on the host.
// screen_rank_init_kernel (a workgroup per query): every target's logit and whether it is ranked; writes out_logit and
//   out_rank = 1 (ranked) or 0 (not ranked: the final value).
// screen_rank_kernel (n_q x S workgroups of 256 threads, S and the deal of the 64 x 64 tiles of the upper triangle are
//   wg_splits and WgDeal of tipk_wg_topk.h, the screen's): per chunk of SR_CHUNK targets of its query the workgroup
//     1. computes the chunk's target logits (the init kernel's function: same bits) and sorts them best first in LDS
//        under the total order of 4c (logit desc, key asc; wg_bitonic); targets that are not ranked sort last;
//     2. streams its tiles through wg_score_tile, the screen's staging and 4 x 4-per-thread fmaf loop -- one function,
//        so a candidate's logit is the screen's, and a target's logit is its own candidate's;
//     3. for a candidate that beats the chunk's WEAKEST target (the order is total: one that does not beats none) and is
//        not a known pair (WgKnown: LDS bitmap or binary search, consulted only now) finds by binary search the first
//        sorted target it beats and adds 1 to that position's LDS bucket;
//     4. turns the buckets into an inclusive prefix sum -- the target at sorted position j is beaten by sum_{p <= j} of them
//        in this part -- and adds it to out_rank with an integer atomic.
//   The order is irreflexive: a target never counts itself or its repeats, listed or not.  A NaN candidate beats nothing.
//   The counts are integers, so the sum over parts and chunks does not depend on the order of the atomics.
#include "tipk_wg_topk.h"

namespace {

constexpr int SR_NT = WG_NT;               // threads per workgroup
constexpr int SR_CHUNK = 2048;             // targets of one query ranked per pass (power of two)
constexpr int SR_PER = SR_CHUNK / SR_NT;   // buckets a thread sums in the prefix step
constexpr int SR_DIM_MAX = 256;
constexpr int64_t SR_NMAX = 46340;         // n^2 < 2^31: a key a*n+b is an int32
constexpr int64_t SR_RMAX = 65536;

struct ScreenRankArgs {
    const float* z;
    const float* w;
    const int32_t* qrel;       // [n_q]
    const int64_t* tptr;       // [n_q + 1]
    const int32_t* tu;         // [n_tgt]
    const int32_t* tv;
    const int64_t* keys;       // nullable
    const int64_t* kptr;       // [n_rel + 1], nullable with keys
    int64_t n_q, n_tgt;
    int n, dim, n_rel, splits, bitmap;
    int32_t* out_rank;
    float* out_logit;          // nullable
};

// query qi's targets [tb, te), clamped to [0, n_tgt]
__device__ __forceinline__ bool target_range(const int64_t* tptr, int64_t qi, int64_t n_tgt, int64_t& tb, int64_t& te) {
    tb = tptr[qi];
    te = tptr[qi + 1];
    if (tb < 0) tb = 0;
    if (te > n_tgt) te = n_tgt;
    return tb < te;
}

// Target (u, v) of a relation whose row of rel_w is w (global or LDS): its key a*n+b, a < b, and the logit the tile loop
// gives candidate (a, b): x = z[a,k] * w[k] rounded once, acc = fmaf(x, z[b,k], acc), k ascending.  false: not ranked
// (an id outside [0, n), a self pair, a NaN logit).
__device__ __forceinline__ bool target_logit(const float* z, const float* w, int n, int dim, int u, int v, float& s, int& key) {
    s = NAN;
    key = WG_KEY_PAD;
    if (u < 0 || v < 0 || u >= n || v >= n || u == v) return false;
    const int a = u < v ? u : v, b = u < v ? v : u;
    const float* za = z + (int64_t)a * dim;
    const float* zb = z + (int64_t)b * dim;
    float acc = 0.f;
    for (int k0 = 0; k0 < dim; k0 += 4) {
        const float4 x = tipk_ld4(za + k0), y = tipk_ld4(zb + k0);
        acc = fmaf(__fmul_rn(x.x, w[k0]), y.x, acc);
        acc = fmaf(__fmul_rn(x.y, w[k0 + 1]), y.y, acc);
        acc = fmaf(__fmul_rn(x.z, w[k0 + 2]), y.z, acc);
        acc = fmaf(__fmul_rn(x.w, w[k0 + 3]), y.w, acc);
    }
    if (acc != acc) return false;
    s = acc;
    key = a * n + b;
    return true;
}

__global__ void __launch_bounds__(SR_NT) screen_rank_init_kernel(ScreenRankArgs a) {
    for (int64_t qi = blockIdx.x; qi < a.n_q; qi += gridDim.x) {
        int64_t tb, te;
        if (!target_range(a.tptr, qi, a.n_tgt, tb, te)) continue;
        const int r = a.qrel[qi];
        const bool act = r >= 0 && r < a.n_rel;
        const float* w = a.w + (int64_t)(act ? r : 0) * a.dim;
        for (int64_t i = tb + threadIdx.x; i < te; i += SR_NT) {
            float s = NAN;
            int key;
            const bool ok = act && target_logit(a.z, w, a.n, a.dim, a.tu[i], a.tv[i], s, key);
            a.out_rank[i] = ok ? 1 : 0;
            if (a.out_logit) a.out_logit[i] = s;
        }
    }
}

__global__ void __launch_bounds__(SR_NT) screen_rank_kernel(ScreenRankArgs a) {
    __shared__ float As[WG_KC * WG_LD];
    __shared__ float Zs[WG_KC * WG_LD];
    __shared__ float ts[SR_CHUNK];             // the chunk's targets, best first: logit, key, position in the chunk
    __shared__ int tk[SR_CHUNK];
    __shared__ int ti[SR_CHUNK];
    __shared__ unsigned hist[SR_CHUNK];        // hist[j]: candidates whose first beaten target is sorted position j
    __shared__ unsigned psum[SR_NT];
    __shared__ float wl[SR_DIM_MAX];
    __shared__ int n_ranked;
    extern __shared__ uint32_t bm[];           // bitmap route only

    const int t = threadIdx.x;
    const int64_t qi = blockIdx.x / a.splits;
    const int part = blockIdx.x % a.splits;
    const int n = a.n, dim = a.dim;
    const int r = a.qrel[qi];
    if (r < 0 || r >= a.n_rel) return;                         // the init kernel has written (0, NaN)
    int64_t tb, te;
    if (!target_range(a.tptr, qi, a.n_tgt, tb, te)) return;

    // this part's share of the tiles of the upper triangle
    const WgDeal deal0(n, part, a.splits);
    if (deal0.t0 >= deal0.t1) return;

    for (int i = t; i < dim; i += SR_NT) wl[i] = a.w[(int64_t)r * dim + i];
    WgKnown known;
    known.build<SR_NT>(bm, a.keys, a.kptr, r, n, a.bitmap);
    const int ty = t >> 4, tx = t & 15;

    for (int64_t ch = tb; ch < te; ch += SR_CHUNK) {
        const int cnt = te - ch < SR_CHUNK ? (int)(te - ch) : SR_CHUNK;
        int p = 2;
        while (p < cnt) p <<= 1;
        if (t == 0) n_ranked = 0;
        __syncthreads();                                       // w and the bitmap are in place; the previous chunk is done
        for (int i = t; i < SR_CHUNK; i += SR_NT) {
            hist[i] = 0u;
            if (i >= p) continue;
            float s = NAN;
            int key = WG_KEY_PAD;
            const bool ok = i < cnt && target_logit(a.z, wl, n, dim, a.tu[ch + i], a.tv[ch + i], s, key);
            ts[i] = ok ? s : -INFINITY;
            tk[i] = key;
            ti[i] = i;
            if (ok) atomicAdd(&n_ranked, 1);
        }
        __syncthreads();
        wg_bitonic<SR_NT, true>(ts, tk, ti, p);
        const int m = n_ranked;                                // ranked targets: sorted positions [0, m)
        __syncthreads();                                       // everyone has read it before the next chunk clears it
        if (m == 0) continue;
        const float weak_s = ts[m - 1];
        const int weak_k = tk[m - 1];

        WgDeal deal = deal0;
        for (int64_t tile = deal.t0; tile < deal.t1; ++tile) {
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
            wg_score_tile(As, Zs, a.z, wl, n, dim, deal.bu, deal.bv, acc);
            const int u0 = deal.bu * WG_TILE + 4 * ty, v0 = deal.bv * WG_TILE + 4 * tx;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int u = u0 + i, v = v0 + j;
                    if (!(u < v && v < n)) continue;
                    const float s = acc[i][j];
                    const int key = u * n + v;
                    if (!better(s, key, weak_s, weak_k)) continue;
                    if (known.known(u, v)) continue;
                    int lo = 0, hi = m - 1;                      // it beats position m - 1: the first beaten one is in [0, m)
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (better(s, key, ts[mid], tk[mid])) hi = mid; else lo = mid + 1;
                    }
                    atomicAdd(&hist[lo], 1u);
                }
            }
            deal.next();
        }
        __syncthreads();                                       // every bucket is final

        unsigned own = 0;
#pragma unroll
        for (int e = 0; e < SR_PER; ++e) own += hist[SR_PER * t + e];
        psum[t] = own;
        __syncthreads();
        for (int off = 1; off < SR_NT; off <<= 1) {
            const unsigned add = t >= off ? psum[t - off] : 0u;
            __syncthreads();
            psum[t] += add;
            __syncthreads();
        }
        unsigned run = psum[t] - own;
#pragma unroll
        for (int e = 0; e < SR_PER; ++e) {
            const int j = SR_PER * t + e;
            run += hist[j];
            if (j < m && run > 0u) atomicAdd(&a.out_rank[ch + ti[j]], (int)run);
        }
    }
}

}  // namespace

extern "C" int tipk_distmult_screen_rank_supported(int64_t n_nodes, int dim, int64_t n_rel) {
    return n_nodes >= 1 && n_nodes <= SR_NMAX && dim >= 4 && dim <= SR_DIM_MAX && dim % 4 == 0 && n_rel >= 1 &&
           n_rel <= SR_RMAX;
}

extern "C" int64_t tipk_distmult_screen_rank_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q, int64_t n_tgt) {
    if (n_q < 0 || n_tgt < 0 || !tipk_distmult_screen_rank_supported(n_nodes, dim, 1)) return -1;
    return 0;                                                  // the counts are summed in out_rank itself
}

extern "C" int tipk_distmult_screen_rank_chunk(void) { return SR_CHUNK; }

extern "C" int tipk_distmult_screen_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                         const int32_t* q_rel, int64_t n_q, const int64_t* tgt_ptr, const int32_t* tgt_u,
                                         const int32_t* tgt_v, int64_t n_tgt, const int64_t* known_keys,
                                         const int64_t* known_ptr, int32_t* out_rank, float* out_logit, void* workspace,
                                         tipk_stream_t stream) {
    if (n_q < 0 || n_tgt < 0 || n_nodes < 1 || n_rel < 1 || dim < 1) return TIPK_EINVAL;
    if ((known_keys == nullptr) != (known_ptr == nullptr)) return TIPK_EINVAL;
    if (n_q > 0 && n_tgt > 0 && (!z || !rel_w || !q_rel || !tgt_ptr || !tgt_u || !tgt_v || !out_rank)) return TIPK_EINVAL;
    (void)workspace;                                           // _workspace_bytes is 0: there is nothing to require
    if (!tipk_distmult_screen_rank_supported(n_nodes, dim, n_rel)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_tgt == 0) return TIPK_OK;

    ScreenRankArgs a;
    a.z = z; a.w = rel_w; a.qrel = q_rel; a.tptr = tgt_ptr; a.tu = tgt_u; a.tv = tgt_v;
    a.keys = known_keys; a.kptr = known_ptr;
    a.n_q = n_q; a.n_tgt = n_tgt;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel;
    a.splits = wg_splits(n_nodes, n_q);
    a.bitmap = known_keys && tipk_distmult_screen_bitmap_route(n_nodes);
    a.out_rank = out_rank; a.out_logit = out_logit;
    if (n_q * a.splits > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = a.bitmap ? (size_t)((n_nodes * n_nodes + 31) / 32 * 4) : 0;
    hipError_t e = hipFuncSetAttribute((const void*)screen_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    const unsigned init_grid = (unsigned)(n_q < 65536 ? n_q : 65536);
    hipLaunchKernelGGL(screen_rank_init_kernel, dim3(init_grid), dim3(SR_NT), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(screen_rank_kernel, dim3((unsigned)(n_q * a.splits)), dim3(SR_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}
