// DistMult screen: the k best unseen candidates of a query (include/tipk.h section 4c).
//
// One launch scores every candidate of a query split into S parts (S from the query count: a relation query's upper
// triangle of 64 x 64 tiles, a drug query's 256-node blocks) and keeps each part's k best in LDS; a merge launch (two
// when S > 8) combines the sorted part lists by rank into the exact order of the contract.
//
// Scoring (screen_kernel, 256 threads): a relation tile stages A = z[u-rows] * w[r] and Z = z[v-rows] transposed in LDS
// in chunks of 32 columns; a thread owns a 4 x 4 block of (u, v) and accumulates fmaf(A[u][k], Z[v][k], acc) with k
// ascending.  A drug block keeps a = z[u] * w[r] in LDS and a thread sums fmaf(a[k], z[v][k], acc) over its own row of z,
// k ascending: the same two roundings per term in the same order, so a pair's logit is one number on every route.
// Selection: a candidate enters the workgroup's LDS buffer only when it is not below the running threshold (the k-th best
// kept so far); only then is the known-pair filter consulted (LDS bitmap of the relation, or binary search in its sorted
// keys).  When the buffer could overflow in the next round it is sorted (bitonic) and cut to k, which raises the
// threshold.  Dropping a candidate below the threshold is exact: k kept entries are better than it.  The result is a set
// defined by the total order (logit desc, key asc), so it does not depend on the order of the appends.
// The tile deal and scorer, the known-pair filter, the selection and its bitonic network are the shared pieces of
// tipk_wg_topk.h; this file holds the query loop over tiles and drug blocks, the merge kernel and the workspace layout.
#include "tipk_wg_topk.h"
#include <vector>

namespace {

constexpr int SC_NT = WG_NT;               // threads per workgroup
constexpr int SC_DBLK = 256;               // candidates per block of a drug query (one per thread)
constexpr int SC_CAP = 2048;               // buffer entries (power of two >= k_max + one round)
constexpr int SC_ROUND = 1024;             // most appends of one round (relation: 256 threads x 4; drug: 256)
constexpr int SC_KMAX = 1024;
constexpr int SC_DIM_MAX = 256;
constexpr int64_t SC_NMAX = 46340;         // n^2 < 2^31: a key u*n+v is an int32
constexpr int SC_BITMAP_BYTES = 65536;     // LDS bitmap route: n^2 bits within this
constexpr int SC_MERGE_G = 8;              // part lists merged per merge workgroup

struct ScreenArgs {
    const float* z;
    const float* w;
    const int32_t* q;          // [n_q][2] (relation, drug | -1), device copy
    const int64_t* keys;       // nullable
    const int64_t* kptr;       // [n_rel + 1], nullable with keys
    int n, dim, k, splits, bitmap;
    float* part_s;             // [n_q * splits][k]
    int32_t* part_k;
};

using Sel = WgSel<SC_NT, SC_CAP, SC_ROUND>;

// every lane calls this (uniform control flow): append (s, u*n+v) when ok, not below the threshold, not known -- the filter
// is consulted only for a candidate that passed the threshold
__device__ __forceinline__ void offer(Sel& sel, const WgKnown& known, bool ok, float s, int u, int v) {
    bool pass = sel.wants(ok, s);
    if (pass) pass = !known.known(u, v);
    sel.append(pass, s, u * known.n + v);
}

__global__ void __launch_bounds__(SC_NT) screen_kernel(ScreenArgs a) {
    __shared__ float As[WG_KC * WG_LD];
    __shared__ float Zs[WG_KC * WG_LD];
    __shared__ float bs[SC_CAP];
    __shared__ int bk[SC_CAP];
    __shared__ float wl[SC_DIM_MAX];
    __shared__ float al[SC_DIM_MAX];
    __shared__ unsigned ctr[3];
    extern __shared__ uint32_t bm[];           // bitmap route only

    const int t = threadIdx.x;
    const int qi = blockIdx.x / a.splits, part = blockIdx.x % a.splits;
    const int r = a.q[2 * qi], du = a.q[2 * qi + 1];
    const int n = a.n, dim = a.dim;

    Sel sel;
    sel.init(bs, bk, ctr, a.k);
    WgKnown known;

    if (t < 3) ctr[t] = 0u;
    for (int i = t; i < dim; i += SC_NT) {
        const float wv = a.w[(int64_t)r * dim + i];
        wl[i] = wv;
        if (du >= 0) al[i] = a.z[(int64_t)du * dim + i] * wv;
    }
    known.build<SC_NT>(bm, a.keys, a.kptr, r, n, a.bitmap);
    __syncthreads();                                           // counters, w, a and the bitmap are in place

    if (du < 0) {
        // relation query: this part's share of the tiles of the upper triangle
        WgDeal deal(n, part, a.splits);
        const int ty = t >> 4, tx = t & 15;
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
                    offer(sel, known, u < v && v < n, acc[i][j], u, v);
                }
                sel.end_round();
            }
            deal.next();
        }
    } else {
        // drug query (r, du): blocks of 256 partners v != du
        const int nvb = (n + SC_DBLK - 1) / SC_DBLK;
        const int b0 = (int)((int64_t)nvb * part / a.splits), b1 = (int)((int64_t)nvb * (part + 1) / a.splits);
        for (int blk = b0; blk < b1; ++blk) {
            const int v = blk * SC_DBLK + t;
            float acc = 0.f;
            if (v < n) {
                const float* zv = a.z + (int64_t)v * dim;
                for (int k0 = 0; k0 < dim; k0 += 4) {
                    const float4 x = tipk_ld4(zv + k0);
                    acc = fmaf(al[k0], x.x, acc);
                    acc = fmaf(al[k0 + 1], x.y, acc);
                    acc = fmaf(al[k0 + 2], x.z, acc);
                    acc = fmaf(al[k0 + 3], x.w, acc);
                }
            }
            offer(sel, known, v < n && v != du, acc, du, v);
            sel.end_round();
        }
    }

    sel.flush();
    __syncthreads();
    float* ps = a.part_s + (int64_t)blockIdx.x * a.k;
    int32_t* pk = a.part_k + (int64_t)blockIdx.x * a.k;
    for (int i = t; i < a.k; i += SC_NT) {
        const bool have = i < sel.c;
        ps[i] = have ? bs[i] : -INFINITY;
        pk[i] = have ? bk[i] : -1;
    }
}

// Merge of up to SC_MERGE_G sorted part lists per workgroup: an entry's rank is its index in its own list plus the number of
// entries of the other lists that are better (binary search); ranks below k are written, the rest of the k slots padded.
// Keys are unique across the parts of a query (disjoint candidate sets), so the ranks are distinct.
__global__ void __launch_bounds__(SC_NT) screen_merge_kernel(const float* in_s, const int32_t* in_k, int s_in, int s_out,
                                                             int k, int n, float* out_s, int32_t* out_k,
                                                             float* fin_s, int32_t* fin_u, int32_t* fin_v) {
    __shared__ int nval[SC_MERGE_G];
    const int t = threadIdx.x;
    const int qi = blockIdx.x / s_out, g = blockIdx.x % s_out;
    const int l0 = g * SC_MERGE_G;
    const int m = (s_in - l0) < SC_MERGE_G ? (s_in - l0) : SC_MERGE_G;
    const float* ls = in_s + ((int64_t)qi * s_in + l0) * k;
    const int32_t* lk = in_k + ((int64_t)qi * s_in + l0) * k;
    if (t < m) {                                               // valid entries form a prefix of each list
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (lk[(int64_t)t * k + mid] >= 0) lo = mid + 1; else hi = mid;
        }
        nval[t] = lo;
    }
    __syncthreads();
    int total = 0;
    for (int s = 0; s < m; ++s) total += nval[s];
    const int64_t o = (int64_t)blockIdx.x * k;
    for (int e = t; e < m * k; e += SC_NT) {
        const int s = e / k, j = e % k;
        if (j >= nval[s]) continue;
        const float xs = ls[(int64_t)s * k + j];
        const int xk = lk[(int64_t)s * k + j];
        int rank = j;
        for (int s2 = 0; s2 < m && rank < k; ++s2) {
            if (s2 == s) continue;
            int lo = 0, hi = nval[s2];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (better(ls[(int64_t)s2 * k + mid], lk[(int64_t)s2 * k + mid], xs, xk)) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank >= k) continue;
        if (fin_s) {
            fin_s[o + rank] = xs;
            fin_u[o + rank] = xk / n;
            fin_v[o + rank] = xk % n;
        } else {
            out_s[o + rank] = xs;
            out_k[o + rank] = xk;
        }
    }
    for (int p = (total < k ? total : k) + t; p < k; p += SC_NT) {
        if (fin_s) { fin_s[o + p] = -INFINITY; fin_u[o + p] = -1; fin_v[o + p] = -1; }
        else { out_s[o + p] = -INFINITY; out_k[o + p] = -1; }
    }
}

int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
    int splits, splits2;
    int64_t q_off, a_s, a_k, b_s, b_k, total;
};

Layout screen_layout(int64_t n, int64_t n_q, int k) {
    Layout L;
    L.splits = wg_splits(n, n_q);
    L.splits2 = L.splits > SC_MERGE_G ? (L.splits + SC_MERGE_G - 1) / SC_MERGE_G : 0;
    L.q_off = 0;
    int64_t off = align256(n_q * 8);
    const int64_t la = n_q * L.splits * (int64_t)k * 4, lb = n_q * L.splits2 * (int64_t)k * 4;
    L.a_s = off; off += align256(la);
    L.a_k = off; off += align256(la);
    L.b_s = off; off += align256(lb);
    L.b_k = off; off += align256(lb);
    L.total = off;
    return L;
}

}  // namespace

extern "C" int tipk_distmult_screen_supported(int64_t n_nodes, int dim, int k) {
    return n_nodes >= 1 && n_nodes <= SC_NMAX && dim >= 4 && dim <= SC_DIM_MAX && dim % 4 == 0 && k >= 1 &&
           k <= SC_KMAX;
}

extern "C" int64_t tipk_distmult_screen_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q, int k) {
    if (n_q < 0 || !tipk_distmult_screen_supported(n_nodes, dim, k)) return -1;
    return screen_layout(n_nodes, n_q, k).total;
}

extern "C" int tipk_distmult_screen_bitmap_route(int64_t n_nodes) {
    return n_nodes >= 1 && n_nodes <= SC_NMAX && (n_nodes * n_nodes + 31) / 32 * 4 <= SC_BITMAP_BYTES &&
           !tipk_option(TIPK_OPT_SCREEN_SEARCH);
}

extern "C" int tipk_distmult_screen(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                    const int32_t* queries, int64_t n_q, const int64_t* known_keys,
                                    const int64_t* known_ptr, int k, float* out_score, int32_t* out_u, int32_t* out_v,
                                    void* workspace, tipk_stream_t stream) {
    if (k <= 0 || n_q < 0 || n_nodes < 1 || n_rel < 1 || dim <= 0) return TIPK_EINVAL;
    if ((known_keys == nullptr) != (known_ptr == nullptr)) return TIPK_EINVAL;
    if (n_q > 0 && (!queries || !z || !rel_w || !out_score || !out_u || !out_v || !workspace)) return TIPK_EINVAL;
    for (int64_t i = 0; i < n_q; ++i) {                       // host array: checked before anything is launched
        const int32_t r = queries[2 * i], u = queries[2 * i + 1];
        if (r < 0 || r >= n_rel || u < -1 || u >= n_nodes) return TIPK_EINVAL;
    }
    if (!tipk_distmult_screen_supported(n_nodes, dim, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
        return TIPK_EUNSUPPORTED;
    if (n_q == 0) return TIPK_OK;
    const Layout L = screen_layout(n_nodes, n_q, k);
    if (n_q * L.splits > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* q_dev = (int32_t*)(ws + L.q_off);
    // the query list is host memory that the caller may reuse on return: copy, then wait for the copy
    hipError_t e = hipMemcpyAsync(q_dev, queries, (size_t)n_q * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return tipk_hip_status(e);

    ScreenArgs a;
    a.z = z; a.w = rel_w; a.q = q_dev; a.keys = known_keys; a.kptr = known_ptr;
    a.n = (int)n_nodes; a.dim = dim; a.k = k; a.splits = L.splits;
    a.bitmap = known_keys && tipk_distmult_screen_bitmap_route(n_nodes);
    a.part_s = (float*)(ws + L.a_s); a.part_k = (int32_t*)(ws + L.a_k);
    const size_t lds = a.bitmap ? (size_t)((n_nodes * n_nodes + 31) / 32 * 4) : 0;
    e = hipFuncSetAttribute((const void*)screen_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(screen_kernel, dim3((unsigned)(n_q * L.splits)), dim3(SC_NT), lds, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    const float* in_s = a.part_s;
    const int32_t* in_k = a.part_k;
    int s_in = L.splits;
    if (L.splits2 > 0) {
        float* bs = (float*)(ws + L.b_s);
        int32_t* bk = (int32_t*)(ws + L.b_k);
        hipLaunchKernelGGL(screen_merge_kernel, dim3((unsigned)(n_q * L.splits2)), dim3(SC_NT), 0, st, in_s, in_k, s_in,
                           L.splits2, k, (int)n_nodes, bs, bk, nullptr, nullptr, nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) return tipk_hip_status(e);
        in_s = bs; in_k = bk; s_in = L.splits2;
    }
    hipLaunchKernelGGL(screen_merge_kernel, dim3((unsigned)n_q), dim3(SC_NT), 0, st, in_s, in_k, s_in, 1, k,
                       (int)n_nodes, nullptr, nullptr, out_score, out_u, out_v);
    TIPK_RETURN_LAUNCH();
}
