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
#include "tipk_common.h"
#include <math.h>
#include <vector>

namespace {

constexpr int SC_NT = 256;                 // threads per workgroup
constexpr int SC_TILE = 64;                // rows of the A and Z tiles of a relation query
constexpr int SC_KC = 32;                  // columns of z per staged chunk
constexpr int SC_LD = SC_TILE + 4;         // LDS row stride of the transposed tiles (floats; keeps float4 alignment)
constexpr int SC_DBLK = 256;               // candidates per block of a drug query (one per thread)
constexpr int SC_CAP = 2048;               // buffer entries (power of two >= k_max + one round)
constexpr int SC_ROUND = 1024;             // most appends of one round (relation: 256 threads x 4; drug: 256)
constexpr int SC_KMAX = 1024;
constexpr int SC_DIM_MAX = 256;
constexpr int64_t SC_NMAX = 46340;         // n^2 < 2^31: a key u*n+v is an int32
constexpr int SC_BITMAP_BYTES = 65536;     // LDS bitmap route: n^2 bits within this
constexpr int SC_MERGE_G = 8;              // part lists merged per merge workgroup
constexpr int SC_SPLIT_MAX = 64;
constexpr int SC_TARGET_WG = 4096;
constexpr int SC_KEY_PAD = 0x7fffffff;

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

__device__ __forceinline__ bool better(float sa, int ka, float sb, int kb) {
    return sa > sb || (sa == sb && ka < kb);
}

__device__ __forceinline__ bool key_in(const int64_t* keys, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t v = keys[mid];
        if (v == x) return true;
        if (v < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

struct Sel {
    float* bs;
    int* bk;
    unsigned* ctr;             // [3] rotating append counters (one barrier per round)
    const uint32_t* bm;        // LDS bitmap or nullptr
    const int64_t* keys;
    int64_t klo, khi;
    int n, k;
    int c;                     // entries in the buffer (uniform)
    int rr;                    // round number (uniform)
    float thr;

    // every lane calls this (uniform control flow): append (s, u*n+v) when ok, not below the threshold, not known
    __device__ __forceinline__ void offer(bool ok, float s, int u, int v) {
        bool pass = ok && s >= thr;
        if (pass) {
            if (bm) {
                const uint32_t b = (uint32_t)(u * n + v);
                pass = !((bm[b >> 5] >> (b & 31)) & 1u);
            } else if (keys) {
                pass = !key_in(keys, klo, khi, (int64_t)u * n + v) && !key_in(keys, klo, khi, (int64_t)v * n + u);
            }
        }
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
            bk[pos] = u * n + v;
        }
    }

    // sort the c entries best first and keep k of them (every thread, uniform)
    __device__ void flush() {
        const int t = threadIdx.x;
        int p = 2;
        while (p < c) p <<= 1;
        for (int i = c + t; i < p; i += SC_NT) { bs[i] = -INFINITY; bk[i] = SC_KEY_PAD; }
        __syncthreads();
        for (int size = 2; size <= p; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int x = t; x < (p >> 1); x += SC_NT) {
                    const int i = 2 * stride * (x / stride) + (x % stride), j = i + stride;
                    const float si = bs[i], sj = bs[j];
                    const int ki = bk[i], kj = bk[j];
                    const bool up = (i & size) == 0;
                    if (up ? better(sj, kj, si, ki) : better(si, ki, sj, kj)) {
                        bs[i] = sj; bk[i] = kj; bs[j] = si; bk[j] = ki;
                    }
                }
                __syncthreads();
            }
        }
        c = c < k ? c : k;
        thr = c == k ? bs[k - 1] : -INFINITY;
    }

    // end of a round: everything appended is visible; c moves on; the counter of round rr - 1 is cleared for rr + 2
    __device__ __forceinline__ void end_round() {
        __syncthreads();
        c += (int)ctr[rr % 3];
        if (threadIdx.x == 0) ctr[(rr + 2) % 3] = 0u;
        ++rr;
        if (c > SC_CAP - SC_ROUND) flush();
    }
};

__global__ void __launch_bounds__(SC_NT) screen_kernel(ScreenArgs a) {
    __shared__ float As[SC_KC * SC_LD];
    __shared__ float Zs[SC_KC * SC_LD];
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
    sel.bs = bs; sel.bk = bk; sel.ctr = ctr; sel.bm = nullptr; sel.keys = nullptr; sel.klo = sel.khi = 0;
    sel.n = n; sel.k = a.k; sel.c = 0; sel.rr = 0; sel.thr = -INFINITY;

    if (t < 3) ctr[t] = 0u;
    for (int i = t; i < dim; i += SC_NT) {
        const float wv = a.w[(int64_t)r * dim + i];
        wl[i] = wv;
        if (du >= 0) al[i] = a.z[(int64_t)du * dim + i] * wv;
    }
    if (a.keys) {
        sel.klo = a.kptr[r];
        sel.khi = a.kptr[r + 1];
        if (a.bitmap) {
            const int words = (int)(((int64_t)n * n + 31) / 32);
            for (int i = t; i < words; i += SC_NT) bm[i] = 0u;
            __syncthreads();                                   // cleared before any bit is set
            const int64_t nn = (int64_t)n * n;
            for (int64_t e = sel.klo + t; e < sel.khi; e += SC_NT) {
                const int64_t key = a.keys[e];
                if (key < 0 || key >= nn) continue;
                const int x = (int)(key / n), y = (int)(key % n);
                const uint32_t b0 = (uint32_t)(x * n + y), b1 = (uint32_t)(y * n + x);
                atomicOr(&bm[b0 >> 5], 1u << (b0 & 31));
                atomicOr(&bm[b1 >> 5], 1u << (b1 & 31));
            }
            sel.bm = bm;
        } else {
            sel.keys = a.keys;
        }
    }
    __syncthreads();                                           // counters, w, a and the bitmap are in place

    if (du < 0) {
        // relation query: tiles (bu <= bv) of the upper triangle in row-major order, this part's share of them
        const int nb = (n + SC_TILE - 1) / SC_TILE;
        const int64_t n_tiles = (int64_t)nb * (nb + 1) / 2;
        const int64_t t0 = n_tiles * part / a.splits, t1 = n_tiles * (part + 1) / a.splits;
        int bu = 0;
        int64_t row_start = 0;                                  // linear index of tile (bu, bu)
        while (t0 < t1 && t0 >= row_start + (nb - bu)) { row_start += nb - bu; ++bu; }
        int bv = bu + (int)(t0 - row_start);
        const int ty = t >> 4, tx = t & 15;
        for (int64_t tile = t0; tile < t1; ++tile) {
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
            for (int k0 = 0; k0 < dim; k0 += SC_KC) {
                const int kc = dim - k0 < SC_KC ? dim - k0 : SC_KC;
                __syncthreads();                                 // the previous chunk has been read
                for (int idx = t; idx < 2 * SC_TILE * (SC_KC / 4); idx += SC_NT) {
                    const int which = idx / (SC_TILE * (SC_KC / 4));
                    const int rem = idx % (SC_TILE * (SC_KC / 4));
                    const int row = rem >> 3, qd = rem & 7;
                    if (4 * qd >= kc) continue;
                    const int node = (which == 0 ? bu : bv) * SC_TILE + row;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (node < n) v = tipk_ld4(a.z + (int64_t)node * dim + k0 + 4 * qd);
                    float* dst = which == 0 ? As : Zs;
                    if (which == 0) {
                        const int kk = k0 + 4 * qd;
                        v.x *= wl[kk]; v.y *= wl[kk + 1]; v.z *= wl[kk + 2]; v.w *= wl[kk + 3];
                    }
                    dst[(4 * qd + 0) * SC_LD + row] = v.x;
                    dst[(4 * qd + 1) * SC_LD + row] = v.y;
                    dst[(4 * qd + 2) * SC_LD + row] = v.z;
                    dst[(4 * qd + 3) * SC_LD + row] = v.w;
                }
                __syncthreads();
                for (int kk = 0; kk < kc; ++kk) {
                    const float4 av = *reinterpret_cast<const float4*>(&As[kk * SC_LD + 4 * ty]);
                    const float4 zv = *reinterpret_cast<const float4*>(&Zs[kk * SC_LD + 4 * tx]);
                    const float ar[4] = {av.x, av.y, av.z, av.w}, zr[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], zr[j], acc[i][j]);
                }
            }
            const int u0 = bu * SC_TILE + 4 * ty, v0 = bv * SC_TILE + 4 * tx;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int u = u0 + i, v = v0 + j;
                    sel.offer(u < v && v < n, acc[i][j], u, v);
                }
                sel.end_round();
            }
            if (++bv == nb) { ++bu; bv = bu; }
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
            sel.offer(v < n && v != du, acc, du, v);
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

int64_t screen_tiles(int64_t n) {
    const int64_t nb = (n + SC_TILE - 1) / SC_TILE;
    return nb * (nb + 1) / 2;
}

// parts per query: enough workgroups to fill the chip for few queries, one part per query for thousands of them
int screen_splits(int64_t n, int64_t n_q) {
    int64_t s = n_q > 0 ? SC_TARGET_WG / n_q : 1;
    if (s < 1) s = 1;
    if (s > SC_SPLIT_MAX) s = SC_SPLIT_MAX;
    const int64_t tiles = screen_tiles(n);
    if (s > tiles) s = tiles;
    return (int)s;
}

int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
    int splits, splits2;
    int64_t q_off, a_s, a_k, b_s, b_k, total;
};

Layout screen_layout(int64_t n, int64_t n_q, int k) {
    Layout L;
    L.splits = screen_splits(n, n_q);
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
