// Add-on burden: the expected weighted number of side effects a candidate drug adds to a patient's drug list, for every
// (query, candidate) task, and the k candidates of every query with the lowest burden (include/tipk.h section 4i).  The
// logit, the known bitmap, the softplus and the bitonic cut are the shared pieces of tipk_wave_topk.h; this file holds the
// task / window / context loop, the reduction over relations and the per-query selection.
//
// Launch 1, addon_burden_kernel: persistent workgroups (16 wavefronts) take blocks of 16 tasks, ONE WAVEFRONT PER TASK.
//   Lane l keeps the l-th context drug of the task's query (a context has at most 64 entries) and, with a known list, the
//   position of the pair (candidate, that drug) in the known keys, found once per task.
//   Windows.  The relation axis is walked in windows of 64 x AB_A relations: lane l owns relations c0 + l, c0 + l + 64, ...
//   with AB_A aggregate registers.  Per window the wave loops over the context drugs in list order; per drug it scores its
//   AB_A relations (h = z[c] * z[s] rounded once into the wave's LDS row, then the shared fma chain; table variant: one
//   add of two coalesced table rows) and updates the registers unless the triple is known.  A NaN logit of a triple that
//   is not known marks the task.  After the last drug the lane turns each aggregate into P_r and adds w_r * P_r to ITS
//   partial burden: a lane's partial runs over r = l, l + 64, l + 128, ... ascending.
//   Reduction.  The 64 partials are summed by the halving tree p_l += p_(l + off), off = 32, 16, ..., 1; lane 0 writes.
// rel_w.  An LDS image, staged once per workgroup, when it fits beside the waves' state; otherwise (or under option
//   "addon_global") each lane reads its rows from global memory.  Same arithmetic, same bits.
// Launch 2 (k > 0), addon_select_kernel: ONE WAVEFRONT PER QUERY streams the query's row of out_burden in windows of 64 and
//   keeps the k best of (-burden descending, position ascending) with the shared buffer cut; NaN never enters.
#include "tipk_wave_topk.h"

namespace {

constexpr int AB_M_MAX = TIPK_WAVE;         // context drugs per query: one lane each
constexpr int AB_A = 4;                     // relations per lane and window
constexpr int AB_WIN = TIPK_WAVE * AB_A;    // relations per window
constexpr int64_t AB_CAND_MAX = 0x7fffffff; // candidate entries of a call: positions are int32

struct AddonArgs {
    const float* a;            // z [n x dim]            | s1 [n x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2 [n x ld]
    const int32_t* ctx;
    const int64_t* cptr;
    const int32_t* cand;
    const int64_t* dptr;       // nullable: one candidate list shared by all queries
    const float* wts;          // nullable: every weight is 1
    const int64_t* kkeys;      // nullable with kptr, krel
    const int64_t* kptr;
    const int32_t* krel;
    int64_t n_known, n_q, n_cand, n_tasks, ld;
    int n, dim, n_rel, k, stride, noisy;
    float* out_b;
    float* best_b;
    int32_t* best_p;
};

// the query that owns entry `task` of the CSR candidate lists: the largest q in [0, n_q) with dptr[q] <= task, or -1 when
// that q does not hold it (device lists cannot be validated on the host; every read is inside dptr[0 .. n_q])
__device__ __forceinline__ int64_t ab_owner(const int64_t* dptr, int64_t n_q, int64_t task) {
    int64_t lo = 0, hi = n_q;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (dptr[mid] <= task) lo = mid; else hi = mid;
    }
    return dptr[lo] <= task && task < dptr[lo + 1] ? lo : -1;
}

__device__ __forceinline__ float ab_sigma(float s) { return 1.0f / (1.0f + expf(-s)); }

template <int MODE, bool IMAGE>
__global__ void __launch_bounds__(WT_NT) addon_burden_kernel(AddonArgs a) {
    extern __shared__ __align__(16) unsigned char ab_smem[];
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
    const int R = a.n_rel, dim = a.dim;
    const int gdim = MODE == WT_DISTMULT16 ? 16 : dim;                // row stride of rel_w in global memory: a shift for dim 16

    // LDS: [rel_w image] [h rows] | bitmaps
    float* Ws = reinterpret_cast<float*>(ab_smem);
    float* hs_all = Ws + (IMAGE ? R * a.stride : 0);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(hs_all + (MODE == WT_TABLE ? 0 : WT_NW * dim));
    float* hs = hs_all + wave * dim;
    uint32_t* km = km_all + wave * (AB_WIN / 32);

    if (IMAGE) {
        wt_stage_rows<WT_NT>(Ws, a.b, 0, R, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_tasks + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t task = blk * WT_NW + wave;
        if (task >= a.n_tasks) continue;                               // (the waves of a workgroup never meet in this loop)
        int64_t q;
        int c;
        if (a.dptr) {
            q = ab_owner(a.dptr, a.n_q, task);
            c = a.cand[task];
        } else {
            q = task / a.n_cand;
            c = a.cand[task - q * a.n_cand];
        }
        bool act = q >= 0 && c >= 0 && c < a.n;                        // uniform in the wave
        int64_t p0 = 0, m64 = 0;
        if (act) {
            p0 = a.cptr[q];
            m64 = a.cptr[q + 1] - p0;
            act = m64 >= 1 && m64 <= AB_M_MAX;
        }
        const int m = act ? (int)m64 : 0;
        int dl = 0;
        if (act) {
            if (lane < m) dl = a.ctx[p0 + lane];
            act = __ballot(lane < m && (dl < 0 || dl >= a.n || dl == c)) == 0ull;
        }
        float part = 0.f;                                              // this lane's share of the burden
        bool bad = false;                                              // a NaN logit of a triple that is not known
        int at_l = -1;                                                 // known block of the pair (c, this lane's drug)

        for (int c0 = 0; act && c0 < R; c0 += AB_WIN) {
            const int c1 = c0 + AB_WIN < R ? c0 + AB_WIN : R;
            float agg[AB_A];                                           // noisy-or: sum softplus; max: the largest logit
#pragma unroll
            for (int x = 0; x < AB_A; ++x) agg[x] = a.noisy ? 0.f : -INFINITY;

            for (int i = 0; i < m; ++i) {
                const int s = __shfl(dl, i);
                float4 hq[MODE == WT_DISTMULT16 ? 4 : 1];
                wave_sync();                                           // the previous drug is done with hs and km
                if (MODE != WT_TABLE) wt_write_row(hs, a.a + (int64_t)c * dim, a.a + (int64_t)s * dim, dim, lane);
                bool filt = false;
                if (a.kkeys) {
                    int at;
                    if (c0 == 0) {
                        const int lo = c < s ? c : s, hi = c < s ? s : c;
                        at = (int)find_key(a.kkeys, a.n_known, (int64_t)lo * a.n + hi, lane);
                        if (lane == i) at_l = at;
                    } else {
                        at = __shfl(at_l, i);
                    }
                    if (at >= 0) {
                        int64_t kc = a.kptr[at];
                        const int64_t kend = a.kptr[at + 1];
                        if (c0 > 0) kc = wt_lower_bound(a.krel, kc, kend, c0, lane);
                        const int first = kc < kend ? a.krel[kc] : WT_REL_PAD;
                        if (first < c1) {
                            // no fence in front of the clear: the one at the top of the drug loop serves
                            filt = true;
                            wt_merge_window<AB_WIN / 32>(km, kc, kend, c0, c1, lane,
                                                         [&](int64_t idx) { return a.krel[idx]; });
                        }
                    }
                }
                wave_sync();
                wt_row16<MODE>(hq, hs);
                const int u = c < s ? c : s, v = c < s ? s : c;        // table variant: the smaller id is the first argument
#pragma unroll
                for (int x = 0; x < AB_A; ++x) {
                    const int r = c0 + x * TIPK_WAVE + lane;
                    if (c0 + x * TIPK_WAVE >= c1) break;               // uniform
                    if (r >= c1) continue;
                    float sc = 0.f;
                    if (MODE == WT_TABLE) sc = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                    else sc = wt_dot<MODE>(IMAGE ? Ws + r * a.stride : a.b + (int64_t)r * gdim, hs, hq, dim);
                    if (filt && wt_bit(km, r - c0)) continue;          // known: contributes nothing, NaN or not
                    if (sc != sc) { bad = true; continue; }
                    if (a.noisy) agg[x] += wt_softplus(sc);
                    else agg[x] = sc > agg[x] ? sc : agg[x];
                }
            }

            // the window's relations, ascending per lane: P_r, then part = fmaf(w_r, P_r, part)
#pragma unroll
            for (int x = 0; x < AB_A; ++x) {
                const int r = c0 + x * TIPK_WAVE + lane;
                if (r >= c1) break;
                const float p = a.noisy ? -expm1f(-agg[x]) : ab_sigma(agg[x]);
                part = fmaf(a.wts ? a.wts[r] : 1.0f, p, part);
            }
        }

        const bool nan = __ballot(bad) != 0ull;
#pragma unroll
        for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) part += __shfl_down(part, off);
        if (lane == 0) a.out_b[task] = act && !nan ? part : NAN;
    }
}

__global__ void __launch_bounds__(WT_NT) addon_select_kernel(AddonArgs a) {
    extern __shared__ __align__(16) unsigned char ab_smem[];
    const int lane = tipk_lane(), wave = threadIdx.x >> 6;
    const int k = a.k;
    const int flush_at = wt_flush_at(k);
    float* bs = reinterpret_cast<float*>(ab_smem) + wave * WT_CAP;
    int* br = reinterpret_cast<int*>(reinterpret_cast<float*>(ab_smem) + WT_NW * WT_CAP) + wave * WT_CAP;

    const int64_t n_blocks = (a.n_q + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t q = blk * WT_NW + wave;
        if (q >= a.n_q) continue;                                      // (the waves of a workgroup never meet in this loop)
        int64_t b0, b1;                                                // the query's entries of out_burden, cut to [0, n_tasks)
        if (a.dptr) {
            b0 = a.dptr[q];
            b1 = a.dptr[q + 1];
            b0 = b0 < 0 ? 0 : b0;
            b1 = b1 > a.n_tasks ? a.n_tasks : b1;
        } else {
            b0 = q * a.n_cand;
            b1 = b0 + a.n_cand;
        }
        int c = 0;
        float thr = -INFINITY;
        wave_sync();                                                   // the previous query's buffer has been written out
        for (int64_t w0 = b0; w0 < b1; w0 += TIPK_WAVE) {
            const int64_t idx = w0 + lane;
            const float v = idx < b1 ? a.out_b[idx] : NAN;
            const float sv = -v;                                       // lowest burden first under `better`
            const bool pass = v == v && sv >= thr;                     // NaN is never selected
            const unsigned long long mask = __ballot(pass);
            if (mask == 0ull) continue;
            if (pass) {
                const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                bs[pos] = sv;
                br[pos] = (int)(idx - b0);
            }
            c += __popcll(mask);
            if (c >= flush_at) flush<false>(bs, br, nullptr, c, thr, k, lane);
        }
        if (c > 0) flush<false>(bs, br, nullptr, c, thr, k, lane);
        float* ob = a.best_b + q * k;
        int32_t* op = a.best_p + q * k;
        for (int i = lane; i < k; i += TIPK_WAVE) {
            const bool have = i < c;
            ob[i] = have ? -bs[i] : INFINITY;
            op[i] = have ? br[i] : -1;
        }
    }
}

int64_t ab_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * dim * 4) + (int64_t)WT_NW * (AB_WIN / 32) * 4;
}

int ab_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* ctx_drugs, const int64_t* ctx_ptr, int64_t n_q,
                   const int32_t* cand, int64_t n_cand, const int64_t* keys, const int64_t* kptr, const int32_t* krel,
                   int64_t n_known, int aggregate, int k, const float* out_burden, const float* out_best_burden,
                   const int32_t* out_best_pos) {
    if (k < 0 || n_q < 0 || n_cand < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    if (aggregate != TIPK_REGIMEN_MAX && aggregate != TIPK_REGIMEN_NOISY_OR) return TIPK_EINVAL;
    if (!wt_known_ok(keys, kptr, krel)) return TIPK_EINVAL;
    if (n_q > 0 && n_cand > 0) {
        if (!ctx_drugs || !ctx_ptr || !cand || !out_burden) return TIPK_EINVAL;
        if (k > 0 && (!out_best_burden || !out_best_pos)) return TIPK_EINVAL;
    }
    return TIPK_OK;
}

// cand_ptr given: n_cand entries in all; NULL: n_cand entries per query
bool ab_counts_ok(const int64_t* cand_ptr, int64_t n_q, int64_t n_cand) {
    if (n_cand > AB_CAND_MAX) return false;
    return cand_ptr || n_q == 0 || n_cand <= INT64_MAX / n_q;
}

void ab_fill_lists(AddonArgs& a, int64_t n_nodes, int64_t n_rel, const int32_t* ctx_drugs, const int64_t* ctx_ptr,
                   int64_t n_q, const int32_t* cand, const int64_t* cand_ptr, int64_t n_cand, const float* weights,
                   const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int aggregate, int k,
                   float* out_burden, float* out_best_burden, int32_t* out_best_pos) {
    a.ctx = ctx_drugs; a.cptr = ctx_ptr; a.cand = cand; a.dptr = cand_ptr; a.wts = weights;
    a.kkeys = n_known > 0 ? keys : nullptr; a.kptr = kptr; a.krel = krel;
    a.n_known = n_known; a.n_q = n_q; a.n_cand = n_cand;
    a.n_tasks = cand_ptr ? n_cand : n_q * n_cand;
    a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.k = k;
    a.noisy = aggregate == TIPK_REGIMEN_NOISY_OR;
    a.out_b = out_burden; a.best_b = out_best_burden; a.best_p = out_best_pos;
}

// launch 2 on the same stream, after launch 1 returned `status`
int ab_select(const AddonArgs& a, int status, hipStream_t st) {
    if (status != TIPK_OK || a.k == 0) return status;
    return wt_launch<addon_select_kernel>(a, wt_grid(a.n_q, 2), (size_t)WT_NW * WT_CAP * 8, st);
}

}  // namespace

extern "C" int tipk_addon_max_context(void) { return AB_M_MAX; }

extern "C" int tipk_distmult_addon_burden_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return wt_distmult_shape(n_nodes, dim, n_rel) && k >= 0 && k <= WT_KMAX;
}

extern "C" int64_t tipk_distmult_addon_burden_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_q,
                                                              int64_t n_cand, int k) {
    if (n_q < 0 || n_cand < 0 || !tipk_distmult_addon_burden_supported(n_nodes, dim, n_rel, k)) return -1;
    return 0;                                                          // the burdens themselves are the only intermediate
}

extern "C" int tipk_distmult_addon_burden_lds_route(int dim, int64_t n_rel) {
    return wt_distmult_shape(1, dim, n_rel) && wt_fits_lds(n_rel, dim, ab_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_ADDON_GLOBAL);
}

extern "C" int tipk_distmult_addon_burden(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                          const int32_t* ctx_drugs, const int64_t* ctx_ptr, int64_t n_q,
                                          const int32_t* cand, const int64_t* cand_ptr, int64_t n_cand,
                                          const float* weights, const int64_t* known_pair_keys,
                                          const int64_t* known_pair_ptr, const int32_t* known_rel, int64_t n_known_pairs,
                                          int aggregate, int k, float* out_burden, float* out_best_burden,
                                          int32_t* out_best_pos, void* workspace, tipk_stream_t stream) {
    (void)workspace;
    const int bad = ab_check_lists(n_nodes, n_rel, ctx_drugs, ctx_ptr, n_q, cand, n_cand, known_pair_keys, known_pair_ptr,
                                   known_rel, n_known_pairs, aggregate, k, out_burden, out_best_burden, out_best_pos);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_q > 0 && n_cand > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_addon_burden_supported(n_nodes, dim, n_rel, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rel_w) & 15) != 0 || !ab_counts_ok(cand_ptr, n_q, n_cand)) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_cand == 0) return TIPK_OK;

    AddonArgs a;
    ab_fill_lists(a, n_nodes, n_rel, ctx_drugs, ctx_ptr, n_q, cand, cand_ptr, n_cand, weights, known_pair_keys,
                  known_pair_ptr, known_rel, n_known_pairs, aggregate, k, out_burden, out_best_burden, out_best_pos);
    a.a = z; a.b = rel_w; a.ld = 0; a.dim = dim; a.stride = wt_stride(dim);
    const bool image = tipk_distmult_addon_burden_lds_route(dim, n_rel) != 0;
    const size_t lds = (image ? (size_t)n_rel * a.stride * 4 : 0) + (size_t)ab_fixed_bytes(dim, false);
    const int grid = wt_grid(a.n_tasks, image ? 1 : 2);                // the image allows one workgroup per CU
    hipStream_t st = (hipStream_t)stream;
    int status;
    if (image)
        status = dim == 16 ? wt_launch<addon_burden_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                           : wt_launch<addon_burden_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
    else
        status = dim == 16 ? wt_launch<addon_burden_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                           : wt_launch<addon_burden_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
    return ab_select(a, status, st);
}

extern "C" int tipk_pair_table_addon_burden_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return wt_table_shape(n_nodes, n_rel) && k >= 0 && k <= WT_KMAX;
}

extern "C" int tipk_pair_table_addon_burden(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                            const int32_t* ctx_drugs, const int64_t* ctx_ptr, int64_t n_q,
                                            const int32_t* cand, const int64_t* cand_ptr, int64_t n_cand,
                                            const float* weights, const int64_t* known_pair_keys,
                                            const int64_t* known_pair_ptr, const int32_t* known_rel, int64_t n_known_pairs,
                                            int aggregate, int k, float* out_burden, float* out_best_burden,
                                            int32_t* out_best_pos, tipk_stream_t stream) {
    const int bad = ab_check_lists(n_nodes, n_rel, ctx_drugs, ctx_ptr, n_q, cand, n_cand, known_pair_keys, known_pair_ptr,
                                   known_rel, n_known_pairs, aggregate, k, out_burden, out_best_burden, out_best_pos);
    if (bad != TIPK_OK || ld < n_rel) return TIPK_EINVAL;
    if (n_q > 0 && n_cand > 0 && (!s1 || !s2)) return TIPK_EINVAL;
    if (!tipk_pair_table_addon_burden_supported(n_nodes, n_rel, k)) return TIPK_EUNSUPPORTED;
    if (!ab_counts_ok(cand_ptr, n_q, n_cand)) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_cand == 0) return TIPK_OK;

    AddonArgs a;
    ab_fill_lists(a, n_nodes, n_rel, ctx_drugs, ctx_ptr, n_q, cand, cand_ptr, n_cand, weights, known_pair_keys,
                  known_pair_ptr, known_rel, n_known_pairs, aggregate, k, out_burden, out_best_burden, out_best_pos);
    a.a = s1; a.b = s2; a.ld = ld; a.dim = 0; a.stride = 0;
    hipStream_t st = (hipStream_t)stream;
    const int status = wt_launch<addon_burden_kernel<WT_TABLE, false>>(a, wt_grid(a.n_tasks, 2),
                                                                        (size_t)ab_fixed_bytes(0, true), st);
    return ab_select(a, status, st);
}
