// Regimen top-k: the k best relations of every drug list, aggregated over the list's pairs, with the pair that drives each
// (include/tipk.h section 4e).  The logit, the known bitmap and the bitonic cut are the shared pieces of tipk_wave_topk.h;
// this file holds the window / pair loop and the aggregation.
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 regimens, ONE WAVEFRONT PER REGIMEN.
// Lane l keeps the regimen's l-th drug id (a regimen has at most 64 entries), so a pair's ids are two lane reads.
// Windows.  The relation axis is walked in windows of 64 x RG_A relations: lane l owns relations c0 + l, c0 + l + 64, ...
//   with RG_A aggregate / best-logit / best-pair registers.  Per window the wave loops over the regimen's pairs in pair
//   order; per pair it scores its RG_A relations (h = z[u] * z[v] rounded once into the wave's LDS row, then the shared
//   fma chain; table variant: one add of the two coalesced table rows) and updates the registers unless
//   the triple is known or its logit is NaN.  The noisy-or sum therefore runs in pair order, in fp32, per relation.
// rel_w.  An LDS image, staged once per workgroup, when it fits beside the waves' state;
//   otherwise (or under option "regimen_global") each lane reads its rows from global memory.  Same arithmetic, same bits.
// Known filter.  One 64-ary search per pair finds the pair's block of known_rel; its position is kept in LDS for the first
//   RG_ATC pairs of the regimen so that later windows do not search again.  A 64-ary lower bound inside the block gives
//   the window's start; the window's known ids become bits of a per-wave LDS bitmap that every scoring step tests.
// Selection.  After the last pair of a window, the shared selection (aggregate desc, relation asc).  The driver pair
//   travels with its entry as a 16-bit tag (i | j << 8).
#include "tipk_wave_topk.h"

namespace {

constexpr int RG_M_MAX = TIPK_WAVE;         // drugs per regimen: one lane each
constexpr int RG_A = 4;                     // relations per lane and window
constexpr int RG_WIN = TIPK_WAVE * RG_A;    // relations per window
constexpr int RG_ATC = 256;                 // pairs per regimen whose known-block position is kept in LDS

struct RegimenArgs {
    const float* a;            // z [n x dim]            | s1 [n x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2 [n x ld]
    const int32_t* drugs;
    const int64_t* ptr;
    const int64_t* kkeys;      // nullable with kptr, krel
    const int64_t* kptr;
    const int32_t* krel;
    int64_t n_known, n_reg, ld;
    int n, dim, n_rel, k, stride, noisy;
    float* out_s;
    int32_t* out_r;
    int32_t* out_p;
};

template <int MODE, bool IMAGE>
__global__ void __launch_bounds__(WT_NT) regimen_topk_kernel(RegimenArgs a) {
    extern __shared__ __align__(16) unsigned char rg_smem[];
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
    const int k = a.k, R = a.n_rel, dim = a.dim;
    const int flush_at = wt_flush_at(k);
    const int gdim = MODE == WT_DISTMULT16 ? 16 : dim;                // row stride of rel_w in global memory: a shift for dim 16

    // LDS: [rel_w image] [h rows] | aggregate buffers | relation buffers | known-block positions | bitmaps | pair tags
    float* Ws = reinterpret_cast<float*>(rg_smem);
    float* hs_all = Ws + (IMAGE ? R * a.stride : 0);
    float* bs_all = hs_all + (MODE == WT_TABLE ? 0 : WT_NW * dim);
    int* br_all = reinterpret_cast<int*>(bs_all + WT_NW * WT_CAP);
    int* atc_all = br_all + WT_NW * WT_CAP;
    uint32_t* km_all = reinterpret_cast<uint32_t*>(atc_all + WT_NW * RG_ATC);
    uint16_t* bt_all = reinterpret_cast<uint16_t*>(km_all + WT_NW * (RG_WIN / 32));
    float* hs = hs_all + wave * dim;
    float* bs = bs_all + wave * WT_CAP;
    int* br = br_all + wave * WT_CAP;
    int* atc = atc_all + wave * RG_ATC;
    uint32_t* km = km_all + wave * (RG_WIN / 32);
    uint16_t* bt = bt_all + wave * WT_CAP;

    if (IMAGE) {
        wt_stage_rows<WT_NT>(Ws, a.b, 0, R, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_reg + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t g = blk * WT_NW + wave;
        if (g >= a.n_reg) continue;                                    // (the waves of a workgroup never meet in this loop)
        const int64_t p0 = a.ptr[g], m64 = a.ptr[g + 1] - p0;
        bool act = m64 >= 2 && m64 <= RG_M_MAX;                        // uniform in the wave
        const int m = act ? (int)m64 : 0;
        int dl = 0;
        if (act) {
            if (lane < m) dl = a.drugs[p0 + lane];
            act = __ballot(lane < m && (dl < 0 || dl >= a.n)) == 0ull;
        }
        int c = 0;
        float thr = -INFINITY;
        wave_sync();                                                   // the previous regimen's buffer has been written out

        for (int c0 = 0; act && c0 < R; c0 += RG_WIN) {
            const int c1 = c0 + RG_WIN < R ? c0 + RG_WIN : R;
            float agg[RG_A], best[RG_A];
            int bpr[RG_A];                                             // i | j << 8 of the best contributing pair, -1: none yet
#pragma unroll
            for (int x = 0; x < RG_A; ++x) { agg[x] = 0.f; best[x] = -INFINITY; bpr[x] = -1; }

            int pi = 0;
            for (int i = 0; i + 1 < m; ++i) {
                const int u = __shfl(dl, i);
                for (int j = i + 1; j < m; ++j, ++pi) {
                    const int v = __shfl(dl, j);
                    float4 hq[MODE == WT_DISTMULT16 ? 4 : 1];
                    wave_sync();                                       // the previous pair is done with hs and km
                    if (MODE != WT_TABLE) wt_write_row(hs, a.a + (int64_t)u * dim, a.a + (int64_t)v * dim, dim, lane);
                    bool filt = false;
                    if (a.kkeys) {
                        int at;
                        if (c0 == 0 || pi >= RG_ATC) {
                            const int lo = u < v ? u : v, hi = u < v ? v : u;
                            at = (int)find_key(a.kkeys, a.n_known, (int64_t)lo * a.n + hi, lane);
                            if (c0 == 0 && pi < RG_ATC && lane == 0) atc[pi] = at;
                        } else {
                            at = atc[pi];
                        }
                        if (at >= 0) {
                            int64_t kc = a.kptr[at];
                            const int64_t kend = a.kptr[at + 1];
                            if (c0 > 0) kc = wt_lower_bound(a.krel, kc, kend, c0, lane);
                            const int first = kc < kend ? a.krel[kc] : WT_REL_PAD;
                            if (first < c1) {
                                // no fence in front of the clear: the one at the top of the pair loop serves
                                filt = true;
                                wt_merge_window<RG_WIN / 32>(km, kc, kend, c0, c1, lane,
                                                             [&](int64_t idx) { return a.krel[idx]; });
                            }
                        }
                    }
                    wave_sync();
                    wt_row16<MODE>(hq, hs);
                    const int tag = i | (j << 8);
#pragma unroll
                    for (int x = 0; x < RG_A; ++x) {
                        const int r = c0 + x * TIPK_WAVE + lane;
                        if (c0 + x * TIPK_WAVE >= c1) break;           // uniform
                        if (r >= c1) continue;
                        float s = 0.f;
                        if (MODE == WT_TABLE) s = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                        else s = wt_dot<MODE>(IMAGE ? Ws + r * a.stride : a.b + (int64_t)r * gdim, hs, hq, dim);
                        bool take = s == s;                            // a NaN logit contributes nothing
                        // the bit test, the append and the write-out below are written out here and in the pair top-k:
                        // as shared helpers they measured 1 % slower on the table variants
                        // (profiles/wave_rows_refactor.md)
                        if (take && filt) {
                            const int bit = r - c0;
                            take = !((km[bit >> 5] >> (bit & 31)) & 1u);
                        }
                        if (take) {
                            if (bpr[x] < 0 || s > best[x]) { best[x] = s; bpr[x] = tag; }   // ties: the first in pair order
                            if (a.noisy) agg[x] += wt_softplus(s);
                        }
                    }
                }
            }

            // the window's candidates: relations with a contributing triple
#pragma unroll
            for (int x = 0; x < RG_A; ++x) {
                if (c0 + x * TIPK_WAVE >= c1) break;                   // uniform
                const int r = c0 + x * TIPK_WAVE + lane;
                const float val = a.noisy ? agg[x] : best[x];
                const bool pass = r < c1 && bpr[x] >= 0 && val >= thr;
                const unsigned long long mask = __ballot(pass);
                if (mask == 0ull) continue;
                if (pass) {
                    const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                    bs[pos] = val;
                    br[pos] = r;
                    bt[pos] = (uint16_t)bpr[x];
                }
                c += __popcll(mask);
                if (c >= flush_at) flush<true>(bs, br, bt, c, thr, k, lane);
            }
        }

        if (c > 0) flush<true>(bs, br, bt, c, thr, k, lane);
        float* os = a.out_s + g * k;
        int32_t* orl = a.out_r + g * k;
        int32_t* op = a.out_p + g * k;
        for (int i = lane; i < k; i += TIPK_WAVE) {
            const bool have = i < c;
            const int tag = have ? bt[i] : 0;
            os[i] = have ? bs[i] : -INFINITY;
            orl[i] = have ? br[i] : -1;
            op[i] = have ? ((tag & 0xff) | ((tag >> 8) << 16)) : -1;
        }
    }
}

int64_t rg_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * dim * 4) + (int64_t)WT_NW * WT_CAP * 10 + (int64_t)WT_NW * RG_ATC * 4 +
           (int64_t)WT_NW * (RG_WIN / 32) * 4;
}

int rg_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* reg_drugs, const int64_t* reg_ptr, int64_t n_regimens,
                   const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int aggregate, int k,
                   const float* out_score, const int32_t* out_rel, const int32_t* out_pair) {
    if (k <= 0 || n_regimens < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    if (aggregate != TIPK_REGIMEN_MAX && aggregate != TIPK_REGIMEN_NOISY_OR) return TIPK_EINVAL;
    if (!wt_known_ok(keys, kptr, krel)) return TIPK_EINVAL;
    if (n_regimens > 0 && (!reg_drugs || !reg_ptr || !out_score || !out_rel || !out_pair)) return TIPK_EINVAL;
    return TIPK_OK;
}

void rg_fill_lists(RegimenArgs& a, int64_t n_nodes, int64_t n_rel, const int32_t* reg_drugs, const int64_t* reg_ptr,
                   int64_t n_regimens, const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known,
                   int aggregate, int k, float* out_score, int32_t* out_rel, int32_t* out_pair) {
    a.drugs = reg_drugs; a.ptr = reg_ptr;
    a.kkeys = n_known > 0 ? keys : nullptr; a.kptr = kptr; a.krel = krel;
    a.n_known = n_known; a.n_reg = n_regimens;
    a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.k = k;
    a.noisy = aggregate == TIPK_REGIMEN_NOISY_OR;
    a.out_s = out_score; a.out_r = out_rel; a.out_p = out_pair;
}

}  // namespace

extern "C" int tipk_regimen_max_drugs(void) { return RG_M_MAX; }

extern "C" int tipk_distmult_regimen_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return wt_distmult_shape(n_nodes, dim, n_rel) && k >= 1 && k <= WT_KMAX;
}

extern "C" int64_t tipk_distmult_regimen_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_regimens,
                                                              int k) {
    if (n_regimens < 0 || !tipk_distmult_regimen_topk_supported(n_nodes, dim, n_rel, k)) return -1;
    return 0;                                                          // every list lives in LDS
}

extern "C" int tipk_distmult_regimen_topk_lds_route(int dim, int64_t n_rel) {
    return wt_distmult_shape(1, dim, n_rel) && wt_fits_lds(n_rel, dim, rg_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_REGIMEN_GLOBAL);
}

extern "C" int tipk_distmult_regimen_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                          const int32_t* reg_drugs, const int64_t* reg_ptr, int64_t n_regimens,
                                          const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                          const int32_t* known_rel, int64_t n_known_pairs, int aggregate, int k,
                                          float* out_score, int32_t* out_rel, int32_t* out_pair, void* workspace,
                                          tipk_stream_t stream) {
    (void)workspace;
    const int bad = rg_check_lists(n_nodes, n_rel, reg_drugs, reg_ptr, n_regimens, known_pair_keys, known_pair_ptr, known_rel,
                                   n_known_pairs, aggregate, k, out_score, out_rel, out_pair);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_regimens > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_regimen_topk_supported(n_nodes, dim, n_rel, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rel_w) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_regimens == 0) return TIPK_OK;

    RegimenArgs a;
    rg_fill_lists(a, n_nodes, n_rel, reg_drugs, reg_ptr, n_regimens, known_pair_keys, known_pair_ptr, known_rel,
                  n_known_pairs, aggregate, k, out_score, out_rel, out_pair);
    a.a = z; a.b = rel_w; a.ld = 0; a.dim = dim; a.stride = wt_stride(dim);
    const bool image = tipk_distmult_regimen_topk_lds_route(dim, n_rel) != 0;
    const size_t lds = (image ? (size_t)n_rel * a.stride * 4 : 0) + (size_t)rg_fixed_bytes(dim, false);
    const int grid = wt_grid(n_regimens, image ? 1 : 2);               // the image allows one workgroup per CU
    hipStream_t st = (hipStream_t)stream;
    if (image)
        return dim == 16 ? wt_launch<regimen_topk_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                         : wt_launch<regimen_topk_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
    return dim == 16 ? wt_launch<regimen_topk_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                     : wt_launch<regimen_topk_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_regimen_topk_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return wt_table_shape(n_nodes, n_rel) && k >= 1 && k <= WT_KMAX;
}

extern "C" int tipk_pair_table_regimen_topk(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                            const int32_t* reg_drugs, const int64_t* reg_ptr, int64_t n_regimens,
                                            const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                            const int32_t* known_rel, int64_t n_known_pairs, int aggregate, int k,
                                            float* out_score, int32_t* out_rel, int32_t* out_pair, tipk_stream_t stream) {
    const int bad = rg_check_lists(n_nodes, n_rel, reg_drugs, reg_ptr, n_regimens, known_pair_keys, known_pair_ptr, known_rel,
                                   n_known_pairs, aggregate, k, out_score, out_rel, out_pair);
    if (bad != TIPK_OK || ld < n_rel) return TIPK_EINVAL;
    if (n_regimens > 0 && (!s1 || !s2)) return TIPK_EINVAL;
    if (!tipk_pair_table_regimen_topk_supported(n_nodes, n_rel, k)) return TIPK_EUNSUPPORTED;
    if (n_regimens == 0) return TIPK_OK;

    RegimenArgs a;
    rg_fill_lists(a, n_nodes, n_rel, reg_drugs, reg_ptr, n_regimens, known_pair_keys, known_pair_ptr, known_rel,
                  n_known_pairs, aggregate, k, out_score, out_rel, out_pair);
    a.a = s1; a.b = s2; a.ld = ld; a.dim = 0; a.stride = 0;
    return wt_launch<regimen_topk_kernel<WT_TABLE, false>>(a, wt_grid(n_regimens, 2), (size_t)rg_fixed_bytes(0, true),
                                                           (hipStream_t)stream);
}
