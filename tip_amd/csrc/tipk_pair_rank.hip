// Pair rank: the filtered rank of given relations (held-out side effects) among all relations of their pair
// (include/tipk.h section 4f).
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 pairs, ONE WAVEFRONT PER PAIR.  The
// logits, the known bitmap, the counting step and the total order are the shared pieces of tipk_wave_topk.h, so rank - 1
// is the position the pair top-k gives; this file holds the pair / chunk / window loop.
// Targets.  The wave holds the pair's targets in chunks of 64, one per lane, and computes their logits first, with the
//   same fma chain every candidate gets (a target is a candidate of the other targets).
// Scoring.  DistMult: the wave leaves h = z[u] * z[v] (rounded once) in its LDS row; lane l scores relations l, l + 64, ...
//   with the shared fma chain.  LDS route: the rows come from an LDS image of rel_w staged once per workgroup.  Global
//   route (the image does not fit, or option "pair_rank_stream"): each lane reads its rows from global memory.  Same
//   arithmetic in the same order: same bits.
//   Table variant: lane l adds s1[u][r] + s2[v][r] from the two (coalesced) table rows.
//   A relation is scored once per chunk of 64 targets, i.e. once per pair unless the pair has more than 64 targets.
// Known filter.  One 64-ary search per pair finds the pair's block of known_rel; the block is merged into a 2 048-bit LDS
//   bitmap of the wave, one window of relations at a time, by a cursor that only moves forward.  A known relation's logit
//   becomes NaN, which beats nothing; so does the logit of a lane beyond n_rel.
// Counting.  For a window of 64 candidate logits the wave walks the chunk's targets: target j's (logit, id) is read from lane
//   j, every lane tests its candidate against it under the total order, and the ballot's population count goes to lane j's
//   counter.  The cost follows the number of targets (about 7 per pair on BioSNAP), no LDS traffic, no atomics.  The order
//   is irreflexive, so a target never counts itself, listed or not.
#include "tipk_wave_topk.h"

namespace {

struct PairRankArgs {
    const float* a;            // z [n x dim]            | s1 [n x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2 [n x ld]
    const int32_t* pu;
    const int32_t* pv;
    const int64_t* tptr;       // [n_pairs + 1]
    const int32_t* trel;       // [n_tgt]
    const int64_t* kkeys;      // nullable with kptr, krel
    const int64_t* kptr;
    const int32_t* krel;
    int64_t n_known, n_pairs, n_tgt, ld;
    int n, dim, n_rel, stride;
    int32_t* out_rank;
    float* out_logit;          // nullable
};

template <int MODE, bool GLOBAL>
__global__ void __launch_bounds__(WT_NT) pair_rank_kernel(PairRankArgs a) {
    extern __shared__ __align__(16) unsigned char pr_smem[];
    const int t = threadIdx.x, lane = tipk_lane();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int R = a.n_rel, dim = a.dim;
    // the row stride of whatever holds rel_w: the LDS image's, or dim in global memory
    const int wstride = GLOBAL ? dim : a.stride;

    // LDS: [rel_w image] [h rows] | bitmaps
    float* Ws = reinterpret_cast<float*>(pr_smem);
    float* hs_all = Ws + ((MODE == WT_TABLE || GLOBAL) ? 0 : R * a.stride);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(hs_all + (MODE == WT_TABLE ? 0 : WT_NW * dim));
    float* hs = hs_all + wave * dim;
    uint32_t* km = km_all + wave * (WT_WIN / 32);
    const float* W = GLOBAL ? a.b : Ws;

    if (MODE != WT_TABLE && !GLOBAL) {
        wt_stage_rows<WT_NT>(Ws, a.b, 0, R, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_pairs + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t p = blk * WT_NW + wave;
        if (p >= a.n_pairs) continue;                                  // uniform in the wave; the waves never meet again
        int64_t tb, te;
        if (!wt_target_range(a.tptr, p, a.n_tgt, tb, te)) continue;
        const int u = a.pu[p], v = a.pv[p];
        const bool act = u >= 0 && u < a.n && v >= 0 && v < a.n;
        int64_t kbeg = 0, kend = 0;
        float4 hq[MODE == WT_DISTMULT16 ? 4 : 1];
        if (act) {
            if (MODE != WT_TABLE) {
                wave_sync();                                           // the previous pair's reads of the row are done
                wt_write_row(hs, a.a + (int64_t)u * dim, a.a + (int64_t)v * dim, dim, lane);
                wave_sync();
                wt_row16<MODE>(hq, hs);
            }
            if (a.kkeys) {
                const int lo = u < v ? u : v, hi = u < v ? v : u;
                const int64_t at = find_key(a.kkeys, a.n_known, (int64_t)lo * a.n + hi, lane);
                if (at >= 0) { kbeg = a.kptr[at]; kend = a.kptr[at + 1]; }
            }
        }
        const bool filt = kbeg < kend;

        for (int64_t ch = tb; ch < te; ch += TIPK_WAVE) {
            const int nt = te - ch < TIPK_WAVE ? (int)(te - ch) : TIPK_WAVE;
            const int tr = lane < nt ? a.trel[ch + lane] : -1;
            const bool tok = act && tr >= 0 && tr < R;
            float ts = NAN;
            if (tok) {
                if (MODE == WT_TABLE) ts = a.a[(int64_t)u * a.ld + tr] + a.b[(int64_t)v * a.ld + tr];
                else ts = wt_dot<MODE>(W + (int64_t)tr * wstride, hs, hq, dim);
            }
            int cnt = 0;
            if (act) {
                int64_t kc = kbeg;
                for (int c0 = 0; c0 < R; c0 += WT_WIN) {
                    const int c1 = c0 + WT_WIN < R ? c0 + WT_WIN : R;
                    if (filt) {
                        // the known relations of [c0, c1) as bits; the cursor kc passes every id below c1
                        wave_sync();                                   // the previous window's bits have been read
                        wt_merge_window<WT_WIN / 32>(km, kc, kend, c0, c1, lane, [&](int64_t idx) { return a.krel[idx]; });
                        wave_sync();
                    }
                    for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                        const int r = g0 + lane;
                        bool cand = r < c1;
                        if (cand && filt) cand = !wt_bit(km, r - c0);
                        float s = NAN;                                 // NaN beats nothing
                        if (cand) {
                            if (MODE == WT_TABLE) s = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                            else s = wt_dot<MODE>(W + (int64_t)r * wstride, hs, hq, dim);
                        }
                        wt_count_beaten(cnt, s, r, ts, tr, nt, lane);
                    }
                }
            }
            wt_write_rank(a.out_rank, a.out_logit, ch, nt, tok, cnt, ts, lane);
        }
    }
}

int64_t pr_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * dim * 4) + (int64_t)WT_NW * (WT_WIN / 32) * 4;
}

int pr_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                   const int64_t* tgt_ptr, const int32_t* tgt_rel, int64_t n_tgt, const int64_t* keys, const int64_t* kptr,
                   const int32_t* krel, int64_t n_known, const int32_t* out_rank) {
    if (n_pairs < 0 || n_tgt < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    if (!wt_known_ok(keys, kptr, krel)) return TIPK_EINVAL;
    if (n_pairs > 0 && n_tgt > 0 && (!pair_u || !pair_v || !tgt_ptr || !tgt_rel || !out_rank)) return TIPK_EINVAL;
    return TIPK_OK;
}

void pr_fill_lists(PairRankArgs& a, const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs, const int64_t* tgt_ptr,
                   const int32_t* tgt_rel, int64_t n_tgt, const int64_t* keys, const int64_t* kptr, const int32_t* krel,
                   int64_t n_known, int32_t* out_rank, float* out_logit) {
    a.pu = pair_u; a.pv = pair_v; a.tptr = tgt_ptr; a.trel = tgt_rel;
    a.kkeys = n_known > 0 ? keys : nullptr; a.kptr = kptr; a.krel = krel;
    a.n_known = n_known; a.n_pairs = n_pairs; a.n_tgt = n_tgt;
    a.out_rank = out_rank; a.out_logit = out_logit;
}

}  // namespace

extern "C" int tipk_distmult_pair_rank_supported(int64_t n_nodes, int dim, int64_t n_rel) {
    return wt_distmult_shape(n_nodes, dim, n_rel);
}

extern "C" int tipk_distmult_pair_rank_lds_route(int dim, int64_t n_rel) {
    return wt_distmult_shape(1, dim, n_rel) && wt_fits_lds(n_rel, dim, pr_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_PAIR_RANK_STREAM);
}

extern "C" int tipk_distmult_pair_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                       const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                                       const int64_t* tgt_ptr, const int32_t* tgt_rel, int64_t n_tgt,
                                       const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                       const int32_t* known_rel, int64_t n_known_pairs, int32_t* out_rank, float* out_logit,
                                       tipk_stream_t stream) {
    const int bad = pr_check_lists(n_nodes, n_rel, pair_u, pair_v, n_pairs, tgt_ptr, tgt_rel, n_tgt, known_pair_keys,
                                   known_pair_ptr, known_rel, n_known_pairs, out_rank);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_pairs > 0 && n_tgt > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_pair_rank_supported(n_nodes, dim, n_rel)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rel_w) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_pairs == 0 || n_tgt == 0) return TIPK_OK;

    PairRankArgs a;
    pr_fill_lists(a, pair_u, pair_v, n_pairs, tgt_ptr, tgt_rel, n_tgt, known_pair_keys, known_pair_ptr, known_rel,
                  n_known_pairs, out_rank, out_logit);
    a.a = z; a.b = rel_w; a.ld = 0;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel; a.stride = wt_stride(dim);
    const bool lds_route = tipk_distmult_pair_rank_lds_route(dim, n_rel) != 0;
    const size_t lds = (lds_route ? (size_t)n_rel * a.stride * 4 : 0) + (size_t)pr_fixed_bytes(dim, false);
    const int grid = wt_grid(n_pairs, 1);                              // one workgroup per CU: the image fills its LDS
    hipStream_t st = (hipStream_t)stream;
    if (lds_route)
        return dim == 16 ? wt_launch<pair_rank_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                         : wt_launch<pair_rank_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
    return dim == 16 ? wt_launch<pair_rank_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                     : wt_launch<pair_rank_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_pair_rank_supported(int64_t n_nodes, int64_t n_rel) {
    return wt_table_shape(n_nodes, n_rel);
}

extern "C" int tipk_pair_table_pair_rank(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                         const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                                         const int64_t* tgt_ptr, const int32_t* tgt_rel, int64_t n_tgt,
                                         const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                         const int32_t* known_rel, int64_t n_known_pairs, int32_t* out_rank,
                                         float* out_logit, tipk_stream_t stream) {
    const int bad = pr_check_lists(n_nodes, n_rel, pair_u, pair_v, n_pairs, tgt_ptr, tgt_rel, n_tgt, known_pair_keys,
                                   known_pair_ptr, known_rel, n_known_pairs, out_rank);
    if (bad != TIPK_OK || ld < n_rel) return TIPK_EINVAL;
    if (n_pairs > 0 && n_tgt > 0 && (!s1 || !s2)) return TIPK_EINVAL;
    if (!tipk_pair_table_pair_rank_supported(n_nodes, n_rel)) return TIPK_EUNSUPPORTED;
    if (n_pairs == 0 || n_tgt == 0) return TIPK_OK;

    PairRankArgs a;
    pr_fill_lists(a, pair_u, pair_v, n_pairs, tgt_ptr, tgt_rel, n_tgt, known_pair_keys, known_pair_ptr, known_rel,
                  n_known_pairs, out_rank, out_logit);
    a.a = s1; a.b = s2; a.ld = ld;
    a.n = (int)n_nodes; a.dim = 0; a.n_rel = (int)n_rel; a.stride = 0;
    const int grid = wt_grid(n_pairs, 2);                              // 4 KB of LDS each: two workgroups share a CU
    return wt_launch<pair_rank_kernel<WT_TABLE, false>>(a, grid, (size_t)pr_fixed_bytes(0, true), (hipStream_t)stream);
}
