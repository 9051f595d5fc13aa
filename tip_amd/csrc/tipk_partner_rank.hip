// Partner rank: the filtered rank of given partners (held-out drugs) among all drugs, for (relation, drug) queries
// (include/tipk.h section 4g) -- the evaluation of what the screen's drug queries (4c) serve.
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 queries, ONE WAVEFRONT PER QUERY.  The
// logits and the total order are those of a 4c drug query.  The fma chain, the bitmap merge and the counting step are the
// shared pieces of tipk_wave_topk.h; this file holds the query / chunk / window loop and the reverse-key filter.
// Targets.  The wave holds the query's targets in chunks of 64, one per lane, and computes their logits first, with the
//   same fma chain every candidate gets (a target is a candidate of the other targets).
// Scoring.  DistMult: the wave leaves a = z[u] * w[r] (rounded once) in its LDS row (dim 16: in registers); lane l scores
//   drugs l, l + 64, ... as acc = fmaf(a[k], z[c][k], acc), k ascending (the shared chain).  LDS route: the rows come from
//   an LDS image of z staged once per workgroup.  Global route (the image does not fit, or option "partner_rank_global"):
//   each lane reads its rows from global memory.  Same arithmetic in the same order: same bits.
//   Table variant: lane l adds s1t[r][u] + s2t[r][c] -- the relation's (coalesced) row of the transposed table.
//   A drug is scored once per chunk of 64 targets, i.e. once per query unless the query has more than 64 targets.
// Known filter.  Forward keys u*n+c: two 64-ary searches bound the run [u*n, (u+1)*n) inside relation r's block; that run
//   is the query's ascending partner list and is merged into a 2 048-bit LDS bitmap of the wave, one window of drugs at a
//   time, by a cursor that only moves forward.  Reverse keys c*n+u: a binary search in the relation's block per candidate,
//   run only for a candidate that is not flagged already and beats the chunk's WEAKEST target under the total order (the
//   order is total, so a candidate that beats any target beats the weakest one; all others change no count).  A dropped
//   candidate's logit becomes NaN, which beats nothing; so does the logit of u itself and of a lane beyond n_nodes.
// Counting.  For a window of 64 candidate logits the wave walks the chunk's targets: target j's (logit, id) is read from lane
//   j, every lane tests its candidate against it under the total order, and the ballot's population count goes to lane j's
//   counter.  No LDS traffic, no atomics.  The order is irreflexive, so a target never counts itself, listed or not.
#include "tipk_wave_topk.h"

namespace {

struct PartnerRankArgs {
    const float* a;            // z [n x dim]            | s1t [n_rel x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2t [n_rel x ld]
    const int32_t* qrel;
    const int32_t* qdrug;
    const int64_t* tptr;       // [n_q + 1]
    const int32_t* tnode;      // [n_tgt]
    const int64_t* kkeys;      // nullable with kptr
    const int64_t* kptr;       // [n_rel + 1]
    int64_t n_q, n_tgt, ld;
    int n, dim, n_rel, stride;
    int32_t* out_rank;
    float* out_logit;          // nullable
};

__device__ __forceinline__ bool qr_key_in(const int64_t* keys, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t v = keys[mid];
        if (v == x) return true;
        if (v < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

template <int MODE, bool GLOBAL>
__global__ void __launch_bounds__(WT_NT) partner_rank_kernel(PartnerRankArgs a) {
    extern __shared__ __align__(16) unsigned char qr_smem[];
    const int t = threadIdx.x, lane = tipk_lane();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, dim = a.dim;
    // the row stride of whatever holds z: the LDS image's, or dim in global memory
    const int zstride = GLOBAL ? dim : a.stride;

    // LDS: [z image] [a rows] | bitmaps
    float* Zs = reinterpret_cast<float*>(qr_smem);
    float* as_all = Zs + ((MODE == WT_TABLE || GLOBAL) ? 0 : n * a.stride);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(as_all + (MODE == WT_TABLE ? 0 : WT_NW * dim));
    float* as = as_all + wave * dim;
    uint32_t* km = km_all + wave * (WT_WIN / 32);
    const float* Z = GLOBAL ? a.a : Zs;

    if (MODE != WT_TABLE && !GLOBAL) {
        wt_stage_rows<WT_NT>(Zs, a.a, 0, n, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_q + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t qi = blk * WT_NW + wave;
        if (qi >= a.n_q) continue;                                     // uniform in the wave; the waves never meet again
        int64_t tb, te;
        if (!wt_target_range(a.tptr, qi, a.n_tgt, tb, te)) continue;
        const int r = a.qrel[qi], u = a.qdrug[qi];
        const bool act = r >= 0 && r < a.n_rel && u >= 0 && u < n;
        int64_t klo = 0, khi = 0, fbeg = 0, fend = 0;                  // relation r's block; its keys [u*n, (u+1)*n)
        float4 aq[MODE == WT_DISTMULT16 ? 4 : 1];
        float s1u = 0.f;
        const float* s2r = nullptr;
        if (act) {
            if (MODE != WT_TABLE) {
                wave_sync();                                           // the previous query's reads of the row are done
                wt_write_row(as, a.a + (int64_t)u * dim, a.b + (int64_t)r * dim, dim, lane);
                wave_sync();
                wt_row16<MODE>(aq, as);
            } else {
                s1u = a.a[(int64_t)r * a.ld + u];
                s2r = a.b + (int64_t)r * a.ld;
            }
            if (a.kkeys) {
                klo = a.kptr[r];
                khi = a.kptr[r + 1];
                if (klo < khi) {
                    fbeg = wt_lower_bound(a.kkeys, klo, khi, (int64_t)u * n, lane);
                    fend = wt_lower_bound(a.kkeys, fbeg, khi, (int64_t)(u + 1) * n, lane);
                }
            }
        }
        const bool fwd = fbeg < fend, rev = klo < khi;

        for (int64_t ch = tb; ch < te; ch += TIPK_WAVE) {
            const int nt = te - ch < TIPK_WAVE ? (int)(te - ch) : TIPK_WAVE;
            const int tn = lane < nt ? a.tnode[ch + lane] : -1;
            const bool tok = act && tn >= 0 && tn < n && tn != u;
            float ts = NAN;
            if (tok) {
                if (MODE == WT_TABLE) ts = s1u + s2r[tn];
                else ts = wt_dot<MODE>(Z + (int64_t)tn * zstride, as, aq, dim);
            }
            // the chunk's weakest ranked target under the total order: a candidate that does not beat it beats none
            float ws = ts;
            int wt = (tok && ts == ts) ? tn : -1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float os = __shfl_xor(ws, off);
                const int ot = __shfl_xor(wt, off);
                if (ot >= 0 && (wt < 0 || better(ws, wt, os, ot))) { ws = os; wt = ot; }
            }
            int cnt = 0;
            if (wt >= 0) {
                int64_t kc = fbeg;
                for (int c0 = 0; c0 < n; c0 += WT_WIN) {
                    const int c1 = c0 + WT_WIN < n ? c0 + WT_WIN : n;
                    if (fwd) {
                        // the query's known partners in [c0, c1) as bits; the cursor kc passes every partner below c1
                        wave_sync();                                   // the previous window's bits have been read
                        wt_merge_window<WT_WIN / 32>(km, kc, fend, c0, c1, lane,
                                                     [&](int64_t idx) { return a.kkeys[idx] - (int64_t)u * n; });
                        wave_sync();
                    }
                    for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                        const int c = g0 + lane;
                        bool cand = c < c1 && c != u;
                        if (cand && fwd) cand = !wt_bit(km, c - c0);
                        float s = NAN;                                 // NaN beats nothing
                        if (cand) {
                            if (MODE == WT_TABLE) s = s1u + s2r[c];
                            else s = wt_dot<MODE>(Z + (int64_t)c * zstride, as, aq, dim);
                            if (rev && better(s, c, ws, wt) && qr_key_in(a.kkeys, klo, khi, (int64_t)c * n + u)) s = NAN;
                        }
                        wt_count_beaten(cnt, s, c, ts, tn, nt, lane);
                    }
                }
            }
            wt_write_rank(a.out_rank, a.out_logit, ch, nt, tok, cnt, ts, lane);
        }
    }
}

int64_t qr_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * dim * 4) + (int64_t)WT_NW * (WT_WIN / 32) * 4;
}

int qr_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* q_rel, const int32_t* q_drug, int64_t n_q,
                   const int64_t* tgt_ptr, const int32_t* tgt_node, int64_t n_tgt, const int64_t* keys, const int64_t* kptr,
                   const int32_t* out_rank) {
    if (n_q < 0 || n_tgt < 0 || n_nodes < 1 || n_rel < 1) return TIPK_EINVAL;
    if ((keys != nullptr) != (kptr != nullptr)) return TIPK_EINVAL;
    if (n_q > 0 && n_tgt > 0 && (!q_rel || !q_drug || !tgt_ptr || !tgt_node || !out_rank)) return TIPK_EINVAL;
    return TIPK_OK;
}

void qr_fill_lists(PartnerRankArgs& a, const int32_t* q_rel, const int32_t* q_drug, int64_t n_q, const int64_t* tgt_ptr,
                   const int32_t* tgt_node, int64_t n_tgt, const int64_t* keys, const int64_t* kptr, int32_t* out_rank,
                   float* out_logit) {
    a.qrel = q_rel; a.qdrug = q_drug; a.tptr = tgt_ptr; a.tnode = tgt_node;
    a.kkeys = keys; a.kptr = kptr;
    a.n_q = n_q; a.n_tgt = n_tgt;
    a.out_rank = out_rank; a.out_logit = out_logit;
}

}  // namespace

extern "C" int tipk_distmult_partner_rank_supported(int64_t n_nodes, int dim, int64_t n_rel) {
    return wt_distmult_shape(n_nodes, dim, n_rel);
}

extern "C" int tipk_distmult_partner_rank_lds_route(int64_t n_nodes, int dim) {
    return wt_distmult_shape(n_nodes, dim, 1) && wt_fits_lds(n_nodes, dim, qr_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_PARTNER_RANK_GLOBAL);
}

extern "C" int tipk_distmult_partner_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                          const int32_t* q_rel, const int32_t* q_drug, int64_t n_q, const int64_t* tgt_ptr,
                                          const int32_t* tgt_node, int64_t n_tgt, const int64_t* known_keys,
                                          const int64_t* known_ptr, int32_t* out_rank, float* out_logit,
                                          tipk_stream_t stream) {
    const int bad = qr_check_lists(n_nodes, n_rel, q_rel, q_drug, n_q, tgt_ptr, tgt_node, n_tgt, known_keys, known_ptr,
                                   out_rank);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_q > 0 && n_tgt > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_partner_rank_supported(n_nodes, dim, n_rel)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_tgt == 0) return TIPK_OK;

    PartnerRankArgs a;
    qr_fill_lists(a, q_rel, q_drug, n_q, tgt_ptr, tgt_node, n_tgt, known_keys, known_ptr, out_rank, out_logit);
    a.a = z; a.b = rel_w; a.ld = 0;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel; a.stride = wt_stride(dim);
    const bool lds_route = tipk_distmult_partner_rank_lds_route(n_nodes, dim) != 0;
    const size_t lds = (lds_route ? (size_t)n_nodes * a.stride * 4 : 0) + (size_t)qr_fixed_bytes(dim, false);
    const int grid = wt_grid(n_q, 1);                                  // one workgroup of 16 waves per CU
    hipStream_t st = (hipStream_t)stream;
    if (lds_route)
        return dim == 16 ? wt_launch<partner_rank_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                         : wt_launch<partner_rank_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
    return dim == 16 ? wt_launch<partner_rank_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                     : wt_launch<partner_rank_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_partner_rank_supported(int64_t n_nodes, int64_t n_rel) {
    return wt_table_shape(n_nodes, n_rel);
}

extern "C" int tipk_pair_table_partner_rank(const float* s1t, const float* s2t, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                            const int32_t* q_rel, const int32_t* q_drug, int64_t n_q, const int64_t* tgt_ptr,
                                            const int32_t* tgt_node, int64_t n_tgt, const int64_t* known_keys,
                                            const int64_t* known_ptr, int32_t* out_rank, float* out_logit,
                                            tipk_stream_t stream) {
    const int bad = qr_check_lists(n_nodes, n_rel, q_rel, q_drug, n_q, tgt_ptr, tgt_node, n_tgt, known_keys, known_ptr,
                                   out_rank);
    if (bad != TIPK_OK || ld < n_nodes) return TIPK_EINVAL;
    if (n_q > 0 && n_tgt > 0 && (!s1t || !s2t)) return TIPK_EINVAL;
    if (!tipk_pair_table_partner_rank_supported(n_nodes, n_rel)) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_tgt == 0) return TIPK_OK;

    PartnerRankArgs a;
    qr_fill_lists(a, q_rel, q_drug, n_q, tgt_ptr, tgt_node, n_tgt, known_keys, known_ptr, out_rank, out_logit);
    a.a = s1t; a.b = s2t; a.ld = ld;
    a.n = (int)n_nodes; a.dim = 0; a.n_rel = (int)n_rel; a.stride = 0;
    const int grid = wt_grid(n_q, 2);                                  // 4 KB of LDS each: two workgroups share a CU
    return wt_launch<partner_rank_kernel<WT_TABLE, false>>(a, grid, (size_t)qr_fixed_bytes(0, true), (hipStream_t)stream);
}
