// Partner rank: the filtered rank of given partners (held-out drugs) among all drugs, for (relation, drug) queries
// (include/tipk.h section 4g) -- the evaluation of what the screen's drug queries (4c) serve.
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 queries, ONE WAVEFRONT PER QUERY, as
// the pair rank (tipk_pair_rank.hip) does.  The logits and the total order are those of a 4c drug query.
// Targets.  The wave holds the query's targets in chunks of 64, one per lane, and computes their logits first, with the
//   same fma chain every candidate gets (a target is a candidate of the other targets).
// Scoring.  DistMult: the wave leaves a = z[u] * w[r] (rounded once) in its LDS row (dim 16: in registers); lane l scores
//   drugs l, l + 64, ... as acc = fmaf(a[k], z[c][k], acc), k ascending.  LDS route: the rows come from an LDS image of z
//   staged once per workgroup (row stride S with S / 4 odd, as in 4d).  Global route (the image does not fit, or option
//   "partner_rank_global"): each lane reads its rows from global memory.  Same arithmetic in the same order: same bits.
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

constexpr int QR_NT = 1024;                 // threads per workgroup
constexpr int QR_NW = QR_NT / TIPK_WAVE;    // queries per block (one per wavefront)
constexpr int QR_DIM_MAX = 256;
constexpr int64_t QR_NMAX = 46340;          // n^2 < 2^31, as 4c
constexpr int64_t QR_RMAX = 65536;
constexpr int QR_WIN = 2048;                // drugs per bitmap window (64 words: lane l clears word l)
constexpr int QR_LDS_BYTES = 152 * 1024;    // dynamic LDS a workgroup may ask for

enum { QR_DISTMULT = 0, QR_DISTMULT16 = 1, QR_TABLE = 2 };

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

// logit of drug c for the wave's query: zc = row c of z (LDS image or global), as = the wave's a row
template <int MODE>
__device__ __forceinline__ float qr_dot(const float* zc, const float* as, const float4* aq, int dim) {
    float s = 0.f;
    if (MODE == QR_DISTMULT16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 z4 = *reinterpret_cast<const float4*>(zc + 4 * q);
            s = fmaf(aq[q].x, z4.x, s);
            s = fmaf(aq[q].y, z4.y, s);
            s = fmaf(aq[q].z, z4.z, s);
            s = fmaf(aq[q].w, z4.w, s);
        }
    } else {
        for (int k0 = 0; k0 < dim; k0 += 4) {
            const float4 z4 = *reinterpret_cast<const float4*>(zc + k0);
            const float4 a4 = *reinterpret_cast<const float4*>(as + k0);
            s = fmaf(a4.x, z4.x, s);
            s = fmaf(a4.y, z4.y, s);
            s = fmaf(a4.z, z4.z, s);
            s = fmaf(a4.w, z4.w, s);
        }
    }
    return s;
}

// first index in [lo, hi) of the ascending keys whose key is >= `key` (hi if none): every lane calls it with the same
// arguments and gets the same answer; the 64 lanes probe 64 keys per step
__device__ int64_t qr_lower_bound(const int64_t* keys, int64_t lo, int64_t hi, int64_t key, int lane) {
    const int64_t big = 0x7fffffffffffffffLL;
    while (hi - lo > TIPK_WAVE) {
        const int64_t step = (hi - lo + TIPK_WAVE - 1) / TIPK_WAVE;
        const int64_t idx = lo + (int64_t)lane * step;
        const int64_t v = idx < hi ? keys[idx] : big;
        const int c = __popcll(__ballot(v < key));               // the probes ascend: the lanes with v < key are a prefix
        if (c == 0) return lo;
        const int64_t top = lo + (int64_t)c * step;              // the first probe that is not below key, or past the end
        lo += (int64_t)(c - 1) * step + 1;
        hi = top < hi ? top : hi;
    }
    const int64_t idx = lo + lane;
    const int64_t v = idx < hi ? keys[idx] : big;
    return lo + __popcll(__ballot(v < key));
}

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
__global__ void __launch_bounds__(QR_NT) partner_rank_kernel(PartnerRankArgs a) {
    extern __shared__ __align__(16) unsigned char qr_smem[];
    const int t = threadIdx.x, lane = tipk_lane();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, dim = a.dim;
    // the row stride of whatever holds z: the LDS image's, or dim in global memory
    const int zstride = GLOBAL ? dim : a.stride;

    // LDS: [z image] [a rows] | bitmaps
    float* Zs = reinterpret_cast<float*>(qr_smem);
    float* as_all = Zs + ((MODE == QR_TABLE || GLOBAL) ? 0 : n * a.stride);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(as_all + (MODE == QR_TABLE ? 0 : QR_NW * dim));
    float* as = as_all + wave * dim;
    uint32_t* km = km_all + wave * (QR_WIN / 32);
    const float* Z = GLOBAL ? a.a : Zs;

    if (MODE != QR_TABLE && !GLOBAL) {
        const int q4 = dim >> 2;
        for (int idx = t; idx < n * q4; idx += QR_NT) {
            const int row = idx / q4, q = idx - row * q4;
            tipk_st4(Zs + row * a.stride + 4 * q, tipk_ld4(a.a + (int64_t)row * dim + 4 * q));
        }
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_q + QR_NW - 1) / QR_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t qi = blk * QR_NW + wave;
        if (qi >= a.n_q) continue;                                     // uniform in the wave; the waves never meet again
        int64_t tb = a.tptr[qi], te = a.tptr[qi + 1];
        tb = tb < 0 ? 0 : tb;                                          // device lists cannot be validated on the host:
        te = te > a.n_tgt ? a.n_tgt : te;                              // nothing outside [0, n_tgt) is read or written
        if (tb >= te) continue;
        const int r = a.qrel[qi], u = a.qdrug[qi];
        const bool act = r >= 0 && r < a.n_rel && u >= 0 && u < n;
        int64_t klo = 0, khi = 0, fbeg = 0, fend = 0;                  // relation r's block; its keys [u*n, (u+1)*n)
        float4 aq[MODE == QR_DISTMULT16 ? 4 : 1];
        float s1u = 0.f;
        const float* s2r = nullptr;
        if (act) {
            if (MODE != QR_TABLE) {
                const float* zu = a.a + (int64_t)u * dim;
                const float* wr = a.b + (int64_t)r * dim;
                wave_sync();                                           // the previous query's reads of the row are done
                for (int kk = lane; kk < dim; kk += TIPK_WAVE) as[kk] = zu[kk] * wr[kk];
                wave_sync();
                if (MODE == QR_DISTMULT16) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) aq[q] = *reinterpret_cast<const float4*>(as + 4 * q);
                }
            } else {
                s1u = a.a[(int64_t)r * a.ld + u];
                s2r = a.b + (int64_t)r * a.ld;
            }
            if (a.kkeys) {
                klo = a.kptr[r];
                khi = a.kptr[r + 1];
                if (klo < khi) {
                    fbeg = qr_lower_bound(a.kkeys, klo, khi, (int64_t)u * n, lane);
                    fend = qr_lower_bound(a.kkeys, fbeg, khi, (int64_t)(u + 1) * n, lane);
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
                if (MODE == QR_TABLE) ts = s1u + s2r[tn];
                else ts = qr_dot<MODE>(Z + (int64_t)tn * zstride, as, aq, dim);
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
                for (int c0 = 0; c0 < n; c0 += QR_WIN) {
                    const int c1 = c0 + QR_WIN < n ? c0 + QR_WIN : n;
                    if (fwd) {
                        // the query's known partners in [c0, c1) as bits; the cursor kc passes every partner below c1
                        wave_sync();                                   // the previous window's bits have been read
                        km[lane] = 0u;
                        wave_sync();
                        for (;;) {
                            const int64_t idx = kc + lane;
                            const int64_t x = idx < fend ? a.kkeys[idx] - (int64_t)u * n : (int64_t)WT_REL_PAD;
                            const bool below = x < c1;
                            if (below && x >= c0) atomicOr(&km[(int)(x - c0) >> 5], 1u << ((int)(x - c0) & 31));
                            const int nb = __popcll(__ballot(below));
                            kc += nb;
                            if (nb < TIPK_WAVE) break;
                        }
                        wave_sync();
                    }
                    for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                        const int c = g0 + lane;
                        bool cand = c < c1 && c != u;
                        if (cand && fwd) {
                            const int bit = c - c0;
                            cand = !((km[bit >> 5] >> (bit & 31)) & 1u);
                        }
                        float s = NAN;                                 // NaN beats nothing
                        if (cand) {
                            if (MODE == QR_TABLE) s = s1u + s2r[c];
                            else s = qr_dot<MODE>(Z + (int64_t)c * zstride, as, aq, dim);
                            if (rev && better(s, c, ws, wt) && qr_key_in(a.kkeys, klo, khi, (int64_t)c * n + u)) s = NAN;
                        }
                        for (int j = 0; j < nt; ++j) {
                            const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ts), j));
                            const int tj = __builtin_amdgcn_readlane(tn, j);
                            const int beat = __popcll(__ballot(better(s, c, sj, tj)));
                            cnt += lane == j ? beat : 0;
                        }
                    }
                }
            }
            if (lane < nt) {
                const bool ranked = tok && ts == ts;
                a.out_rank[ch + lane] = ranked ? 1 + cnt : 0;
                if (a.out_logit) a.out_logit[ch + lane] = ranked ? ts : NAN;
            }
        }
    }
}

int64_t qr_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)QR_NW * dim * 4) + (int64_t)QR_NW * (QR_WIN / 32) * 4;
}

bool qr_fits_lds(int64_t n_nodes, int dim) {
    return n_nodes * wt_stride(dim) * 4 + qr_fixed_bytes(dim, false) <= QR_LDS_BYTES;
}

int qr_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* q_rel, const int32_t* q_drug, int64_t n_q,
                   const int64_t* tgt_ptr, const int32_t* tgt_node, int64_t n_tgt, const int64_t* keys, const int64_t* kptr,
                   const int32_t* out_rank) {
    if (n_q < 0 || n_tgt < 0 || n_nodes < 1 || n_rel < 1) return TIPK_EINVAL;
    if ((keys != nullptr) != (kptr != nullptr)) return TIPK_EINVAL;
    if (n_q > 0 && n_tgt > 0 && (!q_rel || !q_drug || !tgt_ptr || !tgt_node || !out_rank)) return TIPK_EINVAL;
    return TIPK_OK;
}

template <int MODE, bool GLOBAL>
int qr_launch(const PartnerRankArgs& a, int grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)partner_rank_kernel<MODE, GLOBAL>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL((partner_rank_kernel<MODE, GLOBAL>), dim3((unsigned)grid), dim3(QR_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
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
    return n_nodes >= 1 && n_nodes <= QR_NMAX && dim >= 4 && dim <= QR_DIM_MAX && dim % 4 == 0 && n_rel >= 1 &&
           n_rel <= QR_RMAX;
}

extern "C" int tipk_distmult_partner_rank_lds_route(int64_t n_nodes, int dim) {
    return n_nodes >= 1 && n_nodes <= QR_NMAX && dim >= 4 && dim <= QR_DIM_MAX && dim % 4 == 0 && qr_fits_lds(n_nodes, dim) &&
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
    const int64_t n_blocks = (n_q + QR_NW - 1) / QR_NW;
    const int64_t most = wt_cu_count();                                // one workgroup of 16 waves per CU
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    hipStream_t st = (hipStream_t)stream;
    if (lds_route)
        return dim == 16 ? qr_launch<QR_DISTMULT16, false>(a, grid, lds, st) : qr_launch<QR_DISTMULT, false>(a, grid, lds, st);
    return dim == 16 ? qr_launch<QR_DISTMULT16, true>(a, grid, lds, st) : qr_launch<QR_DISTMULT, true>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_partner_rank_supported(int64_t n_nodes, int64_t n_rel) {
    return n_nodes >= 1 && n_nodes <= QR_NMAX && n_rel >= 1 && n_rel <= QR_RMAX;
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
    const int64_t n_blocks = (n_q + QR_NW - 1) / QR_NW;
    const int64_t most = 2 * (int64_t)wt_cu_count();                   // 4 KB of LDS each: two workgroups share a CU
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    return qr_launch<QR_TABLE, false>(a, grid, (size_t)qr_fixed_bytes(0, true), (hipStream_t)stream);
}
