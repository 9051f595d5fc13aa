// Pair top-k: the k best relations of every pair of a list, known ones dropped (include/tipk.h section 4d).
// The pieces it shares with the other wave-per-row kernels (the logit, the known bitmap, the bitonic cut) are in
// tipk_wave_topk.h; this file holds the pair loop and the streamed route.
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 pairs, ONE WAVEFRONT PER PAIR.
// Scoring.  DistMult: the wave leaves h = z[u] * z[v] (rounded once) in its LDS row; lane l scores relations l, l + 64, ...
//   with the shared fma chain from an LDS image of rel_w.  LDS route: all of rel_w is staged once per workgroup and the
//   waves never meet again.  Streamed route (rel_w does not fit, or option "pair_topk_stream"): rel_w passes through LDS
//   in tiles, each read once per block of 16 pairs, with two workgroup barriers per tile.  Both routes run the same
//   arithmetic in the same order: same bits.  Table variant: lane l adds s1[u][r] + s2[v][r] straight from the two
//   (coalesced) table rows; no staging, no barrier.
// Known filter.  One 64-ary search per pair finds the pair's block of known_rel.  The block is merged into a 2 048-bit LDS
//   bitmap of the wave, one window of relations at a time, by a cursor that only moves forward (the ids ascend); a
//   candidate that passes the threshold tests one bit.
// Selection.  A candidate not below the running threshold (the k-th best kept so far) and not known is appended to the
//   wave's LDS buffer; the buffer is cut to k (bitonic, logit desc, relation asc) when it fills, which raises the
//   threshold.  The result is a set fixed by the total order, whatever the order of the appends.
#include "tipk_wave_topk.h"

namespace {

constexpr int PT_TILE_BYTES = 48 * 1024;    // rel_w tile of the streamed route (at least 64 rows)

struct PairTopkArgs {
    const float* a;            // z [n x dim]            | s1 [n x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2 [n x ld]
    const int32_t* pu;
    const int32_t* pv;
    const int64_t* kkeys;      // nullable with kptr, krel
    const int64_t* kptr;
    const int32_t* krel;
    int64_t n_known, n_pairs, ld;
    int n, dim, n_rel, k, stride, tile;
    float* out_s;
    int32_t* out_r;
};

template <int MODE, bool STREAM>
__global__ void __launch_bounds__(WT_NT) pair_topk_kernel(PairTopkArgs a) {
    extern __shared__ __align__(16) unsigned char pt_smem[];
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
    const int k = a.k, R = a.n_rel, dim = a.dim;
    const int flush_at = wt_flush_at(k);

    // LDS: [rel_w image] [h rows] | score buffers | relation buffers | bitmaps
    float* Ws = reinterpret_cast<float*>(pt_smem);
    float* hs_all = Ws + (MODE == WT_TABLE ? 0 : a.tile * a.stride);
    float* bs_all = hs_all + (MODE == WT_TABLE ? 0 : WT_NW * dim);
    int* br_all = reinterpret_cast<int*>(bs_all + WT_NW * WT_CAP);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(br_all + WT_NW * WT_CAP);
    float* hs = hs_all + wave * dim;
    float* bs = bs_all + wave * WT_CAP;
    int* br = br_all + wave * WT_CAP;
    uint32_t* km = km_all + wave * (WT_WIN / 32);

    if (MODE != WT_TABLE && !STREAM) {
        wt_stage_rows<WT_NT>(Ws, a.b, 0, R, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_pairs + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t p = blk * WT_NW + wave;
        int u = -1, v = -1;
        if (p < a.n_pairs) { u = a.pu[p]; v = a.pv[p]; }
        const bool act = u >= 0 && u < a.n && v >= 0 && v < a.n;       // uniform in the wave
        int64_t kc = 0, kend = 0;
        bool filt = false;
        float4 hq[MODE == WT_DISTMULT16 ? 4 : 1];
        wave_sync();                                                   // the previous pair's buffer has been written out
        if (act) {
            if (MODE != WT_TABLE) {
                wt_write_row(hs, a.a + (int64_t)u * dim, a.a + (int64_t)v * dim, dim, lane);
                wave_sync();
                wt_row16<MODE>(hq, hs);
            }
            if (a.kkeys) {
                const int lo = u < v ? u : v, hi = u < v ? v : u;
                const int64_t at = find_key(a.kkeys, a.n_known, (int64_t)lo * a.n + hi, lane);
                if (at >= 0) { kc = a.kptr[at]; kend = a.kptr[at + 1]; }
                filt = kc < kend;
            }
        }
        int c = 0;
        float thr = -INFINITY;

        for (int t0 = 0; t0 < R; t0 += a.tile) {
            const int rows = R - t0 < a.tile ? R - t0 : a.tile;
            if (MODE != WT_TABLE && STREAM) {
                __syncthreads();                                       // every wave has finished with the previous tile
                wt_stage_rows<WT_NT>(Ws, a.b, t0, rows, dim, a.stride);
                __syncthreads();
            }
            if (!act) continue;
            for (int c0 = t0; c0 < t0 + rows; c0 += WT_WIN) {
                const int c1 = c0 + WT_WIN < t0 + rows ? c0 + WT_WIN : t0 + rows;
                if (filt) {
                    // no fence in front of the clear: the previous window's bit tests and the clear are accesses of one
                    // wave to the same words, in program order
                    wt_merge_window<WT_WIN / 32>(km, kc, kend, c0, c1, lane, [&](int64_t idx) { return a.krel[idx]; });
                    wave_sync();
                }
                for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                    const int r = g0 + lane;
                    const bool valid = r < c1;
                    float s = 0.f;
                    if (valid) {
                        if (MODE == WT_TABLE) s = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                        else s = wt_dot<MODE>(Ws + (r - t0) * a.stride, hs, hq, dim);
                    }
                    bool pass = valid && s >= thr;
                    // the bit test, the append and the write-out below are written out here and in the regimen top-k: as
                    // shared helpers they measured 1 % slower on the table variants (profiles/wave_rows_refactor.md)
                    if (pass && filt) {
                        const int bit = r - c0;
                        pass = !((km[bit >> 5] >> (bit & 31)) & 1u);
                    }
                    const unsigned long long mask = __ballot(pass);
                    if (mask == 0ull) continue;
                    if (pass) {
                        const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                        bs[pos] = s;
                        br[pos] = r;
                    }
                    c += __popcll(mask);
                    if (c >= flush_at) flush<false>(bs, br, nullptr, c, thr, k, lane);
                }
            }
        }

        if (p < a.n_pairs) {
            if (c > 0) flush<false>(bs, br, nullptr, c, thr, k, lane);
            float* os = a.out_s + p * k;
            int32_t* orl = a.out_r + p * k;
            for (int i = lane; i < k; i += TIPK_WAVE) {
                const bool have = i < c;
                os[i] = have ? bs[i] : -INFINITY;
                orl[i] = have ? br[i] : -1;
            }
        }
    }
}

int64_t pt_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * dim * 4) + (int64_t)WT_NW * WT_CAP * 8 + (int64_t)WT_NW * (WT_WIN / 32) * 4;
}

int pt_stream_tile(int dim) {
    const int rows = PT_TILE_BYTES / (wt_stride(dim) * 4) / TIPK_WAVE * TIPK_WAVE;
    return rows < TIPK_WAVE ? TIPK_WAVE : rows;
}

int pt_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                   const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int k,
                   const float* out_score, const int32_t* out_rel) {
    if (k <= 0 || n_pairs < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    if (!wt_known_ok(keys, kptr, krel)) return TIPK_EINVAL;
    if (n_pairs > 0 && (!pair_u || !pair_v || !out_score || !out_rel)) return TIPK_EINVAL;
    return TIPK_OK;
}

void pt_fill_lists(PairTopkArgs& a, int64_t n_nodes, int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v,
                   int64_t n_pairs, const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int k,
                   float* out_score, int32_t* out_rel) {
    a.pu = pair_u; a.pv = pair_v;
    a.kkeys = n_known > 0 ? keys : nullptr; a.kptr = kptr; a.krel = krel;
    a.n_known = n_known; a.n_pairs = n_pairs;
    a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.k = k;
    a.out_s = out_score; a.out_r = out_rel;
}

}  // namespace

extern "C" int tipk_distmult_pair_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return wt_distmult_shape(n_nodes, dim, n_rel) && k >= 1 && k <= WT_KMAX;
}

extern "C" int64_t tipk_distmult_pair_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_pairs, int k) {
    if (n_pairs < 0 || !tipk_distmult_pair_topk_supported(n_nodes, dim, n_rel, k)) return -1;
    return 0;                                                          // every list lives in LDS
}

extern "C" int tipk_distmult_pair_topk_lds_route(int dim, int64_t n_rel) {
    return wt_distmult_shape(1, dim, n_rel) && wt_fits_lds(n_rel, dim, pt_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_PAIR_TOPK_STREAM);
}

extern "C" int tipk_distmult_pair_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                       const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                                       const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                       const int32_t* known_rel, int64_t n_known_pairs, int k, float* out_score,
                                       int32_t* out_rel, void* workspace, tipk_stream_t stream) {
    (void)workspace;
    const int bad = pt_check_lists(n_nodes, n_rel, pair_u, pair_v, n_pairs, known_pair_keys, known_pair_ptr, known_rel,
                                   n_known_pairs, k, out_score, out_rel);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_pairs > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_pair_topk_supported(n_nodes, dim, n_rel, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rel_w) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_pairs == 0) return TIPK_OK;

    PairTopkArgs a;
    pt_fill_lists(a, n_nodes, n_rel, pair_u, pair_v, n_pairs, known_pair_keys, known_pair_ptr, known_rel, n_known_pairs, k,
                  out_score, out_rel);
    a.a = z; a.b = rel_w; a.ld = 0; a.dim = dim; a.stride = wt_stride(dim);
    const bool lds_route = tipk_distmult_pair_topk_lds_route(dim, n_rel) != 0;
    a.tile = lds_route ? (int)n_rel : pt_stream_tile(dim);
    const size_t lds = (size_t)a.tile * a.stride * 4 + (size_t)pt_fixed_bytes(dim, false);
    const int grid = wt_grid(n_pairs, 1);                              // the LDS image allows one workgroup per CU
    hipStream_t st = (hipStream_t)stream;
    if (lds_route)
        return dim == 16 ? wt_launch<pair_topk_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                         : wt_launch<pair_topk_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
    return dim == 16 ? wt_launch<pair_topk_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                     : wt_launch<pair_topk_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_pair_topk_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return wt_table_shape(n_nodes, n_rel) && k >= 1 && k <= WT_KMAX;
}

extern "C" int tipk_pair_table_pair_topk(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                         const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                                         const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                         const int32_t* known_rel, int64_t n_known_pairs, int k, float* out_score,
                                         int32_t* out_rel, tipk_stream_t stream) {
    const int bad = pt_check_lists(n_nodes, n_rel, pair_u, pair_v, n_pairs, known_pair_keys, known_pair_ptr, known_rel,
                                   n_known_pairs, k, out_score, out_rel);
    if (bad != TIPK_OK || ld < n_rel) return TIPK_EINVAL;
    if (n_pairs > 0 && (!s1 || !s2)) return TIPK_EINVAL;
    if (!tipk_pair_table_pair_topk_supported(n_nodes, n_rel, k)) return TIPK_EUNSUPPORTED;
    if (n_pairs == 0) return TIPK_OK;

    PairTopkArgs a;
    pt_fill_lists(a, n_nodes, n_rel, pair_u, pair_v, n_pairs, known_pair_keys, known_pair_ptr, known_rel, n_known_pairs, k,
                  out_score, out_rel);
    a.a = s1; a.b = s2; a.ld = ld; a.dim = 0; a.stride = 0; a.tile = (int)n_rel;
    const int grid = wt_grid(n_pairs, 2);                              // 36 KB of LDS each: two workgroups share a CU
    return wt_launch<pair_topk_kernel<WT_TABLE, false>>(a, grid, (size_t)pt_fixed_bytes(0, true), (hipStream_t)stream);
}
