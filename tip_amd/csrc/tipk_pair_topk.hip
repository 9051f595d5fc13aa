// Pair top-k: the k best relations of every pair of a list, known ones dropped (include/tipk.h section 4d).
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 pairs, ONE WAVEFRONT PER PAIR.
// Scoring.  DistMult: the wave leaves h = z[u] * z[v] (rounded once) in its LDS row; lane l scores relations l, l + 64, ...
//   as acc = fmaf(h[k], w[r][k], acc), k ascending, from an LDS image of rel_w whose row stride S has S / 4 odd, so the 16
//   lanes of a ds_read_b128 group start on 16 different groups of 4 banks.  LDS route: all of rel_w is staged once per
//   workgroup and the waves never meet again.  Streamed route (rel_w does not fit, or option "pair_topk_stream"): rel_w
//   passes through LDS in tiles, each read once per block of 16 pairs, with two workgroup barriers per tile.  Both routes
//   run the same arithmetic in the same order: same bits.  Table variant: lane l adds s1[u][r] + s2[v][r] straight from
//   the two (coalesced) table rows; no staging, no barrier.
// Known filter.  One 64-ary search per pair (the 64 lanes probe 64 keys at a time) finds the pair's block of known_rel.
//   The block is merged into a 2 048-bit LDS bitmap of the wave, one window of relations at a time, by a cursor that only
//   moves forward (the ids ascend); a candidate that passes the threshold tests one bit.
// Selection.  A candidate not below the running threshold (the k-th best kept so far) and not known is appended to the
//   wave's LDS buffer by ballot; when the buffer reaches max(64, 2k) entries (at most 192 of 256) the wave sorts it (bitonic,
//   logit desc, relation asc) and keeps k, which raises the threshold.  Dropping a candidate below the threshold is exact:
//   k kept entries are better.  The result is a set fixed by the total order, whatever the order of the appends.
#include "tipk_wave_topk.h"

namespace {

constexpr int PT_NT = 1024;                 // threads per workgroup
constexpr int PT_NW = PT_NT / TIPK_WAVE;    // pairs per block (one per wavefront)
constexpr int PT_CAP = 256;                 // buffer entries per wave
constexpr int PT_KMAX = 128;
constexpr int PT_DIM_MAX = 256;
constexpr int64_t PT_NMAX = 46340;
constexpr int64_t PT_RMAX = 65536;
constexpr int PT_WIN = 2048;                // relations per bitmap window (64 words: lane l clears word l)
constexpr int PT_LDS_BYTES = 152 * 1024;    // dynamic LDS a workgroup may ask for
constexpr int PT_TILE_BYTES = 48 * 1024;    // rel_w tile of the streamed route (at least 64 rows)
constexpr int PT_REL_PAD = WT_REL_PAD;

enum { PT_DISTMULT = 0, PT_DISTMULT16 = 1, PT_TABLE = 2 };

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

// rows [t0, t0 + rows) of rel_w into the LDS image (row stride a.stride floats), the whole workgroup
__device__ __forceinline__ void stage_rows(const PairTopkArgs& a, float* Ws, int t0, int rows) {
    const int q4 = a.dim >> 2;
    for (int idx = threadIdx.x; idx < rows * q4; idx += PT_NT) {
        const int row = idx / q4, q = idx - row * q4;
        tipk_st4(Ws + row * a.stride + 4 * q, tipk_ld4(a.b + (int64_t)(t0 + row) * a.dim + 4 * q));
    }
}

template <int MODE, bool STREAM>
__global__ void __launch_bounds__(PT_NT) pair_topk_kernel(PairTopkArgs a) {
    extern __shared__ __align__(16) unsigned char pt_smem[];
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
    const int k = a.k, R = a.n_rel, dim = a.dim;
    const int flush_at = k > 32 ? (2 * k < PT_CAP - 64 ? 2 * k : PT_CAP - 64) : 64;   // k < flush_at <= 192

    // LDS: [rel_w image] [h rows] | score buffers | relation buffers | bitmaps
    float* Ws = reinterpret_cast<float*>(pt_smem);
    float* hs_all = Ws + (MODE == PT_TABLE ? 0 : a.tile * a.stride);
    float* bs_all = hs_all + (MODE == PT_TABLE ? 0 : PT_NW * dim);
    int* br_all = reinterpret_cast<int*>(bs_all + PT_NW * PT_CAP);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(br_all + PT_NW * PT_CAP);
    float* hs = hs_all + wave * dim;
    float* bs = bs_all + wave * PT_CAP;
    int* br = br_all + wave * PT_CAP;
    uint32_t* km = km_all + wave * (PT_WIN / 32);

    if (MODE != PT_TABLE && !STREAM) {
        stage_rows(a, Ws, 0, R);
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_pairs + PT_NW - 1) / PT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t p = blk * PT_NW + wave;
        int u = -1, v = -1;
        if (p < a.n_pairs) { u = a.pu[p]; v = a.pv[p]; }
        const bool act = u >= 0 && u < a.n && v >= 0 && v < a.n;       // uniform in the wave
        int64_t kc = 0, kend = 0;
        bool filt = false;
        float4 hq[MODE == PT_DISTMULT16 ? 4 : 1];
        wave_sync();                                                   // the previous pair's buffer has been written out
        if (act) {
            if (MODE != PT_TABLE) {
                const float* zu = a.a + (int64_t)u * dim;
                const float* zv = a.a + (int64_t)v * dim;
                for (int kk = lane; kk < dim; kk += TIPK_WAVE) hs[kk] = zu[kk] * zv[kk];
                wave_sync();
                if (MODE == PT_DISTMULT16) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const float4*>(hs + 4 * q);
                }
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
            if (MODE != PT_TABLE && STREAM) {
                __syncthreads();                                       // every wave has finished with the previous tile
                stage_rows(a, Ws, t0, rows);
                __syncthreads();
            }
            if (!act) continue;
            for (int c0 = t0; c0 < t0 + rows; c0 += PT_WIN) {
                const int c1 = c0 + PT_WIN < t0 + rows ? c0 + PT_WIN : t0 + rows;
                if (filt) {
                    // the known relations of [c0, c1) as bits; the cursor kc passes every id below c1
                    km[lane] = 0u;
                    wave_sync();
                    for (;;) {
                        const int64_t idx = kc + lane;
                        const int x = idx < kend ? a.krel[idx] : PT_REL_PAD;
                        const bool below = x < c1;
                        if (below && x >= c0) atomicOr(&km[(x - c0) >> 5], 1u << ((x - c0) & 31));
                        const int nb = __popcll(__ballot(below));
                        kc += nb;
                        if (nb < TIPK_WAVE) break;
                    }
                    wave_sync();
                }
                for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                    const int r = g0 + lane;
                    const bool valid = r < c1;
                    float s = 0.f;
                    if (valid) {
                        if (MODE == PT_TABLE) {
                            s = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                        } else if (MODE == PT_DISTMULT16) {
                            const float* wr = Ws + (r - t0) * a.stride;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float4 w4 = *reinterpret_cast<const float4*>(wr + 4 * q);
                                s = fmaf(hq[q].x, w4.x, s);
                                s = fmaf(hq[q].y, w4.y, s);
                                s = fmaf(hq[q].z, w4.z, s);
                                s = fmaf(hq[q].w, w4.w, s);
                            }
                        } else {
                            const float* wr = Ws + (r - t0) * a.stride;
                            for (int k0 = 0; k0 < dim; k0 += 4) {
                                const float4 w4 = *reinterpret_cast<const float4*>(wr + k0);
                                const float4 h4 = *reinterpret_cast<const float4*>(hs + k0);
                                s = fmaf(h4.x, w4.x, s);
                                s = fmaf(h4.y, w4.y, s);
                                s = fmaf(h4.z, w4.z, s);
                                s = fmaf(h4.w, w4.w, s);
                            }
                        }
                    }
                    bool pass = valid && s >= thr;
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

int pt_stride(int dim) { return wt_stride(dim); }

int64_t pt_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)PT_NW * dim * 4) + (int64_t)PT_NW * PT_CAP * 8 + (int64_t)PT_NW * (PT_WIN / 32) * 4;
}

bool pt_fits_lds(int dim, int64_t n_rel) {
    return n_rel * pt_stride(dim) * 4 + pt_fixed_bytes(dim, false) <= PT_LDS_BYTES;
}

int pt_stream_tile(int dim) {
    const int rows = PT_TILE_BYTES / (pt_stride(dim) * 4) / TIPK_WAVE * TIPK_WAVE;
    return rows < TIPK_WAVE ? TIPK_WAVE : rows;
}

int pt_cu_count() { return wt_cu_count(); }

int pt_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                   const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int k,
                   const float* out_score, const int32_t* out_rel) {
    if (k <= 0 || n_pairs < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    const int given = (keys != nullptr) + (kptr != nullptr) + (krel != nullptr);
    if (given != 0 && given != 3) return TIPK_EINVAL;
    if (n_pairs > 0 && (!pair_u || !pair_v || !out_score || !out_rel)) return TIPK_EINVAL;
    return TIPK_OK;
}

template <int MODE, bool STREAM>
int pt_launch(const PairTopkArgs& a, int grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)pair_topk_kernel<MODE, STREAM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL((pair_topk_kernel<MODE, STREAM>), dim3((unsigned)grid), dim3(PT_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_distmult_pair_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return n_nodes >= 1 && n_nodes <= PT_NMAX && dim >= 4 && dim <= PT_DIM_MAX && dim % 4 == 0 && n_rel >= 1 &&
           n_rel <= PT_RMAX && k >= 1 && k <= PT_KMAX;
}

extern "C" int64_t tipk_distmult_pair_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_pairs, int k) {
    if (n_pairs < 0 || !tipk_distmult_pair_topk_supported(n_nodes, dim, n_rel, k)) return -1;
    return 0;                                                          // every list lives in LDS
}

extern "C" int tipk_distmult_pair_topk_lds_route(int dim, int64_t n_rel) {
    return dim >= 4 && dim <= PT_DIM_MAX && dim % 4 == 0 && n_rel >= 1 && n_rel <= PT_RMAX && pt_fits_lds(dim, n_rel) &&
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
    a.a = z; a.b = rel_w; a.pu = pair_u; a.pv = pair_v;
    a.kkeys = n_known_pairs > 0 ? known_pair_keys : nullptr; a.kptr = known_pair_ptr; a.krel = known_rel;
    a.n_known = n_known_pairs; a.n_pairs = n_pairs; a.ld = 0;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel; a.k = k; a.stride = pt_stride(dim);
    a.out_s = out_score; a.out_r = out_rel;
    const bool lds_route = tipk_distmult_pair_topk_lds_route(dim, n_rel) != 0;
    a.tile = lds_route ? (int)n_rel : pt_stream_tile(dim);
    const size_t lds = (size_t)a.tile * a.stride * 4 + (size_t)pt_fixed_bytes(dim, false);
    const int64_t n_blocks = (n_pairs + PT_NW - 1) / PT_NW;
    const int n_cu = pt_cu_count();                                    // the LDS image allows one workgroup per CU
    const int grid = (int)(n_blocks < n_cu ? n_blocks : n_cu);
    hipStream_t st = (hipStream_t)stream;
    if (lds_route)
        return dim == 16 ? pt_launch<PT_DISTMULT16, false>(a, grid, lds, st) : pt_launch<PT_DISTMULT, false>(a, grid, lds, st);
    return dim == 16 ? pt_launch<PT_DISTMULT16, true>(a, grid, lds, st) : pt_launch<PT_DISTMULT, true>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_pair_topk_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return n_nodes >= 1 && n_nodes <= PT_NMAX && n_rel >= 1 && n_rel <= PT_RMAX && k >= 1 && k <= PT_KMAX;
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
    a.a = s1; a.b = s2; a.pu = pair_u; a.pv = pair_v;
    a.kkeys = n_known_pairs > 0 ? known_pair_keys : nullptr; a.kptr = known_pair_ptr; a.krel = known_rel;
    a.n_known = n_known_pairs; a.n_pairs = n_pairs; a.ld = ld;
    a.n = (int)n_nodes; a.dim = 0; a.n_rel = (int)n_rel; a.k = k; a.stride = 0; a.tile = (int)n_rel;
    a.out_s = out_score; a.out_r = out_rel;
    const int64_t n_blocks = (n_pairs + PT_NW - 1) / PT_NW;
    const int64_t most = 2 * (int64_t)pt_cu_count();                   // 36 KB of LDS each: two workgroups share a CU
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    return pt_launch<PT_TABLE, false>(a, grid, (size_t)pt_fixed_bytes(0, true), (hipStream_t)stream);
}
