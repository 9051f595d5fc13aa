// Regimen top-k: the k best relations of every drug list, aggregated over the list's pairs, with the pair that drives each
// (include/tipk.h section 4e).
//
// One launch of persistent workgroups (16 wavefronts); a workgroup takes blocks of 16 regimens, ONE WAVEFRONT PER REGIMEN.
// Lane l keeps the regimen's l-th drug id (a regimen has at most 64 entries), so a pair's ids are two lane reads.
// Windows.  The relation axis is walked in windows of 64 x RG_A relations: lane l owns relations c0 + l, c0 + l + 64, ...
//   with RG_A aggregate / best-logit / best-pair registers.  Per window the wave loops over the regimen's pairs in pair
//   order; per pair it scores its RG_A relations exactly as 4d does (h = z[u] * z[v] rounded once into the wave's LDS row,
//   then fmaf over k ascending; table variant: one add of the two coalesced table rows) and updates the registers unless
//   the triple is known or its logit is NaN.  The noisy-or sum therefore runs in pair order, in fp32, per relation.
// rel_w.  An LDS image with 4d's bank-spreading stride, staged once per workgroup, when it fits beside the waves' state;
//   otherwise (or under option "regimen_global") each lane reads its rows from global memory.  Same arithmetic, same bits.
// Known filter.  One 64-ary search per pair finds the pair's block of known_rel; its position is kept in LDS for the first
//   RG_ATC pairs of the regimen so that later windows do not search again.  A 64-ary lower bound inside the block gives
//   the window's start; the window's known ids become bits of a per-wave LDS bitmap that every scoring step tests.
// Selection.  After the last pair of a window, 4d's selection: a candidate not below the running threshold is appended to
//   the wave's LDS buffer by ballot, the buffer is cut to k by a bitonic sort (aggregate desc, relation asc) when it
//   reaches max(64, 2k) entries.  The driver pair travels with its entry as a 16-bit tag (i | j << 8).
#include "tipk_wave_topk.h"

namespace {

constexpr int RG_NT = 1024;                 // threads per workgroup
constexpr int RG_NW = RG_NT / TIPK_WAVE;    // regimens per block (one per wavefront)
constexpr int RG_CAP = 256;                 // buffer entries per wave
constexpr int RG_KMAX = 128;
constexpr int RG_DIM_MAX = 256;
constexpr int64_t RG_NMAX = 46340;
constexpr int64_t RG_RMAX = 65536;
constexpr int RG_M_MAX = TIPK_WAVE;         // drugs per regimen: one lane each
constexpr int RG_A = 4;                     // relations per lane and window
constexpr int RG_WIN = TIPK_WAVE * RG_A;    // relations per window
constexpr int RG_ATC = 256;                 // pairs per regimen whose known-block position is kept in LDS
constexpr int RG_LDS_BYTES = 152 * 1024;    // dynamic LDS a workgroup may ask for

enum { RG_DISTMULT = 0, RG_DISTMULT16 = 1, RG_TABLE = 2 };

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

// first index in [lo, hi) whose ascending a[] is >= x (hi if none): uniform arguments, uniform answer, 64 probes per step
__device__ int64_t lower_bound_rel(const int32_t* a, int64_t lo, int64_t hi, int x, int lane) {
    while (hi - lo > TIPK_WAVE) {
        const int64_t step = (hi - lo + TIPK_WAVE - 1) / TIPK_WAVE;
        const int64_t idx = lo + (int64_t)lane * step;
        const int c = __popcll(__ballot(idx < hi && a[idx] < x));   // the probes ascend: the lanes below x are a prefix
        if (c == 0) return lo;
        const int64_t top = lo + (int64_t)c * step;
        lo += (int64_t)(c - 1) * step + 1;                           // a[lo - 1] < x <= a[top] (or top is past the end)
        hi = top < hi ? top : hi;
    }
    const int64_t idx = lo + lane;
    return lo + __popcll(__ballot(idx < hi && a[idx] < x));
}

__device__ __forceinline__ float softplus(float s) { return fmaxf(s, 0.f) + log1pf(expf(-fabsf(s))); }

template <int MODE, bool IMAGE>
__global__ void __launch_bounds__(RG_NT) regimen_topk_kernel(RegimenArgs a) {
    extern __shared__ __align__(16) unsigned char rg_smem[];
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
    const int k = a.k, R = a.n_rel, dim = a.dim;
    const int flush_at = k > 32 ? (2 * k < RG_CAP - 64 ? 2 * k : RG_CAP - 64) : 64;   // k < flush_at <= 192

    // LDS: [rel_w image] [h rows] | aggregate buffers | relation buffers | known-block positions | bitmaps | pair tags
    float* Ws = reinterpret_cast<float*>(rg_smem);
    float* hs_all = Ws + (IMAGE ? R * a.stride : 0);
    float* bs_all = hs_all + (MODE == RG_TABLE ? 0 : RG_NW * dim);
    int* br_all = reinterpret_cast<int*>(bs_all + RG_NW * RG_CAP);
    int* atc_all = br_all + RG_NW * RG_CAP;
    uint32_t* km_all = reinterpret_cast<uint32_t*>(atc_all + RG_NW * RG_ATC);
    uint16_t* bt_all = reinterpret_cast<uint16_t*>(km_all + RG_NW * (RG_WIN / 32));
    float* hs = hs_all + wave * dim;
    float* bs = bs_all + wave * RG_CAP;
    int* br = br_all + wave * RG_CAP;
    int* atc = atc_all + wave * RG_ATC;
    uint32_t* km = km_all + wave * (RG_WIN / 32);
    uint16_t* bt = bt_all + wave * RG_CAP;

    if (IMAGE) {
        const int q4 = dim >> 2;
        for (int idx = t; idx < R * q4; idx += RG_NT) {
            const int row = idx / q4, q = idx - row * q4;
            tipk_st4(Ws + row * a.stride + 4 * q, tipk_ld4(a.b + (int64_t)row * dim + 4 * q));
        }
        __syncthreads();
    }

    const int64_t n_blocks = (a.n_reg + RG_NW - 1) / RG_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t g = blk * RG_NW + wave;
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
                    float4 hq[MODE == RG_DISTMULT16 ? 4 : 1];
                    wave_sync();                                       // the previous pair is done with hs and km
                    if (MODE != RG_TABLE) {
                        const float* zu = a.a + (int64_t)u * dim;
                        const float* zv = a.a + (int64_t)v * dim;
                        for (int kk = lane; kk < dim; kk += TIPK_WAVE) hs[kk] = zu[kk] * zv[kk];
                    }
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
                            if (c0 > 0) kc = lower_bound_rel(a.krel, kc, kend, c0, lane);
                            const int first = kc < kend ? a.krel[kc] : WT_REL_PAD;
                            if (first < c1) {
                                // the known relations of [c0, c1) as bits
                                filt = true;
                                if (lane < RG_WIN / 32) km[lane] = 0u;
                                wave_sync();
                                for (;;) {
                                    const int64_t idx = kc + lane;
                                    const int x = idx < kend ? a.krel[idx] : WT_REL_PAD;
                                    const bool below = x < c1;
                                    if (below && x >= c0) atomicOr(&km[(x - c0) >> 5], 1u << ((x - c0) & 31));
                                    const int nb = __popcll(__ballot(below));
                                    kc += nb;
                                    if (nb < TIPK_WAVE) break;
                                }
                            }
                        }
                    }
                    wave_sync();
                    if (MODE == RG_DISTMULT16) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const float4*>(hs + 4 * q);
                    }
                    const int tag = i | (j << 8);
#pragma unroll
                    for (int x = 0; x < RG_A; ++x) {
                        const int r = c0 + x * TIPK_WAVE + lane;
                        if (c0 + x * TIPK_WAVE >= c1) break;           // uniform
                        if (r >= c1) continue;
                        float s = 0.f;
                        if (MODE == RG_TABLE) {
                            s = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                        } else if (MODE == RG_DISTMULT16) {
                            const float* wr = IMAGE ? Ws + r * a.stride : a.b + (int64_t)r * 16;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float4 w4 = *reinterpret_cast<const float4*>(wr + 4 * q);
                                s = fmaf(hq[q].x, w4.x, s);
                                s = fmaf(hq[q].y, w4.y, s);
                                s = fmaf(hq[q].z, w4.z, s);
                                s = fmaf(hq[q].w, w4.w, s);
                            }
                        } else {
                            const float* wr = IMAGE ? Ws + r * a.stride : a.b + (int64_t)r * dim;
                            for (int k0 = 0; k0 < dim; k0 += 4) {
                                const float4 w4 = *reinterpret_cast<const float4*>(wr + k0);
                                const float4 h4 = *reinterpret_cast<const float4*>(hs + k0);
                                s = fmaf(h4.x, w4.x, s);
                                s = fmaf(h4.y, w4.y, s);
                                s = fmaf(h4.z, w4.z, s);
                                s = fmaf(h4.w, w4.w, s);
                            }
                        }
                        bool take = s == s;                            // a NaN logit contributes nothing
                        if (take && filt) {
                            const int bit = r - c0;
                            take = !((km[bit >> 5] >> (bit & 31)) & 1u);
                        }
                        if (take) {
                            if (bpr[x] < 0 || s > best[x]) { best[x] = s; bpr[x] = tag; }   // ties: the first in pair order
                            if (a.noisy) agg[x] += softplus(s);
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
    return (table ? 0 : (int64_t)RG_NW * dim * 4) + (int64_t)RG_NW * RG_CAP * 10 + (int64_t)RG_NW * RG_ATC * 4 +
           (int64_t)RG_NW * (RG_WIN / 32) * 4;
}

bool rg_fits_lds(int dim, int64_t n_rel) {
    return n_rel * wt_stride(dim) * 4 + rg_fixed_bytes(dim, false) <= RG_LDS_BYTES;
}

int rg_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* reg_drugs, const int64_t* reg_ptr, int64_t n_regimens,
                   const int64_t* keys, const int64_t* kptr, const int32_t* krel, int64_t n_known, int aggregate, int k,
                   const float* out_score, const int32_t* out_rel, const int32_t* out_pair) {
    if (k <= 0 || n_regimens < 0 || n_nodes < 1 || n_rel < 1 || n_known < 0) return TIPK_EINVAL;
    if (aggregate != TIPK_REGIMEN_MAX && aggregate != TIPK_REGIMEN_NOISY_OR) return TIPK_EINVAL;
    const int given = (keys != nullptr) + (kptr != nullptr) + (krel != nullptr);
    if (given != 0 && given != 3) return TIPK_EINVAL;
    if (n_regimens > 0 && (!reg_drugs || !reg_ptr || !out_score || !out_rel || !out_pair)) return TIPK_EINVAL;
    return TIPK_OK;
}

template <int MODE, bool IMAGE>
int rg_launch(const RegimenArgs& a, int grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)regimen_topk_kernel<MODE, IMAGE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL((regimen_topk_kernel<MODE, IMAGE>), dim3((unsigned)grid), dim3(RG_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_regimen_max_drugs(void) { return RG_M_MAX; }

extern "C" int tipk_distmult_regimen_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return n_nodes >= 1 && n_nodes <= RG_NMAX && dim >= 4 && dim <= RG_DIM_MAX && dim % 4 == 0 && n_rel >= 1 &&
           n_rel <= RG_RMAX && k >= 1 && k <= RG_KMAX;
}

extern "C" int64_t tipk_distmult_regimen_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_regimens,
                                                              int k) {
    if (n_regimens < 0 || !tipk_distmult_regimen_topk_supported(n_nodes, dim, n_rel, k)) return -1;
    return 0;                                                          // every list lives in LDS
}

extern "C" int tipk_distmult_regimen_topk_lds_route(int dim, int64_t n_rel) {
    return dim >= 4 && dim <= RG_DIM_MAX && dim % 4 == 0 && n_rel >= 1 && n_rel <= RG_RMAX && rg_fits_lds(dim, n_rel) &&
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
    a.a = z; a.b = rel_w; a.drugs = reg_drugs; a.ptr = reg_ptr;
    a.kkeys = n_known_pairs > 0 ? known_pair_keys : nullptr; a.kptr = known_pair_ptr; a.krel = known_rel;
    a.n_known = n_known_pairs; a.n_reg = n_regimens; a.ld = 0;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel; a.k = k; a.stride = wt_stride(dim);
    a.noisy = aggregate == TIPK_REGIMEN_NOISY_OR;
    a.out_s = out_score; a.out_r = out_rel; a.out_p = out_pair;
    const bool image = tipk_distmult_regimen_topk_lds_route(dim, n_rel) != 0;
    const size_t lds = (image ? (size_t)n_rel * a.stride * 4 : 0) + (size_t)rg_fixed_bytes(dim, false);
    const int64_t n_blocks = (n_regimens + RG_NW - 1) / RG_NW;
    const int64_t most = (image ? 1 : 2) * (int64_t)wt_cu_count();     // the image allows one workgroup per CU
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    hipStream_t st = (hipStream_t)stream;
    if (image)
        return dim == 16 ? rg_launch<RG_DISTMULT16, true>(a, grid, lds, st) : rg_launch<RG_DISTMULT, true>(a, grid, lds, st);
    return dim == 16 ? rg_launch<RG_DISTMULT16, false>(a, grid, lds, st) : rg_launch<RG_DISTMULT, false>(a, grid, lds, st);
}

extern "C" int tipk_pair_table_regimen_topk_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return n_nodes >= 1 && n_nodes <= RG_NMAX && n_rel >= 1 && n_rel <= RG_RMAX && k >= 1 && k <= RG_KMAX;
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
    a.a = s1; a.b = s2; a.drugs = reg_drugs; a.ptr = reg_ptr;
    a.kkeys = n_known_pairs > 0 ? known_pair_keys : nullptr; a.kptr = known_pair_ptr; a.krel = known_rel;
    a.n_known = n_known_pairs; a.n_reg = n_regimens; a.ld = ld;
    a.n = (int)n_nodes; a.dim = 0; a.n_rel = (int)n_rel; a.k = k; a.stride = 0;
    a.noisy = aggregate == TIPK_REGIMEN_NOISY_OR;
    a.out_s = out_score; a.out_r = out_rel; a.out_p = out_pair;
    const int64_t n_blocks = (n_regimens + RG_NW - 1) / RG_NW;
    const int64_t most = 2 * (int64_t)wt_cu_count();
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    return rg_launch<RG_TABLE, false>(a, grid, (size_t)rg_fixed_bytes(0, true), (hipStream_t)stream);
}
