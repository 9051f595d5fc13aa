// Partner sum: the expected number of unrecorded partners of a drug per side effect -- the marginal of the model over the
// partner axis -- and the k largest cells of every queried drug's row (include/tipk.h section 4l).
//   out_sum[q, j] = sum over candidates c of partner_w[c] * sigma(logit(r_j, u_q, c)),   out_count[q, j] = #candidates.
// The logit (fma chain of tipk_wave_topk.h, the queried drug multiplied with w first; table variant: one add), the forward
// key range, the bitmap merge and the bitonic cut are the shared pieces; this file holds the item / window / group loop,
// the register blocking over relations, the reduction over partners and the per-row selection.
//
// Launch 1, partner_sum_kernel: persistent workgroups (16 wavefronts); an ITEM is (queried drug q, block of PS_RB columns
//   of the result), ONE WAVEFRONT PER ITEM.  Lane l owns the partners c = l, l + 64, ... ascending.
//   Register blocking.  A partner's row z[c] is read ONCE (LDS image or global memory) and serves the PS_RB relations of
//   the item: dim 16 keeps the PS_RB product rows a_x = z[u] * w[r_x] in registers (4 x 16 VGPRs), so a logit costs a
//   quarter of a 64-byte LDS read and the kernel is bound by the vector ALU, not by LDS; other widths read the product rows
//   from the wave's LDS rows (a broadcast) in the same k order.
//   Known filter.  Forward keys only: per relation of the item two 64-ary searches bound the run [u*n, (u+1)*n) inside the
//   relation's block; the runs are merged into PS_RB bitmaps of the wave, one window of 2 048 drugs at a time.
//   Sum.  term = partner_w[c] * sigma(logit), sigma(s) = 1.0f / (1.0f + expf(-s)); lane l adds its terms in ascending c
//   from +0.0f, then the 64 partials are summed by the halving tree p_l += p_(l + off), off = 32, 16, ..., 1; lane 0 writes.
//   The order depends on nothing but n_nodes: the cell is BITWISE repeatable and the same on both routes.  A partner that
//   is no candidate (c == u, weight 0, recorded) is skipped, never multiplied.
// z.  An LDS image, staged once per workgroup, when it fits beside the waves' state; otherwise (or under option
//   "partner_sum_global") each lane reads its rows from global memory.  Same arithmetic, same bits.
// Launch 2 (k > 0), partner_sum_select_kernel: ONE WAVEFRONT PER QUERIED DRUG streams its row of out_sum in windows of 64
//   and keeps the k best of (value descending, column ascending) with the shared buffer cut; NaN never enters.
#include "tipk_wave_topk.h"

namespace {

constexpr int PS_RB = 4;                    // relations (columns) per item: the register block
constexpr int PS_WORDS = WT_WIN / 32;       // bitmap words per relation and window
constexpr int64_t PS_SEL_MAX = 0x7fffffff;  // columns of a call: positions are int32

struct PartnerSumArgs {
    const float* a;            // z [n x dim]            | s1t [n_rel x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2t [n_rel x ld]
    const int32_t* qdrug;      // [n_q]
    const int32_t* rel;        // [n_sel], nullable: column j is relation j
    const float* pw;           // [n], nullable: every weight is 1
    const int64_t* kkeys;      // nullable with kptr
    const int64_t* kptr;       // [n_rel + 1]
    int64_t n_q, n_sel, n_jb, ld;
    int n, dim, n_rel, stride, k;
    float* out_sum;
    int32_t* out_cnt;
    float* top_val;
    int32_t* top_pos;
};

__device__ __forceinline__ float ps_sigma(float s) { return 1.0f / (1.0f + expf(-s)); }

template <int MODE, bool GLOBAL>
__global__ void __launch_bounds__(WT_NT) partner_sum_kernel(PartnerSumArgs a) {
    extern __shared__ __align__(16) unsigned char ps_smem[];
    const int t = threadIdx.x, lane = tipk_lane();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, dim = a.dim;
    const int zstride = GLOBAL ? dim : a.stride;                       // row stride of whatever holds z

    // LDS: [z image] [product rows: PS_RB per wave] | bitmaps: PS_RB per wave
    float* Zs = reinterpret_cast<float*>(ps_smem);
    float* as_all = Zs + ((MODE == WT_TABLE || GLOBAL) ? 0 : n * a.stride);
    uint32_t* km_all = reinterpret_cast<uint32_t*>(as_all + (MODE == WT_TABLE ? 0 : WT_NW * PS_RB * dim));
    float* as = as_all + wave * PS_RB * dim;
    uint32_t* km = km_all + wave * PS_RB * PS_WORDS;
    const float* Z = GLOBAL ? a.a : Zs;

    if (MODE != WT_TABLE && !GLOBAL) {
        wt_stage_rows<WT_NT>(Zs, a.a, 0, n, dim, a.stride);
        __syncthreads();
    }

    const int64_t n_items = a.n_q * a.n_jb;
    const int64_t n_blocks = (n_items + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t item = blk * WT_NW + wave;
        if (item >= n_items) continue;                                 // uniform in the wave; the waves never meet again
        const int64_t q = item / a.n_jb, j0 = (item - q * a.n_jb) * PS_RB;
        const int u = a.qdrug[q];
        const bool uok = u >= 0 && u < n;

        int r[PS_RB];
        bool rok[PS_RB], fwd[PS_RB];
        int64_t kc[PS_RB], kend[PS_RB];                                // relation r_x's keys [u*n, (u+1)*n): cursor and end
        float4 aq[MODE == WT_DISTMULT16 ? PS_RB : 1][4];
        float s1u[PS_RB];
        bool any_fwd = false;
        if (MODE != WT_TABLE) wave_sync();                             // the previous item's reads of the product rows are done
#pragma unroll
        for (int x = 0; x < PS_RB; ++x) {
            const int64_t j = j0 + x;
            r[x] = j < a.n_sel ? (a.rel ? a.rel[j] : (int)j) : -1;
            rok[x] = uok && r[x] >= 0 && r[x] < a.n_rel;
            fwd[x] = false;
            kc[x] = kend[x] = 0;
            s1u[x] = 0.f;
            if (!rok[x]) continue;                                     // uniform
            if (MODE == WT_TABLE) s1u[x] = a.a[(int64_t)r[x] * a.ld + u];
            else wt_write_row(as + x * dim, a.a + (int64_t)u * dim, a.b + (int64_t)r[x] * dim, dim, lane);
            if (a.kkeys) {
                const int64_t klo = a.kptr[r[x]], khi = a.kptr[r[x] + 1];
                if (klo < khi) {
                    kc[x] = wt_lower_bound(a.kkeys, klo, khi, (int64_t)u * n, lane);
                    kend[x] = wt_lower_bound(a.kkeys, kc[x], khi, (int64_t)(u + 1) * n, lane);
                }
            }
            fwd[x] = kc[x] < kend[x];
            any_fwd = any_fwd || fwd[x];
        }
        if (MODE == WT_DISTMULT16) {
            wave_sync();
#pragma unroll
            for (int x = 0; x < PS_RB; ++x)
                if (rok[x]) wt_row16<WT_DISTMULT16>(aq[x], as + x * 16);
        }

        float acc[PS_RB];
        int cnt[PS_RB];
#pragma unroll
        for (int x = 0; x < PS_RB; ++x) { acc[x] = 0.f; cnt[x] = 0; }

        for (int c0 = 0; uok && c0 < n; c0 += WT_WIN) {
            const int c1 = c0 + WT_WIN < n ? c0 + WT_WIN : n;
            wave_sync();                                               // the previous window's bits have been read; the
                                                                       // product rows are written (first window)
            if (any_fwd) {
#pragma unroll
                for (int x = 0; x < PS_RB; ++x)
                    if (fwd[x])
                        wt_merge_window<PS_WORDS>(km + x * PS_WORDS, kc[x], kend[x], c0, c1, lane,
                                                  [&](int64_t idx) { return a.kkeys[idx] - (int64_t)u * n; });
                wave_sync();
            }
            for (int g0 = c0; g0 < c1; g0 += TIPK_WAVE) {
                const int c = g0 + lane;
                bool valid = c < c1 && c != u;
                float w = 1.0f;
                if (valid && a.pw) {
                    w = a.pw[c];
                    valid = w != 0.f;                                  // weight 0: no candidate (skipped, not multiplied)
                }
                const int cr = c < c1 ? c : c1 - 1;                    // a lane past the end reads a row that exists
                float s[PS_RB];
#pragma unroll
                for (int x = 0; x < PS_RB; ++x) s[x] = 0.f;
                if (MODE == WT_TABLE) {
#pragma unroll
                    for (int x = 0; x < PS_RB; ++x)
                        if (rok[x]) s[x] = s1u[x] + a.b[(int64_t)r[x] * a.ld + cr];
                } else if (MODE == WT_DISTMULT16) {
                    const float* zr = Z + (int64_t)cr * zstride;
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        const float4 z4 = *reinterpret_cast<const float4*>(zr + 4 * qd);
#pragma unroll
                        for (int x = 0; x < PS_RB; ++x) {
                            s[x] = fmaf(aq[x][qd].x, z4.x, s[x]);
                            s[x] = fmaf(aq[x][qd].y, z4.y, s[x]);
                            s[x] = fmaf(aq[x][qd].z, z4.z, s[x]);
                            s[x] = fmaf(aq[x][qd].w, z4.w, s[x]);
                        }
                    }
                } else {
                    const float* zr = Z + (int64_t)cr * zstride;
                    for (int k0 = 0; k0 < dim; k0 += 4) {
                        const float4 z4 = *reinterpret_cast<const float4*>(zr + k0);
#pragma unroll
                        for (int x = 0; x < PS_RB; ++x) {
                            const float4 h4 = *reinterpret_cast<const float4*>(as + x * dim + k0);
                            s[x] = fmaf(h4.x, z4.x, s[x]);
                            s[x] = fmaf(h4.y, z4.y, s[x]);
                            s[x] = fmaf(h4.z, z4.z, s[x]);
                            s[x] = fmaf(h4.w, z4.w, s[x]);
                        }
                    }
                }
#pragma unroll
                for (int x = 0; x < PS_RB; ++x) {
                    if (!rok[x]) continue;                             // uniform
                    bool cand = valid;
                    if (cand && fwd[x]) cand = !wt_bit(km + x * PS_WORDS, c - c0);
                    if (cand) {
                        acc[x] += w * ps_sigma(s[x]);
                        cnt[x] += 1;
                    }
                }
            }
        }

#pragma unroll
        for (int x = 0; x < PS_RB; ++x) {
            float p = acc[x];
            int m = cnt[x];
#pragma unroll
            for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) {
                p += __shfl_down(p, off);
                m += __shfl_down(m, off);
            }
            const int64_t j = j0 + x;
            if (lane == 0 && j < a.n_sel) {
                a.out_sum[q * a.n_sel + j] = rok[x] ? p : NAN;
                a.out_cnt[q * a.n_sel + j] = rok[x] ? m : 0;
            }
        }
    }
}

__global__ void __launch_bounds__(WT_NT) partner_sum_select_kernel(PartnerSumArgs a) {
    extern __shared__ __align__(16) unsigned char ps_smem[];
    const int lane = tipk_lane(), wave = threadIdx.x >> 6;
    const int k = a.k;
    const int flush_at = wt_flush_at(k);
    float* bs = reinterpret_cast<float*>(ps_smem) + wave * WT_CAP;
    int* br = reinterpret_cast<int*>(reinterpret_cast<float*>(ps_smem) + WT_NW * WT_CAP) + wave * WT_CAP;

    const int64_t n_blocks = (a.n_q + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t q = blk * WT_NW + wave;
        if (q >= a.n_q) continue;                                      // (the waves of a workgroup never meet in this loop)
        const float* row = a.out_sum + q * a.n_sel;
        int c = 0;
        float thr = -INFINITY;
        wave_sync();                                                   // the previous row's buffer has been written out
        for (int64_t w0 = 0; w0 < a.n_sel; w0 += TIPK_WAVE) {
            const int64_t idx = w0 + lane;
            const float v = idx < a.n_sel ? row[idx] : NAN;
            const bool pass = v == v && v >= thr;                      // NaN is never selected
            const unsigned long long mask = __ballot(pass);
            if (mask == 0ull) continue;
            if (pass) {
                const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                bs[pos] = v;
                br[pos] = (int)idx;
            }
            c += __popcll(mask);
            if (c >= flush_at) flush<false>(bs, br, nullptr, c, thr, k, lane);
        }
        if (c > 0) flush<false>(bs, br, nullptr, c, thr, k, lane);
        float* ov = a.top_val + q * k;
        int32_t* op = a.top_pos + q * k;
        for (int i = lane; i < k; i += TIPK_WAVE) {
            const bool have = i < c;
            ov[i] = have ? bs[i] : -INFINITY;
            op[i] = have ? br[i] : -1;
        }
    }
}

int64_t ps_fixed_bytes(int dim, bool table) {
    return (table ? 0 : (int64_t)WT_NW * PS_RB * dim * 4) + (int64_t)WT_NW * PS_RB * PS_WORDS * 4;
}

int ps_check_lists(int64_t n_nodes, int64_t n_rel, const int32_t* q_drug, int64_t n_q, const int32_t* rel_ids, int64_t n_sel,
                   const int64_t* keys, const int64_t* kptr, int k, const float* out_sum, const int32_t* out_count,
                   const float* out_top_val, const int32_t* out_top_pos) {
    if (k < 0 || k > WT_KMAX || n_q < 0 || n_sel < 0 || n_nodes < 1 || n_rel < 1) return TIPK_EINVAL;
    if (!rel_ids && n_sel != n_rel) return TIPK_EINVAL;                // no list: the columns are the relations
    if ((keys != nullptr) != (kptr != nullptr)) return TIPK_EINVAL;
    if (n_q > 0 && n_sel > 0) {
        if (!q_drug || !out_sum || !out_count) return TIPK_EINVAL;
        if (k > 0 && (!out_top_val || !out_top_pos)) return TIPK_EINVAL;
    }
    return TIPK_OK;
}

void ps_fill_lists(PartnerSumArgs& a, int64_t n_nodes, int64_t n_rel, const int32_t* q_drug, int64_t n_q,
                   const int32_t* rel_ids, int64_t n_sel, const float* partner_w, const int64_t* keys, const int64_t* kptr,
                   int k, float* out_sum, int32_t* out_count, float* out_top_val, int32_t* out_top_pos) {
    a.qdrug = q_drug; a.rel = rel_ids; a.pw = partner_w; a.kkeys = keys; a.kptr = kptr;
    a.n_q = n_q; a.n_sel = n_sel; a.n_jb = (n_sel + PS_RB - 1) / PS_RB;
    a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.k = k;
    a.out_sum = out_sum; a.out_cnt = out_count; a.top_val = out_top_val; a.top_pos = out_top_pos;
}

// launch 2 on the same stream, after launch 1 returned `status`
int ps_select(const PartnerSumArgs& a, int status, hipStream_t st) {
    if (status != TIPK_OK || a.k == 0) return status;
    return wt_launch<partner_sum_select_kernel>(a, wt_grid(a.n_q, 2), (size_t)WT_NW * WT_CAP * 8, st);
}

}  // namespace

extern "C" int tipk_distmult_partner_sum_supported(int64_t n_nodes, int dim, int64_t n_rel) {
    return wt_distmult_shape(n_nodes, dim, n_rel);
}

extern "C" int tipk_distmult_partner_sum_lds_route(int64_t n_nodes, int dim) {
    return wt_distmult_shape(n_nodes, dim, 1) && wt_fits_lds(n_nodes, dim, ps_fixed_bytes(dim, false)) &&
           !tipk_option(TIPK_OPT_PARTNER_SUM_GLOBAL);
}

extern "C" int tipk_distmult_partner_sum(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                         const int32_t* q_drug, int64_t n_q, const int32_t* rel_ids, int64_t n_sel,
                                         const float* partner_w, const int64_t* known_keys, const int64_t* known_ptr, int k,
                                         float* out_sum, int32_t* out_count, float* out_top_val, int32_t* out_top_pos,
                                         tipk_stream_t stream) {
    const int bad = ps_check_lists(n_nodes, n_rel, q_drug, n_q, rel_ids, n_sel, known_keys, known_ptr, k, out_sum, out_count,
                                   out_top_val, out_top_pos);
    if (bad != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_q > 0 && n_sel > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_partner_sum_supported(n_nodes, dim, n_rel) || n_sel > PS_SEL_MAX) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_sel == 0) return TIPK_OK;

    PartnerSumArgs a;
    ps_fill_lists(a, n_nodes, n_rel, q_drug, n_q, rel_ids, n_sel, partner_w, known_keys, known_ptr, k, out_sum, out_count,
                  out_top_val, out_top_pos);
    a.a = z; a.b = rel_w; a.ld = 0; a.dim = dim; a.stride = wt_stride(dim);
    const bool lds_route = tipk_distmult_partner_sum_lds_route(n_nodes, dim) != 0;
    const size_t lds = (lds_route ? (size_t)n_nodes * a.stride * 4 : 0) + (size_t)ps_fixed_bytes(dim, false);
    const int grid = wt_grid(a.n_q * a.n_jb, 1);                       // one workgroup of 16 waves per CU
    hipStream_t st = (hipStream_t)stream;
    int status;
    if (lds_route)
        status = dim == 16 ? wt_launch<partner_sum_kernel<WT_DISTMULT16, false>>(a, grid, lds, st)
                           : wt_launch<partner_sum_kernel<WT_DISTMULT, false>>(a, grid, lds, st);
    else
        status = dim == 16 ? wt_launch<partner_sum_kernel<WT_DISTMULT16, true>>(a, grid, lds, st)
                           : wt_launch<partner_sum_kernel<WT_DISTMULT, true>>(a, grid, lds, st);
    return ps_select(a, status, st);
}

extern "C" int tipk_pair_table_partner_sum_supported(int64_t n_nodes, int64_t n_rel) {
    return wt_table_shape(n_nodes, n_rel);
}

extern "C" int tipk_pair_table_partner_sum(const float* s1t, const float* s2t, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                           const int32_t* q_drug, int64_t n_q, const int32_t* rel_ids, int64_t n_sel,
                                           const float* partner_w, const int64_t* known_keys, const int64_t* known_ptr, int k,
                                           float* out_sum, int32_t* out_count, float* out_top_val, int32_t* out_top_pos,
                                           tipk_stream_t stream) {
    const int bad = ps_check_lists(n_nodes, n_rel, q_drug, n_q, rel_ids, n_sel, known_keys, known_ptr, k, out_sum, out_count,
                                   out_top_val, out_top_pos);
    if (bad != TIPK_OK || ld < n_nodes) return TIPK_EINVAL;
    if (n_q > 0 && n_sel > 0 && (!s1t || !s2t)) return TIPK_EINVAL;
    if (!tipk_pair_table_partner_sum_supported(n_nodes, n_rel) || n_sel > PS_SEL_MAX) return TIPK_EUNSUPPORTED;
    if (n_q == 0 || n_sel == 0) return TIPK_OK;

    PartnerSumArgs a;
    ps_fill_lists(a, n_nodes, n_rel, q_drug, n_q, rel_ids, n_sel, partner_w, known_keys, known_ptr, k, out_sum, out_count,
                  out_top_val, out_top_pos);
    a.a = s1t; a.b = s2t; a.ld = ld; a.dim = 0; a.stride = 0;
    hipStream_t st = (hipStream_t)stream;
    const int grid = wt_grid(a.n_q * a.n_jb, 2);                       // 16 KB of LDS each: two workgroups share a CU
    const int status = wt_launch<partner_sum_kernel<WT_TABLE, false>>(a, grid, (size_t)ps_fixed_bytes(0, true), st);
    return ps_select(a, status, st);
}
