// Protein attribution: the logit of a query split exactly over every protein target and every drug's own feature row, by one
// reverse pass through both R-GCN layers and the P -> D stage (include/tipk.h section 4o).
//
// Four kernels, the first once per call, the others once per chunk of PA_QCHUNK queries:
//   a. pa_cells_kernel   the pair cells of BOTH layers, C_l[i][j][b] = 1/deg_j * sum_{e: i -> j} att_l[rel_e][b], dense
//                        [N][N][B] in the workspace.  A workgroup owns destination j: it clears column j, then every run of
//                        equal sources in j's segment (sorted by (source, relation)) is summed by ONE group of lanes, edges
//                        ascending, and multiplied once by 1.0f / deg.  No atomics: one writer per cell.
//   b. pa_a1_kernel      a workgroup per query: G2 = basis2 g and root2 g in LDS, then
//                        a1[j][o] = (sum_b C2[j][v][b] G2[b][o] + [j == v] (root2 g)[o]) * (h[j][o] > 0).
//   c. pa_reverse_kernel a workgroup owns drug i and a tile of queries (PA_COLS = 256 columns = queries x padded d1):
//                        U[b][col] = sum_j C1[i][j][b] a1[j][col] on v_mfma_f32_32x32x2_f32, C1[i] and a1 streamed through LDS
//                        in slices of PA_KS rows j, zero-padded (no branch in the MFMA loop); U goes to LDS; then
//                        a0[c] = sum_{b,o} basis1[b][c][o] U[b][o] + sum_o root1[c][o] a1[i][o] (ONE fma chain), own = a0e . xe[i],
//                        qv = W_pd a0p.  Only own and qv are written: U, a0 and every per-edge value stay on the chip.
//   d. pa_protein_kernel a workgroup per query over the protein-side CSR: c_t = sum over t's entries of inv_cnt[i] * (hp[t] .
//                        qv[i]), the k largest through WgSel (tipk_wg_topk.h), both totals in fp64 in a fixed tree.
#include "tipk_wg_topk.h"

namespace {

constexpr int PA_NT = WG_NT;
constexpr int PA_DMAX = 128;               // every width
constexpr int PA_BMAX = 64;
constexpr int PA_KMAX = 1024;
constexpr int64_t PA_NMAX = 4096;          // dense cells: 2 N^2 B floats
constexpr int64_t PA_QCHUNK = 256;         // queries per pass over the workspace
constexpr int PA_KS = 32;                  // rows j per staged slice
constexpr int PA_COLS = 256;               // columns of a query tile: TQ queries x d1p
constexpr int PA_CAP = 4096;               // selection buffer entries
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PaArgs {
    const float *hp, *w_pd, *xe, *h, *basis1, *att1, *root1, *basis2, *att2, *root2, *inv_cnt, *probe;
    const int64_t *pe_ptr, *prot_ptr;
    const int32_t *pe_src, *pe_rel, *prot_drug, *q_node;
    int64_t ld_hp, ld_xe, ld_h, ld_att1, ld_att2, ld_probe, n_edges, n_pd, n_prot, n_rel;
    int n, p, pd, ne, d0, d1, d2, B, cat, k;
    int bp, d1p, tq;                       // padded bases (32 | 64), padded d1 (32 | 64 | 128), queries per tile
    int64_t q0;                            // first query of the chunk
    int nq;                                // queries of the chunk
    float *C1, *C2, *a1, *own, *qv;        // workspace
    float *out_contrib, *out_direct, *out_features, *out_proteins;
    int32_t* out_protein;
};

// ------------------------------------------------------------------------------------------------ a. cells
__global__ void __launch_bounds__(PA_NT) pa_cells_kernel(PaArgs a) {
    const int t = threadIdx.x, n = a.n, B = a.B, j = blockIdx.x;
    for (int idx = t; idx < n * B; idx += PA_NT) {
        const int i = idx / B, b = idx - i * B;
        const int64_t at = ((int64_t)i * n + j) * B + b;
        a.C1[at] = 0.f;
        a.C2[at] = 0.f;
    }
    __syncthreads();                                               // column j is clear before any cell of it is written
    const int bl = B <= 32 ? 32 : 64, slots = PA_NT / bl;
    const int b = t % bl, slot = t / bl;
    int64_t e0 = a.pe_ptr[j], e1 = a.pe_ptr[j + 1];
    e0 = e0 < 0 ? 0 : (e0 > a.n_edges ? a.n_edges : e0);
    e1 = e1 < e0 ? e0 : (e1 > a.n_edges ? a.n_edges : e1);
    const int64_t deg = e1 - e0;
    const float inv = 1.0f / (float)(deg > 0 ? deg : 1);
    for (int64_t pos = e0 + slot; pos < e1; pos += slots) {
        const int s = a.pe_src[pos];
        if (pos > e0 && a.pe_src[pos - 1] == s) continue;          // not the first edge of its pair
        float acc1 = 0.f, acc2 = 0.f;
        for (int64_t e = pos; e < e1 && a.pe_src[e] == s; ++e) {
            const int r = a.pe_rel[e];
            if (b < B && r >= 0 && r < a.n_rel) {
                acc1 += a.att1[(int64_t)r * a.ld_att1 + b];
                acc2 += a.att2[(int64_t)r * a.ld_att2 + b];
            }
        }
        if (b < B && s >= 0 && s < n) {
            const int64_t at = ((int64_t)s * n + j) * B + b;
            a.C1[at] = inv * acc1;
            a.C2[at] = inv * acc2;
        }
    }
}

// ------------------------------------------------------------------------------------------------ b. a1 of a query
__global__ void __launch_bounds__(PA_NT) pa_a1_kernel(PaArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* gv = smem;                                              // [d2]
    float* rg = gv + PA_DMAX;                                      // [d1]
    float* G2 = rg + PA_DMAX;                                      // [B][d1]
    const int t = threadIdx.x, n = a.n, B = a.B, d1 = a.d1, d2 = a.d2;
    const int ql = blockIdx.x;
    const int64_t q = a.q0 + ql;
    float* out = a.a1 + (int64_t)ql * n * d1;
    const int v = a.q_node[q];
    if (v < 0 || v >= n) {                                         // uniform: stage c reads zeros, stage d pads the row
        for (int idx = t; idx < n * d1; idx += PA_NT) out[idx] = 0.f;
        return;
    }
    if (t < d2) gv[t] = a.probe[q * a.ld_probe + t];
    __syncthreads();
    for (int pq = t; pq < B * d1; pq += PA_NT) {
        const float* row = a.basis2 + (int64_t)pq * d2;
        float acc = 0.f;
        for (int o = 0; o < d2; ++o) acc = fmaf(row[o], gv[o], acc);
        G2[pq] = acc;
    }
    for (int i = t; i < d1; i += PA_NT) {
        const float* row = a.root2 + (int64_t)i * d2;
        float acc = 0.f;
        for (int o = 0; o < d2; ++o) acc = fmaf(row[o], gv[o], acc);
        rg[i] = acc;
    }
    __syncthreads();
    for (int idx = t; idx < n * d1; idx += PA_NT) {
        const int j = idx / d1, o = idx - j * d1;
        const float* cell = a.C2 + ((int64_t)j * n + v) * B;
        float acc = 0.f;
#pragma unroll 4
        for (int b = 0; b < B; ++b) acc = fmaf(cell[b], G2[b * d1 + o], acc);
        if (j == v) acc += rg[o];
        out[idx] = a.h[(int64_t)j * a.ld_h + o] > 0.f ? acc : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ c. the large product
__host__ __device__ constexpr int pa_us_ld(int tq, int d1p) { return tq * (d1p + 1); }
// floats of LDS: Cs [KS][bp], As [KS][COLS], Us [bp][tq (d1p + 1)], a0s [tq][d0]
static int64_t pa_reverse_floats(int bp, int tq, int d1p, int d0) {
    return (int64_t)PA_KS * bp + (int64_t)PA_KS * PA_COLS + (int64_t)bp * pa_us_ld(tq, d1p) + (int64_t)tq * d0;
}

template <int MT>
__global__ void __launch_bounds__(PA_NT) pa_reverse_kernel(PaArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BP = 32 * MT;
    const int t = threadIdx.x, n = a.n, B = a.B, d1 = a.d1, d0 = a.d0, d1p = a.d1p, tq = a.tq;
    const int usld = pa_us_ld(tq, d1p);
    float* Cs = smem;                                              // [KS][BP]
    float* As = Cs + PA_KS * BP;                                   // [KS][COLS]
    float* Us = As + PA_KS * PA_COLS;                              // [BP][usld]
    float* a0s = Us + BP * usld;                                   // [tq][d0]
    const int i = blockIdx.x;
    const int ql0 = blockIdx.y * tq;                               // first query (in the chunk) of the tile
    const int lane = tipk_lane(), w = t >> 6, lo = lane & 31, hi = lane >> 5;
    const float* c1 = a.C1 + (int64_t)i * n * B;

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][c][r] = 0.f;

    for (int j0 = 0; j0 < n; j0 += PA_KS) {
        __syncthreads();                                           // the previous slice has been read
        for (int idx = t; idx < PA_KS * BP; idx += PA_NT) {
            const int kk = idx / BP, b = idx - kk * BP;
            Cs[idx] = (j0 + kk < n && b < B) ? c1[(int64_t)(j0 + kk) * B + b] : 0.f;
        }
        for (int idx = t; idx < PA_KS * PA_COLS; idx += PA_NT) {
            const int kk = idx / PA_COLS, col = idx - kk * PA_COLS;
            const int qi = col / d1p, o = col - qi * d1p;
            float x = 0.f;
            if (j0 + kk < n && o < d1 && ql0 + qi < a.nq) x = a.a1[((int64_t)(ql0 + qi) * n + j0 + kk) * d1 + o];
            As[idx] = x;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < PA_KS; kk += 2) {
            const float b0 = As[(kk + hi) * PA_COLS + (2 * w) * 32 + lo];
            const float b1 = As[(kk + hi) * PA_COLS + (2 * w + 1) * 32 + lo];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float av = Cs[(kk + hi) * BP + m * 32 + lo];
                acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[m][0], 0, 0, 0);
                acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[m][1], 0, 0, 0);
            }
        }
    }
    // U to LDS: row b, column (qi, o) at qi (d1p + 1) + o -- the odd stride keeps the epilogue's reads off one bank
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = (2 * w + c) * 32 + lo;
            const int qi = col / d1p, o = col - qi * d1p;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int b = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                Us[b * usld + qi * (d1p + 1) + o] = acc[m][c][r];
            }
        }
    __syncthreads();
    // a0[c] of every query of the tile: ONE chain over (b, o) ascending, then over root1's o
    for (int idx = t; idx < d0 * tq; idx += PA_NT) {
        const int qi = idx % tq, c = idx / tq;
        float s = 0.f;
        if (ql0 + qi < a.nq) {
            const float* u = Us + qi * (d1p + 1);
            for (int b = 0; b < B; ++b) {
                const float* brow = a.basis1 + ((int64_t)b * d0 + c) * d1;
                const float* urow = u + b * usld;
#pragma unroll 4
                for (int o = 0; o < d1; ++o) s = fmaf(brow[o], urow[o], s);
            }
            const float* rrow = a.root1 + (int64_t)c * d1;
            const float* arow = a.a1 + ((int64_t)(ql0 + qi) * n + i) * d1;
            for (int o = 0; o < d1; ++o) s = fmaf(rrow[o], arow[o], s);
        }
        a0s[qi * d0 + c] = s;
    }
    __syncthreads();
    const int off = a.cat ? a.ne : 0;
    if (t < tq && ql0 + t < a.nq) {
        const float* xrow = a.xe + (int64_t)i * a.ld_xe;
        float s = 0.f;
        for (int c = 0; c < a.ne; ++c) s = fmaf(a0s[t * d0 + c], xrow[c], s);
        a.own[(int64_t)(ql0 + t) * n + i] = s;
    }
    for (int idx = t; idx < tq * a.p; idx += PA_NT) {
        const int qi = idx / a.p, kx = idx - qi * a.p;
        if (ql0 + qi >= a.nq) continue;
        const float* wrow = a.w_pd + (int64_t)kx * a.pd;
        float s = 0.f;
        for (int c = 0; c < a.pd; ++c) s = fmaf(wrow[c], a0s[qi * d0 + off + c], s);
        a.qv[((int64_t)(ql0 + qi) * n + i) * a.p + kx] = s;
    }
}

// ------------------------------------------------------------------------------------------------ d. proteins of a query
using PaSel = WgSel<PA_NT, PA_CAP, PA_NT>;

__device__ __forceinline__ double pa_tree(double part, double* dred) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
    if (tipk_lane() == 0) dred[threadIdx.x >> 6] = part;
    __syncthreads();
    return ((dred[0] + dred[1]) + dred[2]) + dred[3];
}

// c of protein tt for the drugs `only` (>= 0: that drug alone; < 0: all): entries ascending, each inv_cnt * (hp . qv)
__device__ __forceinline__ float pa_protein_value(const PaArgs& a, const float* qv, int64_t e0, int64_t e1, int64_t tt, int only) {
    const float* hrow = a.hp + tt * a.ld_hp;
    float c = 0.f;
    for (int64_t e = e0; e < e1; ++e) {
        const int i = a.prot_drug[e];
        if (i < 0 || i >= a.n || (only >= 0 && i != only)) continue;
        const float* qrow = qv + (int64_t)i * a.p;
        float dot = 0.f;
        for (int kx = 0; kx < a.p; ++kx) dot = fmaf(hrow[kx], qrow[kx], dot);
        c += a.inv_cnt[i] * dot;
    }
    return c;
}

__global__ void __launch_bounds__(PA_NT) pa_protein_kernel(PaArgs a) {
    __shared__ float bs[PA_CAP];
    __shared__ int bk[PA_CAP];
    __shared__ double dred[2][4];
    __shared__ unsigned ctr[3];
    const int t = threadIdx.x, n = a.n, k = a.k;
    const int ql = blockIdx.x;
    const int64_t q = a.q0 + ql;
    float* oc = a.out_contrib + q * k;
    float* od = a.out_direct + q * k;
    int32_t* op = a.out_protein + q * k;
    const int v = a.q_node[q];
    if (v < 0 || v >= n) {                                         // uniform
        for (int i = t; i < k; i += PA_NT) { oc[i] = -INFINITY; op[i] = -1; od[i] = 0.f; }
        if (t == 0) { a.out_features[q] = NAN; a.out_proteins[q] = NAN; }
        return;
    }
    if (t < 3) ctr[t] = 0u;
    const float* own = a.own + (int64_t)ql * n;
    const float* qv = a.qv + (int64_t)ql * n * a.p;
    double part = 0.0;
    for (int i = t; i < n; i += PA_NT) part += (double)own[i];
    const double features = pa_tree(part, dred[0]);                // (its barrier also publishes ctr)
    PaSel sel;
    sel.init(bs, bk, ctr, k);
    part = 0.0;
    for (int64_t base = 0; base < a.n_prot; base += PA_NT) {
        const int64_t tt = base + t;
        bool ok = false;
        float c = 0.f;
        if (tt < a.n_prot) {
            int64_t e0 = a.prot_ptr[tt], e1 = a.prot_ptr[tt + 1];
            e0 = e0 < 0 ? 0 : (e0 > a.n_pd ? a.n_pd : e0);
            e1 = e1 < e0 ? e0 : (e1 > a.n_pd ? a.n_pd : e1);
            ok = e1 > e0;                                          // a protein no drug targets is no candidate
            if (ok) {
                c = pa_protein_value(a, qv, e0, e1, tt, -1);
                part += (double)c;
            }
        }
        sel.append(sel.wants(ok, c), c, (int)tt);
        sel.end_round();
    }
    const double proteins = pa_tree(part, dred[1]);
    sel.flush();
    __syncthreads();
    if (t == 0) { a.out_features[q] = (float)features; a.out_proteins[q] = (float)proteins; }
    for (int i = t; i < k; i += PA_NT) {
        const bool have = i < sel.c;
        float direct = 0.f;
        if (have) {
            const int64_t tt = bk[i];
            int64_t e0 = a.prot_ptr[tt], e1 = a.prot_ptr[tt + 1];
            e0 = e0 < 0 ? 0 : (e0 > a.n_pd ? a.n_pd : e0);
            e1 = e1 < e0 ? e0 : (e1 > a.n_pd ? a.n_pd : e1);
            direct = pa_protein_value(a, qv, e0, e1, tt, v);
        }
        oc[i] = have ? bs[i] : -INFINITY;
        op[i] = have ? bk[i] : -1;
        od[i] = direct;
    }
}

int pa_pad_d1(int d1) { return d1 <= 32 ? 32 : (d1 <= 64 ? 64 : 128); }

template <int MT>
int pa_launch_reverse(const PaArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)pa_reverse_kernel<MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(pa_reverse_kernel<MT>, grid, dim3(PA_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int64_t tipk_protein_attribution_chunk(void) { return PA_QCHUNK; }

extern "C" int tipk_protein_attribution_supported(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int pd, int p,
                                                  int d1, int d2, int cat, int k) {
    if (n_nodes < 1 || n_nodes > PA_NMAX || n_prot < 1 || n_prot > 0x7fffffffLL || n_rel < 1 || n_bases < 1 || n_bases > PA_BMAX)
        return 0;
    if (ne < 1 || pd < 1 || p < 1 || d1 < 1 || d2 < 1 || p > PA_DMAX || d1 > PA_DMAX || d2 > PA_DMAX || ne > PA_DMAX || pd > PA_DMAX)
        return 0;
    if (cat ? ne + pd > PA_DMAX : ne != pd) return 0;
    return k >= 1 && k <= PA_KMAX;
}

extern "C" int64_t tipk_protein_attribution_workspace_bytes(int64_t n_nodes, int n_bases, int d1, int p, int64_t n_q) {
    if (n_q < 0 || n_nodes < 1 || n_nodes > PA_NMAX || n_bases < 1 || n_bases > PA_BMAX || d1 < 1 || d1 > PA_DMAX || p < 1 ||
        p > PA_DMAX)
        return -1;
    const int64_t qc = n_q < PA_QCHUNK ? n_q : PA_QCHUNK;
    return (2 * n_nodes * n_nodes * n_bases + qc * n_nodes * ((int64_t)d1 + 1 + p)) * 4;
}

extern "C" int tipk_protein_attribution(const float* hp, int64_t ld_hp, int64_t n_prot, int p, const float* w_pd, int pd,
                                        const float* xe, int64_t ld_xe, int ne, const float* h, int64_t ld_h, int64_t n_nodes,
                                        int d1, const float* basis1, const float* att1, int64_t ld_att1, const float* root1,
                                        const float* basis2, const float* att2, int64_t ld_att2, const float* root2, int d2,
                                        int64_t n_rel, int n_bases, const int64_t* pe_ptr, const int32_t* pe_src,
                                        const int32_t* pe_rel, int64_t n_edges, const int64_t* prot_ptr, const int32_t* prot_drug,
                                        int64_t n_pd_edges, const float* inv_cnt, int cat, const int32_t* q_node,
                                        const float* probe, int64_t ld_probe, int64_t n_q, int k, float* out_contrib,
                                        int32_t* out_protein, float* out_direct, float* out_features, float* out_proteins,
                                        void* workspace, tipk_stream_t stream) {
    if (k <= 0 || n_q < 0 || n_edges < 0 || n_pd_edges < 0 || n_nodes < 1 || n_prot < 1 || n_rel < 1 || n_bases < 1 || p < 1 ||
        pd < 1 || ne < 1 || d1 < 1 || d2 < 1)
        return TIPK_EINVAL;
    if (ld_hp < p || ld_xe < ne || ld_h < d1 || ld_att1 < n_bases || ld_att2 < n_bases || ld_probe < d2) return TIPK_EINVAL;
    if (!cat && ne != pd) return TIPK_EINVAL;
    if (n_q > 0 && (!hp || !w_pd || !xe || !h || !basis1 || !att1 || !root1 || !basis2 || !att2 || !root2 || !pe_ptr || !prot_ptr ||
                    !inv_cnt || !q_node || !probe || !out_contrib || !out_protein || !out_direct || !out_features ||
                    !out_proteins || !workspace || (n_edges > 0 && (!pe_src || !pe_rel)) || (n_pd_edges > 0 && !prot_drug)))
        return TIPK_EINVAL;
    if (n_q > 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return TIPK_EINVAL;
    if (!tipk_protein_attribution_supported(n_nodes, n_prot, n_rel, n_bases, ne, pd, p, d1, d2, cat, k)) return TIPK_EUNSUPPORTED;
    if (n_edges > 0x7fffffffLL || n_pd_edges > 0x7fffffffLL || n_q > 0x7fffffffLL || n_rel > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if (n_q == 0) return TIPK_OK;

    PaArgs a;
    a.hp = hp; a.w_pd = w_pd; a.xe = xe; a.h = h; a.basis1 = basis1; a.att1 = att1; a.root1 = root1;
    a.basis2 = basis2; a.att2 = att2; a.root2 = root2; a.inv_cnt = inv_cnt; a.probe = probe;
    a.pe_ptr = pe_ptr; a.prot_ptr = prot_ptr; a.pe_src = pe_src; a.pe_rel = pe_rel; a.prot_drug = prot_drug; a.q_node = q_node;
    a.ld_hp = ld_hp; a.ld_xe = ld_xe; a.ld_h = ld_h; a.ld_att1 = ld_att1; a.ld_att2 = ld_att2; a.ld_probe = ld_probe;
    a.n_edges = n_edges; a.n_pd = n_pd_edges; a.n_prot = n_prot; a.n_rel = n_rel;
    a.n = (int)n_nodes; a.p = p; a.pd = pd; a.ne = ne; a.d0 = cat ? ne + pd : ne; a.d1 = d1; a.d2 = d2; a.B = n_bases;
    a.cat = cat ? 1 : 0; a.k = k;
    a.bp = n_bases <= 32 ? 32 : 64; a.d1p = pa_pad_d1(d1); a.tq = PA_COLS / a.d1p;
    const int64_t qc = n_q < PA_QCHUNK ? n_q : PA_QCHUNK;
    float* ws = (float*)workspace;
    a.C1 = ws;
    a.C2 = a.C1 + n_nodes * n_nodes * n_bases;
    a.a1 = a.C2 + n_nodes * n_nodes * n_bases;
    a.own = a.a1 + qc * n_nodes * d1;
    a.qv = a.own + qc * n_nodes;
    a.out_contrib = out_contrib; a.out_protein = out_protein; a.out_direct = out_direct;
    a.out_features = out_features; a.out_proteins = out_proteins;
    a.q0 = 0; a.nq = 0;
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(pa_cells_kernel, dim3((unsigned)n_nodes), dim3(PA_NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    const size_t lds_a1 = (size_t)(2 * PA_DMAX + (int64_t)n_bases * d1) * 4;
    const size_t lds_rev = (size_t)pa_reverse_floats(a.bp, a.tq, a.d1p, a.d0) * 4;
    for (int64_t q0 = 0; q0 < n_q; q0 += PA_QCHUNK) {
        a.q0 = q0;
        a.nq = (int)(n_q - q0 < PA_QCHUNK ? n_q - q0 : PA_QCHUNK);
        hipLaunchKernelGGL(pa_a1_kernel, dim3((unsigned)a.nq), dim3(PA_NT), lds_a1, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return tipk_hip_status(e);
        const dim3 grid((unsigned)n_nodes, (unsigned)((a.nq + a.tq - 1) / a.tq));
        const int s = a.bp == 32 ? pa_launch_reverse<1>(a, grid, lds_rev, st) : pa_launch_reverse<2>(a, grid, lds_rev, st);
        if (s != TIPK_OK) return s;
        hipLaunchKernelGGL(pa_protein_kernel, dim3((unsigned)a.nq), dim3(PA_NT), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return tipk_hip_status(e);
    }
    return TIPK_OK;
}
