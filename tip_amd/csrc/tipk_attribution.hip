// Edge attribution of the last R-GCN layer: the k in-edges of a node that contribute most to probe . z[node]
// (include/tipk.h section 4j).
//
// One workgroup (256 threads) per query (node v, probe g), four stages with the query's state in LDS:
//   1. G[b][i] = sum_o basis[b][i][o] * g[o] and rg[i] = sum_o root[i][o] * g[o]: a thread per (b, i), o ascending.  G is kept
//      transposed (Gt[i][b], b padded to a multiple of 8) so that stage 2 reads 8 bases of one i with two 16-byte loads.
//   2. The query's table M[s][b] = sum_i h[s][i] * G[b][i] for EVERY node s: blocks of 256 rows of h are staged in LDS 32
//      columns at a time (coalesced rows, row stride 33: conflict-free both ways); a thread owns one row and 8 bases in
//      registers, i ascending; between column chunks the partial sums rest in the table (exact: fp32 in, fp32 out).  The
//      table is stored base-major (Mt[b][s]): stage 3's lanes read neighbouring sources of one base.
//   3. One pass over v's in-edges, 1024 edges per round, four per thread (positions t, t + 256, ...: four chains in
//      flight): c_e = (1 / deg) * sum_b att[rel_e][b] * M[src_e][b], b ascending.  The relation-sorted segment makes
//      neighbouring lanes share att rows.  Every c_e is added to the thread's fp64 partial (positions ascending);
//      candidates go through the selection of tipk_wg_topk.h (WgSel): an LDS buffer (in the place of the staged block of
//      h), a running k-th-best threshold that drops most edges before they are appended, a bitonic cut when the buffer
//      could overflow.  The order is total (value descending, position ascending), so the kept set does not depend on the
//      order of the appends.
//   4. The fp64 partials are added in a fixed tree (lanes by shuffle, 32 .. 1; then the four wavefronts in order) and
//      rounded once; the buffer is cut a last time and written with the edges' source and relation.
// Routes: the table lives in LDS where n_nodes x n_bases floats fit beside the rest (tipk_rgcn_attribution_lds_route: 645 x
// 32 does), else -- or under option "attribution_global" -- in a slice of the caller's workspace owned by the workgroup, and
// at most 256 workgroups loop over the queries.  The arithmetic is the same code: same bits.
#include "tipk_wg_topk.h"

namespace {

constexpr int AT_NT = WG_NT;               // threads per workgroup: rows of a staged block of h, edges of a round
constexpr int AT_IC = 32;                  // columns of h per staged chunk
constexpr int AT_LDT = AT_IC + 1;          // LDS row stride of the staged block (floats)
constexpr int AT_BC = 8;                   // bases a thread keeps in registers
constexpr int AT_EPT = 4;                  // edges per thread and round: four independent chains in flight
constexpr int AT_ROUND = AT_NT * AT_EPT;   // edges per round
constexpr int AT_CAP = 4096;               // selection buffer entries (power of two >= k_max + one round); it takes the
                                           // place of the staged block of h, which is dead by then
constexpr int AT_KMAX = 1024;
constexpr int AT_DMAX = 128;
constexpr int AT_BMAX = 64;
constexpr int64_t AT_NMAX = 46340;
constexpr int64_t AT_RMAX = 65536;
constexpr int64_t AT_LDS_BYTES = 160 * 1024;
constexpr int AT_GLOBAL_WG = 256;          // workgroups (= workspace slices) of the global route

struct AttrArgs {
    const float *h, *basis, *att, *root, *probe;
    const int64_t* in_ptr;
    const int32_t *in_src, *in_rel, *q_node;
    int64_t ld_h, ld_att, ld_probe, n_q, n_edges;
    int n, d_in, d_out, n_bases, bp, k;
    float* out_contrib;
    int32_t *out_src, *out_rel;
    float *out_own, *out_sum;
    float* ws;                 // global route: [gridDim.x][n_bases x n]
};

// the selection of tipk_wg_topk.h with the edge's position in its segment as the key (no filter)
using Sel = WgSel<AT_NT, AT_CAP, AT_ROUND>;

// floats of LDS in front of the table: g, root . g, Gt, the staged block of h (later the selection buffer), the reduction cells
static_assert(2 * AT_CAP <= AT_NT * AT_LDT, "the selection buffer lives in the staged block");
__host__ __device__ constexpr int64_t at_fixed_floats(int d_in, int bp) {
    return 2 * AT_DMAX + (int64_t)d_in * bp + AT_NT * AT_LDT + 16;
}

template <bool LDS_TABLE>
__global__ void __launch_bounds__(AT_NT) attribution_kernel(AttrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* gv = smem;                                          // [d_out]
    float* rg = gv + AT_DMAX;                                  // [d_in]
    float* Gt = rg + AT_DMAX;                                  // [d_in][bp]
    float* tile = Gt + a.d_in * a.bp;                          // [256][33]
    float* bs = tile;                                          // stage 3 on: [AT_CAP] values, [AT_CAP] positions
    int* bk = reinterpret_cast<int*>(bs + AT_CAP);
    double* dred = reinterpret_cast<double*>(tile + AT_NT * AT_LDT);   // [4]
    unsigned* ctr = reinterpret_cast<unsigned*>(dred + 4);     // [3]
    float* Mt = LDS_TABLE ? reinterpret_cast<float*>(ctr + 8)  // [n_bases][n]
                          : a.ws + (int64_t)blockIdx.x * a.n_bases * a.n;

    const int t = threadIdx.x;
    const int n = a.n, d_in = a.d_in, d_out = a.d_out, B = a.n_bases, bp = a.bp, k = a.k;
    // whole att rows as 16-byte pieces (same values, same order): every row start aligned, no tail
    const bool att4 = B % 4 == 0 && a.ld_att % 4 == 0 && (reinterpret_cast<uintptr_t>(a.att) & 15) == 0;

    for (int64_t q = blockIdx.x; q < a.n_q; q += gridDim.x) {
        float* oc = a.out_contrib + q * k;
        int32_t* os = a.out_src + q * k;
        int32_t* orl = a.out_rel + q * k;
        const int v = a.q_node[q];
        if (v < 0 || v >= n) {                                 // uniform
            for (int i = t; i < k; i += AT_NT) { oc[i] = -INFINITY; os[i] = -1; orl[i] = -1; }
            if (t == 0) { a.out_own[q] = NAN; a.out_sum[q] = NAN; }
            continue;
        }
        int64_t e0 = a.in_ptr[v], e1 = a.in_ptr[v + 1];
        e0 = e0 < 0 ? 0 : (e0 > a.n_edges ? a.n_edges : e0);
        e1 = e1 < e0 ? e0 : (e1 > a.n_edges ? a.n_edges : e1);
        const int deg = (int)(e1 - e0);

        // 1. g, then G (transposed) and root . g
        if (t < d_out) gv[t] = a.probe[q * a.ld_probe + t];
        if (t < 3) ctr[t] = 0u;
        for (int i = t; i < d_in * bp; i += AT_NT) Gt[i] = 0.f;
        __syncthreads();
        for (int p = t; p < B * d_in; p += AT_NT) {
            const int b = p / d_in, i = p - b * d_in;
            const float* row = a.basis + (int64_t)p * d_out;
            float acc = 0.f;
#pragma unroll 4
            for (int o = 0; o < d_out; ++o) acc = fmaf(row[o], gv[o], acc);
            Gt[i * bp + b] = acc;
        }
        for (int i = t; i < d_in; i += AT_NT) {
            const float* row = a.root + (int64_t)i * d_out;
            float acc = 0.f;
            for (int o = 0; o < d_out; ++o) acc = fmaf(row[o], gv[o], acc);
            rg[i] = acc;
        }
        __syncthreads();
        if (t == AT_NT - 1) {
            const float* hv = a.h + (int64_t)v * a.ld_h;
            float acc = 0.f;
            for (int i = 0; i < d_in; ++i) acc = fmaf(hv[i], rg[i], acc);
            a.out_own[q] = acc;
        }

        // 2. the table M = h G^T, base-major
        for (int s0 = 0; s0 < n; s0 += AT_NT) {
            const int s = s0 + t;
            for (int i0 = 0; i0 < d_in; i0 += AT_IC) {
                const int ic = d_in - i0 < AT_IC ? d_in - i0 : AT_IC;
                __syncthreads();                                   // the previous chunk has been read
                for (int idx = t; idx < AT_NT * AT_IC; idx += AT_NT) {
                    const int row = idx / AT_IC, col = idx % AT_IC;
                    float x = 0.f;
                    if (s0 + row < n && col < ic) x = a.h[(int64_t)(s0 + row) * a.ld_h + i0 + col];
                    tile[row * AT_LDT + col] = x;
                }
                __syncthreads();
                for (int bc = 0; bc < bp; bc += AT_BC) {
                    float acc[AT_BC];
#pragma unroll
                    for (int j = 0; j < AT_BC; ++j)
                        acc[j] = (i0 > 0 && s < n && bc + j < B) ? Mt[(int64_t)(bc + j) * n + s] : 0.f;
#pragma unroll 4
                    for (int i = 0; i < ic; ++i) {
                        const float x = tile[t * AT_LDT + i];
                        const float4 g0 = tipk_ld4(&Gt[(i0 + i) * bp + bc]);
                        const float4 g1 = tipk_ld4(&Gt[(i0 + i) * bp + bc + 4]);
                        acc[0] = fmaf(x, g0.x, acc[0]); acc[1] = fmaf(x, g0.y, acc[1]);
                        acc[2] = fmaf(x, g0.z, acc[2]); acc[3] = fmaf(x, g0.w, acc[3]);
                        acc[4] = fmaf(x, g1.x, acc[4]); acc[5] = fmaf(x, g1.y, acc[5]);
                        acc[6] = fmaf(x, g1.z, acc[6]); acc[7] = fmaf(x, g1.w, acc[7]);
                    }
#pragma unroll
                    for (int j = 0; j < AT_BC; ++j)
                        if (s < n && bc + j < B) Mt[(int64_t)(bc + j) * n + s] = acc[j];
                }
            }
        }
        __syncthreads();                                           // the table is complete

        // 3. one pass over the in-edges
        Sel sel;
        sel.init(bs, bk, ctr, k);
        const float inv = 1.0f / (float)(deg > 0 ? deg : 1);
        double part = 0.0;
        for (int64_t base = 0; base < deg; base += AT_ROUND) {
            int src[AT_EPT];
            const float* ar[AT_EPT];
            float acc[AT_EPT];
#pragma unroll
            for (int j = 0; j < AT_EPT; ++j) {                     // (a lane past the end reads the segment's first edge)
                const int64_t pos = base + j * AT_NT + t;
                const int64_t e = e0 + (pos < deg ? pos : 0);
                src[j] = a.in_src[e];
                ar[j] = a.att + (int64_t)a.in_rel[e] * a.ld_att;
                acc[j] = 0.f;
            }
            if (att4) {                                            // 16-byte reads of the att rows: a quarter of the requests
#pragma unroll 2
                for (int b = 0; b < B; b += 4) {
                    float4 av[AT_EPT];
#pragma unroll
                    for (int j = 0; j < AT_EPT; ++j) av[j] = tipk_ld4(ar[j] + b);
#pragma unroll
                    for (int j = 0; j < AT_EPT; ++j) {
                        const float* m = Mt + (int64_t)b * n + src[j];
                        acc[j] = fmaf(av[j].x, m[0], acc[j]);
                        acc[j] = fmaf(av[j].y, m[n], acc[j]);
                        acc[j] = fmaf(av[j].z, m[2 * (int64_t)n], acc[j]);
                        acc[j] = fmaf(av[j].w, m[3 * (int64_t)n], acc[j]);
                    }
                }
            } else {
#pragma unroll 4
                for (int b = 0; b < B; ++b) {
#pragma unroll
                    for (int j = 0; j < AT_EPT; ++j) acc[j] = fmaf(ar[j][b], Mt[(int64_t)b * n + src[j]], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < AT_EPT; ++j) {
                const int64_t pos = base + j * AT_NT + t;
                const bool ok = pos < deg;
                const float c = inv * acc[j];
                if (ok) part += (double)c;
                sel.append(sel.wants(ok, c), c, (int)pos);
            }
            sel.end_round();
        }

        // 4. the sum in a fixed tree; the list
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
        if (tipk_lane() == 0) dred[t >> 6] = part;
        sel.flush();                                               // (its barriers publish dred too)
        __syncthreads();
        if (t == 0) a.out_sum[q] = (float)(((dred[0] + dred[1]) + dred[2]) + dred[3]);
        for (int i = t; i < k; i += AT_NT) {
            const bool have = i < sel.c;
            oc[i] = have ? bs[i] : -INFINITY;
            os[i] = have ? a.in_src[e0 + bk[i]] : -1;
            orl[i] = have ? a.in_rel[e0 + bk[i]] : -1;
        }
        __syncthreads();                                           // LDS is free for the next query
    }
}

int at_bp(int n_bases) { return (n_bases + AT_BC - 1) / AT_BC * AT_BC; }

template <bool LDS_TABLE>
int at_launch(const AttrArgs& a, unsigned grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)attribution_kernel<LDS_TABLE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(attribution_kernel<LDS_TABLE>, dim3(grid), dim3(AT_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_rgcn_attribution_supported(int64_t n_nodes, int64_t n_rel, int n_bases, int d_in, int d_out, int k) {
    return n_nodes >= 1 && n_nodes <= AT_NMAX && n_rel >= 1 && n_rel <= AT_RMAX && n_bases >= 1 && n_bases <= AT_BMAX &&
           d_in >= 1 && d_in <= AT_DMAX && d_out >= 1 && d_out <= AT_DMAX && k >= 1 && k <= AT_KMAX;
}

extern "C" int tipk_rgcn_attribution_lds_route(int64_t n_nodes, int n_bases) {
    if (n_nodes < 1 || n_nodes > AT_NMAX || n_bases < 1 || n_bases > AT_BMAX) return 0;
    return (at_fixed_floats(AT_DMAX, at_bp(n_bases)) + n_nodes * n_bases) * 4 <= AT_LDS_BYTES &&
           !tipk_option(TIPK_OPT_ATTRIBUTION_GLOBAL);
}

extern "C" int64_t tipk_rgcn_attribution_workspace_bytes(int64_t n_nodes, int n_bases, int64_t n_q) {
    if (n_q < 0 || n_nodes < 1 || n_nodes > AT_NMAX || n_bases < 1 || n_bases > AT_BMAX) return -1;
    if (tipk_rgcn_attribution_lds_route(n_nodes, n_bases)) return 0;
    return (n_q < AT_GLOBAL_WG ? n_q : AT_GLOBAL_WG) * n_nodes * n_bases * 4;
}

extern "C" int tipk_rgcn_attribution(const float* h, int64_t ld_h, int64_t n_nodes, int d_in, const float* basis,
                                     const float* att, int64_t ld_att, int64_t n_rel, int n_bases, const float* root,
                                     int d_out, const int64_t* in_ptr, const int32_t* in_src, const int32_t* in_rel,
                                     int64_t n_edges, const int32_t* q_node, const float* probe, int64_t ld_probe,
                                     int64_t n_q, int k, float* out_contrib, int32_t* out_src, int32_t* out_rel,
                                     float* out_own, float* out_sum, void* workspace, tipk_stream_t stream) {
    if (k <= 0 || n_q < 0 || n_edges < 0 || n_nodes < 1 || n_rel < 1 || n_bases < 1 || d_in < 1 || d_out < 1)
        return TIPK_EINVAL;
    if (ld_h < d_in || ld_att < n_bases || ld_probe < d_out) return TIPK_EINVAL;
    if (n_q > 0 && (!h || !basis || !att || !root || !in_ptr || !q_node || !probe || !out_contrib || !out_src ||
                    !out_rel || !out_own || !out_sum || (n_edges > 0 && (!in_src || !in_rel))))
        return TIPK_EINVAL;
    if (!tipk_rgcn_attribution_supported(n_nodes, n_rel, n_bases, d_in, d_out, k)) return TIPK_EUNSUPPORTED;
    if (n_edges > 0x7fffffffLL || n_q > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    const bool in_lds = tipk_rgcn_attribution_lds_route(n_nodes, n_bases) != 0;
    if (n_q > 0 && !in_lds && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)) return TIPK_EINVAL;
    if (n_q == 0) return TIPK_OK;

    AttrArgs a;
    a.h = h; a.basis = basis; a.att = att; a.root = root; a.probe = probe;
    a.in_ptr = in_ptr; a.in_src = in_src; a.in_rel = in_rel; a.q_node = q_node;
    a.ld_h = ld_h; a.ld_att = ld_att; a.ld_probe = ld_probe; a.n_q = n_q; a.n_edges = n_edges;
    a.n = (int)n_nodes; a.d_in = d_in; a.d_out = d_out; a.n_bases = n_bases; a.bp = at_bp(n_bases); a.k = k;
    a.out_contrib = out_contrib; a.out_src = out_src; a.out_rel = out_rel; a.out_own = out_own; a.out_sum = out_sum;
    a.ws = (float*)workspace;
    const int64_t fixed = at_fixed_floats(d_in, a.bp);
    hipStream_t st = (hipStream_t)stream;
    if (in_lds) return at_launch<true>(a, (unsigned)n_q, (size_t)((fixed + n_nodes * n_bases) * 4), st);
    return at_launch<false>(a, (unsigned)(n_q < AT_GLOBAL_WG ? n_q : AT_GLOBAL_WG), (size_t)(fixed * 4), st);
}
