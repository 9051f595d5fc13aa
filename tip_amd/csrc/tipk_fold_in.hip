// Fold-in of drugs that are no node of the training graph: x0, h1 and z rows of M new drugs from the frozen model's tables
// (include/tipk.h section 4k).
//
// One workgroup (512 threads, 8 wavefronts) per tile of up to 16 new drugs -- the M of v_mfma_f32_16x16x4_f32; fewer per tile
// in a call of fewer than 4 096 drugs (fi_tile_drugs), which changes no bit: a row depends on its own drug alone -- in four stages:
//   0. x0 of the tile: wavefront w takes drugs w and w + 8; lane j < p sums column j of h_prot over the drug's targets (segment
//      order), scales by 1 / max(t, 1); lane c < pd contracts with hgcn_w (j ascending, the means by shuffle); cat | add with
//      xd.  The rows rest in LDS (the root terms read them) and go to x0_new.
//   1. Aggregate first, in passes of nb <= 16 bases (as many as the LDS image takes): A1[m][b][:] = sum_e att1[rel_e, b] *
//      x0[src_e, :] and A2[m][b][:] = sum_e att2[rel_e, b] * h1[src_e, :] in ONE walk over the segment per pass.  Per drug
//      this is itself a product, att[rel_e, b]^T [nb x deg] . x[src_e, :] [deg x d], with the EDGES as K: it runs on the
//      matrix cores too, four edges per MFMA in segment order (an exact fmaf chain per entry along the segment).  Wavefronts
//      0 .. 3 take the even drugs of the tile, 4 .. 7 the odd ones; the 16-column tiles of A1 and A2 are dealt to the four
//      (tile j to wavefront j mod 4): a hub's segment is walked by four wavefronts side by side and holds up only its own
//      half of the tile.  Edge ids are read 64 at a time (one per lane) and passed by shuffle; the operands of 32 edges
//      (one att value and one table value per lane, MFMA and tile) are in flight together.
//   2. Contract: out1 [16 x d1] += A1 [16 x nb d0] . basis1[b0 .. b0 + nb) and out2 likewise, on the fp32 matrix cores: the K
//      range of the pass in steps of 16, step s on wavefront s mod 8, every basis row read once per tile.
//   3. After the last pass the eight wavefronts' partial tiles are added in a fixed tree, scaled by 1 / max(deg, 1), the root
//      term is added (i ascending), ReLU for layer 1; h1 rests in LDS for layer 2's root term.
// No atomics, no workspace: every output row depends on its own drug alone and is bitwise repeatable, whatever the tile.
#include "tipk_common.h"

namespace {

constexpr int FI_NT = 512;                 // threads per workgroup
constexpr int FI_NW = FI_NT / TIPK_WAVE;   // 8 wavefronts
constexpr int FI_MT = 16;                  // new drugs per tile
constexpr int FI_NB = 16;                  // bases per pass at most: the M of one MFMA tile
constexpr int FI_JOBS = 3;                 // 16-column tiles of A1 | A2 per wavefront: (128 + 64) / 16 over four wavefronts
constexpr int FI_KS = 8;                   // MFMA steps (4 edges each) whose operands a wavefront loads together
constexpr int FI_D0MAX = 128;
constexpr int FI_DMAX = 64;                // d1, d2, p, pd, n_bases
constexpr int FI_NTILE = FI_DMAX / 16;     // 16-column output tiles per layer at most
constexpr int FI_PAD = 4;                  // floats behind a row of the LDS images
constexpr int64_t FI_A_FLOATS = 25088;     // LDS floats for the two images of a pass (98 KB)
constexpr int64_t FI_RMAX = 1 << 24;

typedef float fi_f4 __attribute__((ext_vector_type(4)));

struct FoldArgs {
    const float *h_prot, *hgcn_w, *x0, *h1, *basis1, *att1, *root1, *basis2, *att2, *root2, *xd;
    const int64_t *tgt_ptr, *in_ptr;
    const int32_t *tgt_prot, *in_src, *in_rel;
    int64_t ld_h_prot, ld_x0, ld_h1, ld_att1, ld_att2, ld_xd, n_tgt, n_edges, n_new, ld_x0_new, ld_h1_new, ld_z_new;
    int p, pd, ne, d0, d1, d2, n_bases, cat, nb, tile;
    float *x0_new, *h1_new, *z_new;
};

__host__ __device__ constexpr int fi_up16(int x) { return (x + 15) / 16 * 16; }

// LDS floats of the two images of a pass of nb bases
__host__ __device__ constexpr int64_t fi_images(int nb, int d0, int d1) {
    return (int64_t)FI_MT * (fi_up16(nb * d0) + FI_PAD + fi_up16(nb * d1) + FI_PAD);
}

__global__ void __launch_bounds__(FI_NT) fold_in_kernel(FoldArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* x0n = smem;                                          // [16][d0]
    float* h1n = x0n + FI_MT * FI_D0MAX;                        // [16][d1]
    float* inv = h1n + FI_MT * FI_DMAX;                         // [16]
    int* seg = reinterpret_cast<int*>(inv + FI_MT);             // [16][2] first edge, edge count
    float* img = reinterpret_cast<float*>(seg + 2 * FI_MT);     // the images of a pass; later the wavefronts' partial tiles

    const int t = threadIdx.x, lane = tipk_lane(), w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int p = a.p, pd = a.pd, ne = a.ne, d0 = a.d0, d1 = a.d1, d2 = a.d2, B = a.n_bases;
    const int64_t m0 = (int64_t)blockIdx.x * a.tile;
    const int rows = a.n_new - m0 < a.tile ? (int)(a.n_new - m0) : a.tile;

    // 0. the tile's x0 rows
    if (t < FI_MT) {
        int64_t e0 = 0, e1 = 0;
        if (t < rows) {
            e0 = a.in_ptr[m0 + t]; e1 = a.in_ptr[m0 + t + 1];
            e0 = e0 < 0 ? 0 : (e0 > a.n_edges ? a.n_edges : e0);
            e1 = e1 < e0 ? e0 : (e1 > a.n_edges ? a.n_edges : e1);
        }
        const int deg = (int)(e1 - e0);
        seg[2 * t] = (int)e0; seg[2 * t + 1] = deg;
        inv[t] = 1.0f / (float)(deg > 0 ? deg : 1);
    }
    for (int mm = w; mm < FI_MT; mm += FI_NW) {
        float* xrow = x0n + mm * FI_D0MAX;
        if (mm >= rows) {                                       // (uniform) a row behind the last drug: zeros
            xrow[lane] = 0.f; xrow[lane + 64] = 0.f;
            continue;
        }
        const int64_t m = m0 + mm;
        int64_t s0 = a.tgt_ptr[m], s1 = a.tgt_ptr[m + 1];
        s0 = s0 < 0 ? 0 : (s0 > a.n_tgt ? a.n_tgt : s0);
        s1 = s1 < s0 ? s0 : (s1 > a.n_tgt ? a.n_tgt : s1);
        float acc = 0.f;
        for (int64_t e = s0; e < s1; ++e) {
            const int q = a.tgt_prot[e];
            if (lane < p) acc += a.h_prot[(int64_t)q * a.ld_h_prot + lane];
        }
        const float mean = acc * (1.0f / (float)(s1 > s0 ? s1 - s0 : 1));
        float v = 0.f;
        for (int j = 0; j < p; ++j) {
            const float mj = __shfl(mean, j);
            if (lane < pd) v = fmaf(mj, a.hgcn_w[(int64_t)j * pd + lane], v);
        }
        const float* xdr = a.xd + m * a.ld_xd;
        float* orow = a.x0_new + m * a.ld_x0_new;
        if (a.cat) {
            for (int c = lane; c < ne; c += TIPK_WAVE) { const float x = xdr[c]; xrow[c] = x; orow[c] = x; }
            if (lane < pd) { xrow[ne + lane] = v; orow[ne + lane] = v; }
        } else if (lane < pd) {
            const float x = xdr[lane] + v;
            xrow[lane] = x; orow[lane] = x;
        }
    }
    __syncthreads();

    const int nt1 = (d1 + 15) / 16, nt2 = (d2 + 15) / 16;
    fi_f4 acc1[FI_NTILE], acc2[FI_NTILE];
#pragma unroll
    for (int i = 0; i < FI_NTILE; ++i) { acc1[i] = fi_f4{0.f, 0.f, 0.f, 0.f}; acc2[i] = fi_f4{0.f, 0.f, 0.f, 0.f}; }

    const int half = w >> 2, wb = w & 3;
    const int mrow = lane & 15, kg = lane >> 4;
    // the aggregation's jobs: 16-column tiles of A1 (nj1 of them), then of A2; wavefront wb of its four takes wb, wb + 4, wb + 8
    const int nj1 = (d0 + 15) / 16, nj = nj1 + (d1 + 15) / 16;
    const float* jtab[FI_JOBS];
    int64_t jld[FI_JOBS];
    int jcol[FI_JOBS];
#pragma unroll
    for (int s = 0; s < FI_JOBS; ++s) {
        const int j = wb + 4 * s;
        const bool first = j < nj1;
        const int col = 16 * (first ? j : j - nj1) + mrow, wd = first ? d0 : d1;
        jtab[s] = first ? a.x0 : a.h1;
        jld[s] = first ? a.ld_x0 : a.ld_h1;
        jcol[s] = col < wd ? col : wd - 1;                      // (columns behind the row are computed and dropped)
    }
    for (int b0 = 0; b0 < B; b0 += a.nb) {
        const int nb = B - b0 < a.nb ? B - b0 : a.nb;
        const int k1 = nb * d0, k2 = nb * d1, k1p = fi_up16(k1), k2p = fi_up16(k2);
        const int lda1 = k1p + FI_PAD, lda2 = k2p + FI_PAD;
        float* A1 = img;                                        // [16][lda1]
        float* A2 = img + FI_MT * lda1;                         // [16][lda2]

        // 1. aggregate: one walk over the segment per drug
        for (int i = t; i < FI_MT * 16; i += FI_NT) {           // the columns behind k1 / k2 of every row
            const int r = i >> 4, c = i & 15;
            if (k1 + c < k1p) A1[r * lda1 + k1 + c] = 0.f;
            if (k2 + c < k2p) A2[r * lda2 + k2 + c] = 0.f;
        }
        const int bcl = mrow < nb ? mrow : nb - 1;              // rows behind the pass's bases are computed and dropped
        for (int mm = half; mm < FI_MT; mm += 2) {              // (rows behind the tile's drugs have no edge: zeros)
            const int e0 = __builtin_amdgcn_readfirstlane(seg[2 * mm]), deg = __builtin_amdgcn_readfirstlane(seg[2 * mm + 1]);
            fi_f4 agg[FI_JOBS];
#pragma unroll
            for (int s = 0; s < FI_JOBS; ++s) agg[s] = fi_f4{0.f, 0.f, 0.f, 0.f};
            for (int base = 0; base < deg; base += TIPK_WAVE) {
                const int cnt = deg - base < TIPK_WAVE ? deg - base : TIPK_WAVE;
                const int mine = lane < cnt ? lane : cnt - 1;
                const int srcv = a.in_src[(int64_t)e0 + base + mine], relv = a.in_rel[(int64_t)e0 + base + mine];
                for (int hb = 0; hb < cnt; hb += 4 * FI_KS) {   // FI_KS steps of 4 edges: their loads in flight together
                    float av1[FI_KS], av2[FI_KS], bv[FI_JOBS][FI_KS];
#pragma unroll
                    for (int ks = 0; ks < FI_KS; ++ks) {        // lane (r = lane & 15, k = lane >> 4) of a step: edge 4 ks + k
                        const int e = hb + 4 * ks + kg;
                        const bool ok = e < cnt;                // (an edge past the end: the last one, with coefficient 0)
                        const int ee = ok ? e : cnt - 1;
                        const int64_t src = __shfl(srcv, ee), rel = __shfl(relv, ee);
                        const float c1 = a.att1[rel * a.ld_att1 + b0 + bcl], c2 = a.att2[rel * a.ld_att2 + b0 + bcl];
                        av1[ks] = ok ? c1 : 0.f;
                        av2[ks] = ok ? c2 : 0.f;
#pragma unroll
                        for (int s = 0; s < FI_JOBS; ++s)
                            if (wb + 4 * s < nj) bv[s][ks] = jtab[s][src * jld[s] + jcol[s]];       // uniform
                    }
#pragma unroll
                    for (int ks = 0; ks < FI_KS; ++ks) {
                        if (hb + 4 * ks < cnt) {                // uniform
#pragma unroll
                            for (int s = 0; s < FI_JOBS; ++s)
                                if (wb + 4 * s < nj)            // uniform
                                    agg[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb + 4 * s < nj1 ? av1[ks] : av2[ks], bv[s][ks],
                                                                                  agg[s], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < FI_JOBS; ++s) {                 // rows 4 (lane >> 4) + i of the tile are bases, its columns lane & 15
                const int j = wb + 4 * s;
                if (j < nj) {
                    const bool first = j < nj1;
                    const int col = 16 * (first ? j : j - nj1) + mrow, wd = first ? d0 : d1;
                    float* dst = first ? A1 + mm * lda1 : A2 + mm * lda2;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (4 * kg + i < nb && col < wd) dst[(4 * kg + i) * wd + col] = agg[s][i];
                }
            }
        }
        __syncthreads();

        // 2. contract with the bases of the pass; lane (m = lane & 15, g = lane >> 4) holds k = k0 + 4 g + s in MFMA s of a step
        for (int st = w; st < k1p / 16; st += FI_NW) {
            const int k = st * 16 + 4 * kg;
            const float4 av = tipk_ld4(&A1[mrow * lda1 + k]);
            const float avs[4] = {av.x, av.y, av.z, av.w};
            const float* brow = a.basis1 + ((int64_t)b0 * d0 + k) * d1;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int i = 0; i < FI_NTILE; ++i) {
                    if (i < nt1) {                              // uniform
                        const int n = 16 * i + mrow;
                        const float bv = (k + s < k1 && n < d1) ? brow[(int64_t)s * d1 + n] : 0.f;
                        acc1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(avs[s], bv, acc1[i], 0, 0, 0);
                    }
                }
            }
        }
        for (int st = w; st < k2p / 16; st += FI_NW) {
            const int k = st * 16 + 4 * kg;
            const float4 av = tipk_ld4(&A2[mrow * lda2 + k]);
            const float avs[4] = {av.x, av.y, av.z, av.w};
            const float* brow = a.basis2 + ((int64_t)b0 * d1 + k) * d2;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int i = 0; i < FI_NTILE; ++i) {
                    if (i < nt2) {                              // uniform
                        const int n = 16 * i + mrow;
                        const float bv = (k + s < k2 && n < d2) ? brow[(int64_t)s * d2 + n] : 0.f;
                        acc2[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(avs[s], bv, acc2[i], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                                        // the images are free for the next pass
    }

    // 3. the wavefronts' partial tiles: part[w][layer tile][m][16], m = 4 (lane >> 4) + register, column lane & 15
    float* part = img;
    const int ntt = nt1 + nt2;
#pragma unroll
    for (int i = 0; i < FI_NTILE; ++i) {
        if (i < nt1) {
            float* dst = part + ((w * ntt + i) * FI_MT + 4 * kg) * 16 + mrow;
            dst[0] = acc1[i][0]; dst[16] = acc1[i][1]; dst[32] = acc1[i][2]; dst[48] = acc1[i][3];
        }
        if (i < nt2) {
            float* dst = part + ((w * ntt + nt1 + i) * FI_MT + 4 * kg) * 16 + mrow;
            dst[0] = acc2[i][0]; dst[16] = acc2[i][1]; dst[32] = acc2[i][2]; dst[48] = acc2[i][3];
        }
    }
    __syncthreads();
    const int wstride = ntt * FI_MT * 16;
    auto total = [&](int tile, int mm, int c) {
        const float* q = part + (tile * FI_MT + mm) * 16 + c;
        return ((q[0] + q[wstride]) + (q[2 * wstride] + q[3 * wstride])) +
               ((q[4 * wstride] + q[5 * wstride]) + (q[6 * wstride] + q[7 * wstride]));
    };
    for (int i = t; i < FI_MT * d1; i += FI_NT) {
        const int mm = i / d1, n = i - mm * d1;
        const float* xrow = x0n + mm * FI_D0MAX;
        float own = 0.f;
        for (int c = 0; c < d0; ++c) own = fmaf(xrow[c], a.root1[(int64_t)c * d1 + n], own);
        float v = inv[mm] * total(n >> 4, mm, n & 15) + own;
        v = v > 0.f ? v : 0.f;
        h1n[mm * FI_DMAX + n] = v;
        if (mm < rows) a.h1_new[(m0 + mm) * a.ld_h1_new + n] = v;
    }
    __syncthreads();
    for (int i = t; i < FI_MT * d2; i += FI_NT) {
        const int mm = i / d2, n = i - mm * d2;
        const float* hrow = h1n + mm * FI_DMAX;
        float own = 0.f;
        for (int c = 0; c < d1; ++c) own = fmaf(hrow[c], a.root2[(int64_t)c * d2 + n], own);
        if (mm < rows) a.z_new[(m0 + mm) * a.ld_z_new + n] = inv[mm] * total(nt1 + (n >> 4), mm, n & 15) + own;
    }
}

int fi_d0(int ne, int pd, int cat) { return cat ? ne + pd : ne; }

// bases per pass: as many of 16 as the images' LDS takes (at least one does at the largest widths)
int fi_pass_bases(int n_bases, int d0, int d1) {
    int nb = n_bases < FI_NB ? n_bases : FI_NB;
    while (nb > 1 && fi_images(nb, d0, d1) > FI_A_FLOATS) --nb;
    return nb;
}

// new drugs per workgroup: all 16 rows of the MFMA tile once that still gives every CU a workgroup; fewer (an even number: both
// halves of the wavefronts busy) down to one for small calls, so that a few drugs with long segments spread over the chip
int fi_tile_drugs(int64_t n_new) {
    if (n_new <= 256) return 1;
    const int64_t t = 2 * tipk_ceil_div(n_new, 512);
    return t < FI_MT ? (int)t : FI_MT;
}

}  // namespace

extern "C" int tipk_drug_fold_in_supported(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int p, int pd,
                                           int d1, int d2, int cat) {
    if (n_nodes < 1 || n_nodes > 0x7fffffffLL || n_prot < 1 || n_prot > 0x7fffffffLL || n_rel < 1 || n_rel > FI_RMAX) return 0;
    if (n_bases < 1 || n_bases > FI_DMAX || p < 1 || p > FI_DMAX || pd < 1 || pd > FI_DMAX || d1 < 1 || d1 > FI_DMAX ||
        d2 < 1 || d2 > FI_DMAX || ne < 1 || ne > FI_D0MAX)
        return 0;
    if (!cat && ne != pd) return 0;
    return fi_d0(ne, pd, cat) <= FI_D0MAX;
}

extern "C" int64_t tipk_drug_fold_in_workspace_bytes(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int p,
                                                     int pd, int d1, int d2, int cat, int64_t n_new, int64_t n_edges) {
    if (n_new < 0 || n_edges < 0 || !tipk_drug_fold_in_supported(n_nodes, n_prot, n_rel, n_bases, ne, p, pd, d1, d2, cat))
        return -1;
    return 0;                                                   // every sum is finished inside its workgroup
}

extern "C" int tipk_drug_fold_in(const float* h_prot, int64_t ld_h_prot, int64_t n_prot, int p, const float* hgcn_w, int pd,
                                 const float* x0, int64_t ld_x0, const float* h1, int64_t ld_h1, int64_t n_nodes,
                                 const float* basis1, const float* att1, int64_t ld_att1, const float* root1,
                                 const float* basis2, const float* att2, int64_t ld_att2, const float* root2, int64_t n_rel,
                                 int n_bases, int d1, int d2, const float* xd, int64_t ld_xd, int ne, int cat,
                                 const int64_t* tgt_ptr, const int32_t* tgt_prot, int64_t n_tgt, const int64_t* in_ptr,
                                 const int32_t* in_src, const int32_t* in_rel, int64_t n_edges, int64_t n_new, float* x0_new,
                                 int64_t ld_x0_new, float* h1_new, int64_t ld_h1_new, float* z_new, int64_t ld_z_new,
                                 void* workspace, tipk_stream_t stream) {
    (void)workspace;
    if (n_new < 0 || n_tgt < 0 || n_edges < 0 || n_nodes < 1 || n_prot < 1 || n_rel < 1 || n_bases < 1 || p < 1 || pd < 1 ||
        ne < 1 || d1 < 1 || d2 < 1)
        return TIPK_EINVAL;
    if (!cat && ne != pd) return TIPK_EINVAL;
    const int64_t d0 = (int64_t)ne + (cat ? pd : 0);
    if (ld_h_prot < p || ld_x0 < d0 || ld_h1 < d1 || ld_att1 < n_bases || ld_att2 < n_bases || ld_xd < ne || ld_x0_new < d0 ||
        ld_h1_new < d1 || ld_z_new < d2)
        return TIPK_EINVAL;
    if (n_new > 0 && (!h_prot || !hgcn_w || !x0 || !h1 || !basis1 || !att1 || !root1 || !basis2 || !att2 || !root2 || !xd ||
                      !tgt_ptr || !in_ptr || !x0_new || !h1_new || !z_new || (n_tgt > 0 && !tgt_prot) ||
                      (n_edges > 0 && (!in_src || !in_rel))))
        return TIPK_EINVAL;
    if (!tipk_drug_fold_in_supported(n_nodes, n_prot, n_rel, n_bases, ne, p, pd, d1, d2, cat)) return TIPK_EUNSUPPORTED;
    if (n_edges > 0x7fffffffLL || n_tgt > 0x7fffffffLL || n_new > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if (n_new == 0) return TIPK_OK;

    FoldArgs a;
    a.h_prot = h_prot; a.hgcn_w = hgcn_w; a.x0 = x0; a.h1 = h1; a.basis1 = basis1; a.att1 = att1; a.root1 = root1;
    a.basis2 = basis2; a.att2 = att2; a.root2 = root2; a.xd = xd;
    a.tgt_ptr = tgt_ptr; a.in_ptr = in_ptr; a.tgt_prot = tgt_prot; a.in_src = in_src; a.in_rel = in_rel;
    a.ld_h_prot = ld_h_prot; a.ld_x0 = ld_x0; a.ld_h1 = ld_h1; a.ld_att1 = ld_att1; a.ld_att2 = ld_att2; a.ld_xd = ld_xd;
    a.n_tgt = n_tgt; a.n_edges = n_edges; a.n_new = n_new;
    a.ld_x0_new = ld_x0_new; a.ld_h1_new = ld_h1_new; a.ld_z_new = ld_z_new;
    a.p = p; a.pd = pd; a.ne = ne; a.d0 = (int)d0; a.d1 = d1; a.d2 = d2; a.n_bases = n_bases; a.cat = cat != 0;
    a.nb = fi_pass_bases(n_bases, a.d0, d1);
    a.tile = fi_tile_drugs(n_new);
    a.x0_new = x0_new; a.h1_new = h1_new; a.z_new = z_new;
    // the images of the widest pass, or the eight wavefronts' partial tiles that take their place
    int64_t shared = fi_images(a.nb, a.d0, d1);
    const int64_t parts = (int64_t)FI_NW * ((d1 + 15) / 16 + (d2 + 15) / 16) * FI_MT * 16;
    if (parts > shared) shared = parts;
    const size_t lds = (size_t)(FI_MT * FI_D0MAX + FI_MT * FI_DMAX + FI_MT + 2 * FI_MT + shared) * 4;
    hipError_t e = hipFuncSetAttribute((const void*)fold_in_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(fold_in_kernel, dim3((unsigned)tipk_ceil_div(n_new, a.tile)), dim3(FI_NT), lds, (hipStream_t)stream, a);
    TIPK_RETURN_LAUNCH();
}
