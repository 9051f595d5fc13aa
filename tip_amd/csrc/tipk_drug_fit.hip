// Fit of the embedding of NEW drugs to their recorded (partner, side effect) reports, embeddings and DistMult decoder frozen
// (include/tipk.h section 4q): the statistics (loss, gradient, Hessian) of the expected training objective at trial rows, and
// an entry that enqueues max_iter + 1 (statistics, tipk_newton_step) pairs.  The dual of tipk_side_effect_fit.hip (4m): there
// the unknown is a decoder row and a term is a pair of drugs, here the unknown is an embedding row and a term is a CELL
// (partner v, side effect r) with the feature f = z[v] * rel_w[r].
//
// Statistics, launch 1, drug_dense_kernel: the negative sum as a mask-free stream over ALL n x R cells in RECTANGULAR tiles of
//   64 partners x 64 side effects, numbered partner-block major.  A workgroup (4 wavefronts) takes a SLAB -- a contiguous range
//   of tiles -- and a block of DF_XB new drugs; the tile's z rows and rel_w rows rest in LDS (16-byte aligned, row stride
//   width + 4 floats: off every multiple of 32 banks); the z rows are staged again only when the partner block changes.
//   Wavefront w owns the partners v = 16 w .. 16 w + 15 of the tile; per partner:
//     A. lane = side effect r.  f = z[v] * rel_w[r] rounded once per component, the logit of drug x the fmaf chain over k
//        ascending from +0.0f; the terms from one expf (sf_terms of tipk_fit_terms.h).  The lane adds dense_w softplus to its
//        loss and leaves (dense_w sigma, dense_w sigma') per drug in the wavefront's LDS rows.  The feature is computed ONCE
//        per cell for the block's drugs.
//     B. lane = (component c = lane & 15, cell slot k = lane >> 4): 16 steps of four cells on v_mfma_f32_16x16x4_f32 with the
//        cells as K.  Gradient of all drugs of the block in ONE product (row i of A is drug i), the Hessian of drug x as
//        (sigma' f) f^T per 16 x 16 tile.  The rel_w operands of the 16 steps stay in registers for the tile.
//   The accumulators stay in registers over the slab; at its end every wavefront writes its partial (loss, g, H) to the
//   workspace: part[drug block][slab][wavefront][drug][1 + dim + dim^2].
// Launch 2, drug_finish_kernel: one workgroup per drug sums the 4 * slabs partials of every output in ascending (slab,
//   wavefront) order, adds the sparse correction over the drug's distinct recorded cells (chunks of 256 cells: a chain from
//   +0.0f inside the chunk in list order, the chunks added in ascending order) and the l2 terms around the prior centre.
// A block whose drugs are all inactive returns at once; inactive rows of the outputs are not touched.
// No atomics, no workgroup waits for another, every trip count depends on sizes and list lengths only: BITWISE repeatable.
// The step is tipk_newton_step of 4m, called through its C entry as it is.
#include "tipk_chol.h"
#include "tipk_fit_terms.h"

namespace {

constexpr int DF_NT = 256;                  // threads of a dense workgroup
constexpr int DF_NW = DF_NT / TIPK_WAVE;    // 4 wavefronts: 16 partners of the tile each
constexpr int DF_TILE = 64;
constexpr int DF_XB = 4;                    // new drugs per workgroup: the register block
constexpr int DF_PAD = 4;                   // floats behind a row of the LDS images
constexpr int DF_CW = 2 * DF_XB + 4;        // floats of a lane's coefficient row: 8 used; 12 words apart, the 16-byte stores of
                                            // 8 consecutive lanes fall on 32 different banks
constexpr int DF_CH = 256;                  // recorded cells per chunk of the sparse pass
constexpr int DF_LB = 16;                   // partials a thread of the finish loads before it adds them
constexpr int DF_DMAX = CH_DMAX;
constexpr int64_t DF_CELLMAX = 0x7fffffffLL;            // n * R must stay below 2^31
constexpr int64_t DF_FITMAX = 65536;
constexpr int64_t DF_TARGET_WGS = 1024;     // dense workgroups to aim for: four per CU
constexpr int DF_EPT = (1 + DF_DMAX + DF_DMAX * DF_DMAX + DF_CH - 1) / DF_CH;   // outputs per thread of the finish

struct DrugStatsArgs {
    const float *z, *rel_w, *x, *dense_w, *prior;
    const int64_t* rec_ptr;
    const int32_t *rec_v, *rec_r;
    const float *rec_wpos, *rec_wneg;
    const int32_t* active;
    float l2;
    int n, n_rel, dim, TR, slabs;
    int64_t n_fit, n_tiles, tps;
    float* part;
    float *loss, *grad, *hess;
};

template <int DP>
__global__ void __launch_bounds__(DF_NT) drug_dense_kernel(DrugStatsArgs a) {
    constexpr int NH = DP / 16;
    constexpr int LD = DP + DF_PAD;
    __shared__ __attribute__((aligned(16))) float Zp[DF_TILE * LD];         // z rows of the tile's partners
    __shared__ __attribute__((aligned(16))) float Wr[DF_TILE * LD];         // rel_w rows of the tile's side effects
    __shared__ __attribute__((aligned(16))) float Xs[DF_XB * DP];           // the block's trial rows
    __shared__ __attribute__((aligned(16))) float coef[DF_NW][TIPK_WAVE][DF_CW];

    const int t = threadIdx.x, lane = tipk_lane(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, n_rel = a.n_rel, dim = a.dim;
    const int64_t db = blockIdx.y, slab = blockIdx.x, j0 = db * DF_XB;

    bool any = false;
    float dw[DF_XB];
#pragma unroll
    for (int x = 0; x < DF_XB; ++x) {
        const int64_t j = j0 + x;
        const bool in = j < a.n_fit;
        dw[x] = in ? a.dense_w[j] : 0.f;
        any = any || (in && (!a.active || a.active[j] != 0));
    }
    if (!any) return;                                           // uniform in the workgroup

    for (int i = t; i < DF_XB * DP; i += DF_NT) {
        const int x = i / DP, c = i - x * DP;
        const int64_t j = j0 + x;
        Xs[i] = (j < a.n_fit && c < dim) ? a.x[j * dim + c] : 0.f;
    }

    sf_f4 H[DF_XB][NH][NH], G[NH];
    float lacc[DF_XB];
#pragma unroll
    for (int x = 0; x < DF_XB; ++x) {
        lacc[x] = 0.f;
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int hj = 0; hj < NH; ++hj) H[x][hi][hj] = sf_f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) G[h] = sf_f4{0.f, 0.f, 0.f, 0.f};

    const int64_t t0 = slab * a.tps, t1 = t0 + a.tps < a.n_tiles ? t0 + a.tps : a.n_tiles;
    int pb = (int)(t0 / a.TR), rb = (int)(t0 - (int64_t)pb * a.TR), staged = -1;
    const int cc = lane & 15, kk = lane >> 4;

    for (int64_t tt = t0; tt < t1; ++tt) {
        __syncthreads();                                        // the previous tile has been read; Xs is staged
        const bool fresh = staged != pb;                        // uniform
        for (int i = t; i < DF_TILE * (DP / 4); i += DF_NT) {
            const int r = i / (DP / 4), q = i - r * (DP / 4);
            const int64_t rp = (int64_t)pb * DF_TILE + r, rr = (int64_t)rb * DF_TILE + r;
            float4 xp = make_float4(0.f, 0.f, 0.f, 0.f), xr = xp;
            if (4 * q < dim) {
                if (fresh && rp < n) xp = tipk_ld4(a.z + rp * dim + 4 * q);
                if (rr < n_rel) xr = tipk_ld4(a.rel_w + rr * dim + 4 * q);
            }
            if (fresh) tipk_st4(&Zp[r * LD + 4 * q], xp);
            tipk_st4(&Wr[r * LD + 4 * q], xr);
        }
        staged = pb;
        __syncthreads();

        float wra[DP];                                          // phase A: the lane's own side effect
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
            const float4 x4 = tipk_ld4(&Wr[lane * LD + 4 * q]);
            wra[4 * q] = x4.x; wra[4 * q + 1] = x4.y; wra[4 * q + 2] = x4.z; wra[4 * q + 3] = x4.w;
        }
        float wrb[16][NH];                                      // phase B: component c of the four side effects of every step
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int h = 0; h < NH; ++h) wrb[s][h] = Wr[(4 * s + kk) * LD + 16 * h + cc];

        const bool valid = (int64_t)rb * DF_TILE + lane < n_rel;
        for (int vr = 0; vr < 16; ++vr) {
            const int vv = wave * 16 + vr;
            if ((int64_t)pb * DF_TILE + vv >= n) break;         // uniform in the wavefront

            // A. logits and coefficients, lane = side effect
            float f[DP];
#pragma unroll
            for (int q = 0; q < DP / 4; ++q) {
                const float4 x4 = tipk_ld4(&Zp[vv * LD + 4 * q]);
                f[4 * q] = x4.x * wra[4 * q]; f[4 * q + 1] = x4.y * wra[4 * q + 1];
                f[4 * q + 2] = x4.z * wra[4 * q + 2]; f[4 * q + 3] = x4.w * wra[4 * q + 3];
            }
            float ca[DF_XB], ch[DF_XB];
#pragma unroll
            for (int x = 0; x < DF_XB; ++x) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < DP / 4; ++q) {
                    const float4 x4 = tipk_ld4(&Xs[x * DP + 4 * q]);
                    s = fmaf(f[4 * q], x4.x, s); s = fmaf(f[4 * q + 1], x4.y, s);
                    s = fmaf(f[4 * q + 2], x4.z, s); s = fmaf(f[4 * q + 3], x4.w, s);
                }
                float sp, sig, h;
                sf_terms(s, sp, sig, h);
                if (valid) lacc[x] += dw[x] * sp;
                ca[x] = valid ? dw[x] * sig : 0.f;
                ch[x] = valid ? dw[x] * h : 0.f;
            }
            tipk_st4(&coef[wave][lane][0], make_float4(ca[0], ca[1], ca[2], ca[3]));
            tipk_st4(&coef[wave][lane][4], make_float4(ch[0], ch[1], ch[2], ch[3]));
            sf_wave_sync();

            // B. four cells per MFMA, lane = (component, cell slot)
            float zp[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) zp[h] = Zp[vv * LD + 16 * h + cc];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float4 a4 = tipk_ld4(&coef[wave][4 * s + kk][0]);
                const float4 h4 = tipk_ld4(&coef[wave][4 * s + kk][4]);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
                float fb[NH];
#pragma unroll
                for (int h = 0; h < NH; ++h) fb[h] = zp[h] * wrb[s][h];
                const float ga = cc == 0 ? av[0] : cc == 1 ? av[1] : cc == 2 ? av[2] : cc == 3 ? av[3] : 0.f;
#pragma unroll
                for (int h = 0; h < NH; ++h) G[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, fb[h], G[h], 0, 0, 0);
#pragma unroll
                for (int x = 0; x < DF_XB; ++x)
#pragma unroll
                    for (int hi = 0; hi < NH; ++hi) {
                        const float ha = hv[x] * fb[hi];
#pragma unroll
                        for (int hj = 0; hj < NH; ++hj)
                            H[x][hi][hj] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha, fb[hj], H[x][hi][hj], 0, 0, 0);
                    }
            }
            sf_wave_sync();                                     // the coefficient rows are free for the next partner
        }
        if (++rb == a.TR) { rb = 0; ++pb; }
    }

    // the wavefront's partials: part[db][slab][wave][x][1 + dim + dim^2]
    const int64_t E = sf_elems(dim);
    float* base = a.part + (((db * a.slabs + slab) * DF_NW + wave) * DF_XB) * E;
#pragma unroll
    for (int x = 0; x < DF_XB; ++x) {
        float p = lacc[x];
#pragma unroll
        for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) p += __shfl_down(p, off);
        float* o = base + x * E;
        if (lane == 0) o[0] = p;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (kk == 0 && 16 * h + cc < dim) o[1 + 16 * h + cc] = G[h][x];      // row x of the gradient product
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int hj = 0; hj < NH; ++hj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * hi + 4 * kk + r, col = 16 * hj + cc;
                    if (row < dim && col < dim) o[1 + dim + row * dim + col] = H[x][hi][hj][r];
                }
    }
}

__global__ void __launch_bounds__(DF_CH) drug_finish_kernel(DrugStatsArgs a) {
    __shared__ float fs[DF_CH][DF_DMAX + 1];
    __shared__ float cs[DF_CH][3];
    const int t = threadIdx.x, dim = a.dim;
    const int64_t j = blockIdx.x;
    if (a.active && a.active[j] == 0) return;                   // uniform
    const int64_t E = sf_elems(dim);
    const int64_t db = j / DF_XB, x = j - db * DF_XB;

    float tot[DF_EPT];                                          // output e = t + 256 i: the dense slabs in ascending order
#pragma unroll
    for (int i = 0; i < DF_EPT; ++i) {
        const int64_t e = t + (int64_t)DF_CH * i;
        float s = 0.f;
        if (e < E) {
            const float* p = a.part + ((db * a.slabs * DF_NW) * DF_XB + x) * E + e;
            const int64_t np = (int64_t)a.slabs * DF_NW, step = DF_XB * E;
            int64_t q = 0;
            for (; q + DF_LB <= np; q += DF_LB) {               // DF_LB loads in flight, then added in the same order:
                float v[DF_LB];                                 // one round trip to L2 per batch, not per partial
#pragma unroll
                for (int u = 0; u < DF_LB; ++u) v[u] = p[(q + u) * step];
#pragma unroll
                for (int u = 0; u < DF_LB; ++u) s += v[u];
            }
            for (; q < np; ++q) s += p[q * step];
        }
        tot[i] = s;
    }

    float sparse[DF_EPT];
#pragma unroll
    for (int i = 0; i < DF_EPT; ++i) sparse[i] = 0.f;
    const int64_t p0 = a.rec_ptr[j], p1 = a.rec_ptr[j + 1];
    const float* xr = a.x + j * dim;
    for (int64_t c0 = p0; c0 < p1; c0 += DF_CH) {
        const int cnt = p1 - c0 < DF_CH ? (int)(p1 - c0) : DF_CH;
        __syncthreads();                                        // the previous chunk has been read
        if (t < cnt) {
            int v = a.rec_v[c0 + t], r = a.rec_r[c0 + t];
            v = v < 0 ? 0 : (v >= a.n ? a.n - 1 : v);           // (ids in range are the caller's contract; nothing is
            r = r < 0 ? 0 : (r >= a.n_rel ? a.n_rel - 1 : r);   //  read out of bounds)
            const float* zv = a.z + (int64_t)v * dim;
            const float* wr = a.rel_w + (int64_t)r * dim;
            float s = 0.f;
            for (int k = 0; k < dim; ++k) {
                const float f = zv[k] * wr[k];
                fs[t][k] = f;
                s = fmaf(f, xr[k], s);
            }
            float sp, spn, sig, sigm, h, hm;
            sf_terms(s, sp, sig, h);
            sf_terms(-s, spn, sigm, hm);                        // hm == h
            const float wp = a.rec_wpos[c0 + t], wn = a.rec_wneg[c0 + t];
            cs[t][0] = wp * spn - wn * sp;
            cs[t][1] = -wp * sigm - wn * sig;
            cs[t][2] = (wp - wn) * h;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < DF_EPT; ++i) {
            const int64_t e = t + (int64_t)DF_CH * i;
            if (e >= E) continue;
            float acc = 0.f;
            if (e == 0) {
                for (int p = 0; p < cnt; ++p) acc += cs[p][0];
            } else if (e <= dim) {
                const int k = (int)e - 1;
                for (int p = 0; p < cnt; ++p) acc = fmaf(cs[p][1], fs[p][k], acc);
            } else {
                const int r = (int)(e - 1 - dim) / dim, c = (int)(e - 1 - dim) - r * dim;
                for (int p = 0; p < cnt; ++p) acc = fmaf(cs[p][2] * fs[p][r], fs[p][c], acc);
            }
            sparse[i] += acc;
        }
    }

    const float* pr = a.prior ? a.prior + j * dim : nullptr;    // the l2 terms pull to the prior centre c (NULL: 0)
#pragma unroll
    for (int i = 0; i < DF_EPT; ++i) {
        const int64_t e = t + (int64_t)DF_CH * i;
        if (e >= E) continue;
        const float val = tot[i] + sparse[i];
        if (e == 0) {
            float dd = 0.f;
            for (int k = 0; k < dim; ++k) {
                const float d = xr[k] - (pr ? pr[k] : 0.f);
                dd = fmaf(d, d, dd);
            }
            a.loss[j] = val + 0.5f * a.l2 * dd;
        } else if (e <= dim) {
            a.grad[j * dim + e - 1] = val + a.l2 * (xr[e - 1] - (pr ? pr[e - 1] : 0.f));
        } else {
            const int64_t q = e - 1 - dim;
            a.hess[j * dim * dim + q] = (q / dim == q % dim) ? val + a.l2 : val;
        }
    }
}

struct DrugInitArgs {
    const float *init, *prior;
    float *x, *x_trial, *loss, *grad, *p, *t;
    int32_t *info, *active;
    int64_t n_fit;
    int dim;
};

__global__ void __launch_bounds__(256) drug_init_kernel(DrugInitArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_fit * a.dim) {
        const float v = a.init ? a.init[i] : (a.prior ? a.prior[i] : 0.f);
        a.x[i] = v; a.x_trial[i] = v; a.grad[i] = 0.f; a.p[i] = 0.f;
    }
    if (i < a.n_fit) {
        a.loss[i] = 0.f; a.t[i] = 1.0f; a.active[i] = 1;
        a.info[4 * i] = 0; a.info[4 * i + 1] = 0; a.info[4 * i + 2] = 0; a.info[4 * i + 3] = 0;
    }
}

struct DrugShape {
    int TR, slabs;
    int64_t n_tiles, tps, n_db;
};

DrugShape df_shape(int64_t n_nodes, int64_t n_rel, int64_t n_fit) {
    DrugShape s;
    s.TR = (int)tipk_ceil_div(n_rel, DF_TILE);
    s.n_tiles = tipk_ceil_div(n_nodes, DF_TILE) * s.TR;
    s.n_db = tipk_ceil_div(n_fit < 1 ? 1 : n_fit, DF_XB);
    int64_t want = tipk_ceil_div(DF_TARGET_WGS, s.n_db);
    if (want > s.n_tiles) want = s.n_tiles;
    if (want > 65535) want = 65535;
    s.tps = tipk_ceil_div(s.n_tiles, want);
    s.slabs = (int)tipk_ceil_div(s.n_tiles, s.tps);
    return s;
}

// workspace: [dense partials] then the state of tipk_distmult_drug_fit
struct DrugLayout {
    int64_t part, p, t, x_trial, active, s_loss, s_grad, s_hess, total;
};

DrugLayout df_layout(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    const DrugShape s = df_shape(n_nodes, n_rel, n_fit);
    DrugLayout l;
    int64_t o = 0;
    l.part = o; o += sf_a256(s.n_db * s.slabs * DF_NW * DF_XB * sf_elems(dim) * 4);
    l.p = o; o += sf_a256(n_fit * dim * 4);
    l.t = o; o += sf_a256(n_fit * 4);
    l.x_trial = o; o += sf_a256(n_fit * dim * 4);
    l.active = o; o += sf_a256(n_fit * 4);
    l.s_loss = o; o += sf_a256(n_fit * 4);
    l.s_grad = o; o += sf_a256(n_fit * dim * 4);
    l.s_hess = o; o += sf_a256(n_fit * dim * dim * 4);
    l.total = o;
    return l;
}

int df_stats_check(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel, const float* x, int64_t n_fit,
                   const float* dense_w, const int64_t* rec_ptr, const int32_t* rec_v, const int32_t* rec_r,
                   const float* rec_wpos, const float* rec_wneg, int64_t n_rec, float l2, const float* loss, const float* grad,
                   const float* hess, const void* workspace) {
    if (n_nodes < 1 || n_rel < 1 || dim < 1 || n_fit < 0 || n_rec < 0 || !(l2 >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!z || !rel_w || !x || !dense_w || !rec_ptr || !loss || !grad || !hess || !workspace)) return TIPK_EINVAL;
    if (n_fit > 0 && n_rec > 0 && (!rec_v || !rec_r || !rec_wpos || !rec_wneg)) return TIPK_EINVAL;
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit > 0 ? n_fit : 1)) return TIPK_EUNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(rel_w)) & 15) != 0) return TIPK_EUNSUPPORTED;
    return TIPK_OK;
}

int df_stats_launch(DrugStatsArgs& a, hipStream_t st) {
    const DrugShape s = df_shape(a.n, a.n_rel, a.n_fit);
    a.TR = s.TR; a.slabs = s.slabs; a.n_tiles = s.n_tiles; a.tps = s.tps;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.n_db);
    if (a.dim <= 16) hipLaunchKernelGGL(drug_dense_kernel<16>, grid, dim3(DF_NT), 0, st, a);
    else hipLaunchKernelGGL(drug_dense_kernel<32>, grid, dim3(DF_NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(drug_finish_kernel, dim3((unsigned)a.n_fit), dim3(DF_CH), 0, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_distmult_drug_fit_supported(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    return n_nodes >= 1 && n_rel >= 1 && n_nodes <= DF_CELLMAX && n_rel <= DF_CELLMAX && n_nodes * n_rel <= DF_CELLMAX &&
           dim >= 4 && dim <= DF_DMAX && dim % 4 == 0 && n_fit >= 1 && n_fit <= DF_FITMAX;
}

extern "C" int64_t tipk_distmult_drug_fit_slabs(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit)) return -1;
    return df_shape(n_nodes, n_rel, n_fit).slabs;
}

extern "C" int64_t tipk_distmult_drug_fit_max_chain(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit)) return -1;
    const DrugShape s = df_shape(n_nodes, n_rel, n_fit);
    // dense: 16 partners x 64 cells per tile and wavefront in one accumulator chain over the slab, then the 4 * slabs partials;
    // sparse: 256 cells in a chunk, then the chunks of at most n R distinct cells; + the sparse total, + l2
    const int64_t dense = s.tps * 16 * DF_TILE + 6 + (int64_t)s.slabs * DF_NW;
    const int64_t sparse = DF_CH + tipk_ceil_div(n_nodes * n_rel, DF_CH);
    return (dense > sparse ? dense : sparse) + 2;
}

extern "C" int64_t tipk_distmult_drug_fit_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    if (n_fit == 0 && tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, 1)) return 0;
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit)) return -1;
    return df_layout(n_nodes, dim, n_rel, n_fit).total;
}

extern "C" int tipk_distmult_drug_fit_stats(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                            const float* x, int64_t n_fit, const float* dense_w, const int64_t* rec_ptr,
                                            const int32_t* rec_v, const int32_t* rec_r, const float* rec_wpos,
                                            const float* rec_wneg, int64_t n_rec, const float* prior, float l2,
                                            const int32_t* active, float* loss, float* grad, float* hess, void* workspace,
                                            tipk_stream_t stream) {
    const int bad = df_stats_check(z, n_nodes, dim, rel_w, n_rel, x, n_fit, dense_w, rec_ptr, rec_v, rec_r, rec_wpos, rec_wneg,
                                   n_rec, l2, loss, grad, hess, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_fit == 0) return TIPK_OK;
    DrugStatsArgs a;
    a.z = z; a.rel_w = rel_w; a.x = x; a.dense_w = dense_w; a.prior = prior; a.rec_ptr = rec_ptr; a.rec_v = rec_v;
    a.rec_r = rec_r; a.rec_wpos = rec_wpos; a.rec_wneg = rec_wneg; a.active = active; a.l2 = l2; a.n = (int)n_nodes;
    a.n_rel = (int)n_rel; a.dim = dim; a.n_fit = n_fit; a.part = reinterpret_cast<float*>(workspace); a.loss = loss;
    a.grad = grad; a.hess = hess;
    return df_stats_launch(a, (hipStream_t)stream);
}

extern "C" int tipk_distmult_drug_fit(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel, int64_t n_fit,
                                      const float* dense_w, const int64_t* rec_ptr, const int32_t* rec_v, const int32_t* rec_r,
                                      const float* rec_wpos, const float* rec_wneg, int64_t n_rec, const float* prior, float l2,
                                      const float* init, int max_iter, float gtol, float* out_x, float* out_loss,
                                      float* out_grad, int32_t* out_info, float* out_hess, void* workspace,
                                      tipk_stream_t stream) {
    if (max_iter < 0 || !(gtol >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!out_x || !out_info)) return TIPK_EINVAL;
    const int bad = df_stats_check(z, n_nodes, dim, rel_w, n_rel, out_x, n_fit, dense_w, rec_ptr, rec_v, rec_r, rec_wpos,
                                   rec_wneg, n_rec, l2, out_loss, out_grad, out_loss, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_fit == 0) return TIPK_OK;
    const DrugLayout l = df_layout(n_nodes, dim, n_rel, n_fit);
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;

    DrugInitArgs ia;
    ia.init = init; ia.prior = prior; ia.x = out_x; ia.x_trial = reinterpret_cast<float*>(ws + l.x_trial); ia.loss = out_loss;
    ia.grad = out_grad; ia.p = reinterpret_cast<float*>(ws + l.p); ia.t = reinterpret_cast<float*>(ws + l.t);
    ia.info = out_info; ia.active = reinterpret_cast<int32_t*>(ws + l.active); ia.n_fit = n_fit; ia.dim = dim;
    hipLaunchKernelGGL(drug_init_kernel, dim3((unsigned)tipk_ceil_div(n_fit * dim, 256)), dim3(256), 0, st, ia);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);

    DrugStatsArgs a;
    a.z = z; a.rel_w = rel_w; a.x = ia.x_trial; a.dense_w = dense_w; a.prior = prior; a.rec_ptr = rec_ptr; a.rec_v = rec_v;
    a.rec_r = rec_r; a.rec_wpos = rec_wpos; a.rec_wneg = rec_wneg; a.active = ia.active; a.l2 = l2; a.n = (int)n_nodes;
    a.n_rel = (int)n_rel; a.dim = dim; a.n_fit = n_fit; a.part = reinterpret_cast<float*>(ws + l.part);
    a.loss = reinterpret_cast<float*>(ws + l.s_loss); a.grad = reinterpret_cast<float*>(ws + l.s_grad);
    a.hess = reinterpret_cast<float*>(ws + l.s_hess);
    for (int it = 0; it <= max_iter; ++it) {
        int status = df_stats_launch(a, st);
        if (status != TIPK_OK) return status;
        status = tipk_newton_step(dim, n_fit, a.loss, a.grad, a.hess, gtol, out_x, out_loss, out_grad, ia.p, ia.t, out_info,
                                  ia.x_trial, ia.active, stream);
        if (status != TIPK_OK) return status;
    }
    if (out_hess) {                                             // the Hessian of the accepted rows: one more statistics pair
        a.x = out_x; a.active = nullptr; a.hess = out_hess;     // (its loss and gradient go to the spent statistics slots)
        return df_stats_launch(a, st);
    }
    return TIPK_OK;
}
