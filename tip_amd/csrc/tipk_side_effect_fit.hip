// Fit of DistMult decoder rows for NEW side effects on the frozen embeddings (include/tipk.h section 4m): the statistics
// (loss, gradient, Hessian) of the expected training objective at trial rows, one damped Newton step per call, and an entry
// that enqueues max_iter + 1 (statistics, step) pairs.
//
// Statistics, launch 1, fit_dense_kernel: the negative sum over ALL ordered pairs as a mask-free stream over the unordered
//   pairs u <= v in tiles of 64 x 64 (v-block >= u-block; the diagonal tile masked to u <= v), ordered multiplicity 2 (1 for
//   u == v).  A workgroup (4 wavefronts) takes a SLAB -- a contiguous range of tiles -- and a block of SF_RB relations; both
//   row blocks of a tile rest in LDS (16-byte aligned, row stride width + 4 floats: off every multiple of 32 banks).
//   Wavefront w owns the rows u = 16 w .. 16 w + 15 of the tile; per row:
//     A. lane = v.  f = z[u] * z[v] rounded once per component, the logit of relation x the fmaf chain over k ascending from
//        +0.0f; e = expf(-|s|), r = 1 / (1 + e): softplus(s) = max(s, 0) + log1pf(e), sigma(s) = r | e r, sigma' = e r r.
//        The lane adds m dense_w softplus to its loss and leaves (m dense_w sigma, m dense_w sigma') per relation in the
//        wavefront's LDS rows.  The feature is computed ONCE per pair for the block's relations.
//     B. lane = (component c = lane & 15, pair slot k = lane >> 4): 16 steps of four pairs on v_mfma_f32_16x16x4_f32 with
//        the pairs as K.  Gradient of all relations of the block in ONE product (row i of A is relation i), the Hessian of
//        relation x as (sigma' f) f^T per 16 x 16 tile.  The z[v] operands of the 16 steps stay in registers for the tile.
//   The accumulators stay in registers over the slab; at its end every wavefront writes its partial (loss, g, H) to the
//   workspace: part[relation block][slab][wavefront][relation][1 + dim + dim^2].
// Launch 2, fit_finish_kernel: one workgroup per relation sums the 4 * slabs partials of every output in ascending (slab,
//   wavefront) order, adds the sparse correction over the relation's distinct recorded pairs (chunks of 256 pairs: a chain
//   from +0.0f inside the chunk in list order, the chunks added in ascending order) and the l2 terms, and writes the outputs.
// A block whose relations are all inactive returns at once; inactive rows of the outputs are not touched.
// No atomics, no workgroup waits for another, every trip count depends on sizes and list lengths only: BITWISE repeatable.
//
// Step, newton_step_kernel: one wavefront per relation; lane j owns component j.  Armijo test with 16 ulp slack, Cholesky of
//   the trial Hessian in LDS (ch_factor of tipk_chol.h: right-looking, column k by the lanes i > k), the two triangular
//   solves with the vector in registers (one shuffle per column); a pivot that is not > 0 gives the scaled steepest-descent
//   direction.
#include "tipk_chol.h"
#include "tipk_fit_terms.h"

namespace {

constexpr int SF_NT = 256;                  // threads of a dense workgroup
constexpr int SF_NW = SF_NT / TIPK_WAVE;    // 4 wavefronts: 16 rows of the tile each
constexpr int SF_TILE = 64;
constexpr int SF_RB = 4;                    // relations per workgroup: the register block
constexpr int SF_PAD = 4;                   // floats behind a row of the LDS images
constexpr int SF_CW = 2 * SF_RB + 4;        // floats of a lane's coefficient row: 8 used; 12 words apart, the 16-byte stores of
                                            // 8 consecutive lanes fall on 32 different banks
constexpr int SF_CH = 256;                  // recorded pairs per chunk of the sparse pass
constexpr int SF_DMAX = CH_DMAX;
constexpr int64_t SF_NMAX = 46340;
constexpr int64_t SF_FITMAX = 65536;
constexpr int64_t SF_TARGET_WGS = 1024;     // dense workgroups to aim for: four per CU
constexpr int SF_EPT = (1 + SF_DMAX + SF_DMAX * SF_DMAX + SF_CH - 1) / SF_CH;   // outputs per thread of the finish

struct FitStatsArgs {
    const float *z, *w, *dense_w;
    const int64_t* pair_ptr;
    const int32_t *pair_u, *pair_v;
    const float *pair_wpos, *pair_wneg;
    const int32_t* active;
    float l2;
    int n, dim, T, slabs;
    int64_t n_fit, n_tiles, tps;
    float* part;
    float *loss, *grad, *hess;
};

template <int DP>
__global__ void __launch_bounds__(SF_NT) fit_dense_kernel(FitStatsArgs a) {
    constexpr int NH = DP / 16;
    constexpr int LD = DP + SF_PAD;
    __shared__ __attribute__((aligned(16))) float Zu[SF_TILE * LD];
    __shared__ __attribute__((aligned(16))) float Zv[SF_TILE * LD];
    __shared__ __attribute__((aligned(16))) float Ws[SF_RB * DP];
    __shared__ __attribute__((aligned(16))) float coef[SF_NW][TIPK_WAVE][SF_CW];

    const int t = threadIdx.x, lane = tipk_lane(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, dim = a.dim;
    const int64_t rb = blockIdx.y, slab = blockIdx.x, j0 = rb * SF_RB;

    bool any = false;
    float dw[SF_RB];
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        const int64_t j = j0 + x;
        const bool in = j < a.n_fit;
        dw[x] = in ? a.dense_w[j] : 0.f;
        any = any || (in && (!a.active || a.active[j] != 0));
    }
    if (!any) return;                                           // uniform in the workgroup

    for (int i = t; i < SF_RB * DP; i += SF_NT) {
        const int x = i / DP, c = i - x * DP;
        const int64_t j = j0 + x;
        Ws[i] = (j < a.n_fit && c < dim) ? a.w[j * dim + c] : 0.f;
    }

    sf_f4 H[SF_RB][NH][NH], G[NH];
    float lacc[SF_RB];
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        lacc[x] = 0.f;
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int hj = 0; hj < NH; ++hj) H[x][hi][hj] = sf_f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) G[h] = sf_f4{0.f, 0.f, 0.f, 0.f};

    const int64_t t0 = slab * a.tps, t1 = t0 + a.tps < a.n_tiles ? t0 + a.tps : a.n_tiles;
    int ub = 0, vb;
    {
        int64_t rest = t0;
        while (rest >= a.T - ub) { rest -= a.T - ub; ++ub; }    // (trip count: tile rows)
        vb = ub + (int)rest;
    }
    const int cc = lane & 15, kk = lane >> 4;

    for (int64_t tt = t0; tt < t1; ++tt) {
        __syncthreads();                                        // the previous tile has been read; Ws is staged
        for (int i = t; i < SF_TILE * (DP / 4); i += SF_NT) {
            const int r = i / (DP / 4), q = i - r * (DP / 4);
            const int64_t ru = (int64_t)ub * SF_TILE + r, rv = (int64_t)vb * SF_TILE + r;
            float4 xu = make_float4(0.f, 0.f, 0.f, 0.f), xv = xu;
            if (4 * q < dim) {
                if (ru < n) xu = tipk_ld4(a.z + ru * dim + 4 * q);
                if (rv < n) xv = tipk_ld4(a.z + rv * dim + 4 * q);
            }
            tipk_st4(&Zu[r * LD + 4 * q], xu);
            tipk_st4(&Zv[r * LD + 4 * q], xv);
        }
        __syncthreads();

        float zva[DP];                                          // phase A: the lane's own row v
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
            const float4 x4 = tipk_ld4(&Zv[lane * LD + 4 * q]);
            zva[4 * q] = x4.x; zva[4 * q + 1] = x4.y; zva[4 * q + 2] = x4.z; zva[4 * q + 3] = x4.w;
        }
        float zvb[16][NH];                                      // phase B: component c of the four rows of every step
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int h = 0; h < NH; ++h) zvb[s][h] = Zv[(4 * s + kk) * LD + 16 * h + cc];

        const int64_t v = (int64_t)vb * SF_TILE + lane;
        for (int ur = 0; ur < 16; ++ur) {
            const int uu = wave * 16 + ur;
            const int64_t u = (int64_t)ub * SF_TILE + uu;
            if (u >= n) break;                                  // uniform in the wavefront
            const float mult = (v < n && u <= v) ? (u == v ? 1.f : 2.f) : 0.f;

            // A. logits and coefficients, lane = v
            float f[DP];
#pragma unroll
            for (int q = 0; q < DP / 4; ++q) {
                const float4 x4 = tipk_ld4(&Zu[uu * LD + 4 * q]);
                f[4 * q] = x4.x * zva[4 * q]; f[4 * q + 1] = x4.y * zva[4 * q + 1];
                f[4 * q + 2] = x4.z * zva[4 * q + 2]; f[4 * q + 3] = x4.w * zva[4 * q + 3];
            }
            float ca[SF_RB], ch[SF_RB];
#pragma unroll
            for (int x = 0; x < SF_RB; ++x) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < DP / 4; ++q) {
                    const float4 w4 = tipk_ld4(&Ws[x * DP + 4 * q]);
                    s = fmaf(f[4 * q], w4.x, s); s = fmaf(f[4 * q + 1], w4.y, s);
                    s = fmaf(f[4 * q + 2], w4.z, s); s = fmaf(f[4 * q + 3], w4.w, s);
                }
                float sp, sig, h;
                sf_terms(s, sp, sig, h);
                const float cm = mult * dw[x];
                const bool valid = mult > 0.f;
                if (valid) lacc[x] += cm * sp;
                ca[x] = valid ? cm * sig : 0.f;
                ch[x] = valid ? cm * h : 0.f;
            }
            tipk_st4(&coef[wave][lane][0], make_float4(ca[0], ca[1], ca[2], ca[3]));
            tipk_st4(&coef[wave][lane][4], make_float4(ch[0], ch[1], ch[2], ch[3]));
            sf_wave_sync();

            // B. four pairs per MFMA, lane = (component, pair slot)
            float zu[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) zu[h] = Zu[uu * LD + 16 * h + cc];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float4 a4 = tipk_ld4(&coef[wave][4 * s + kk][0]);
                const float4 h4 = tipk_ld4(&coef[wave][4 * s + kk][4]);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
                float fb[NH];
#pragma unroll
                for (int h = 0; h < NH; ++h) fb[h] = zu[h] * zvb[s][h];
                const float ga = cc == 0 ? av[0] : cc == 1 ? av[1] : cc == 2 ? av[2] : cc == 3 ? av[3] : 0.f;
#pragma unroll
                for (int h = 0; h < NH; ++h) G[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, fb[h], G[h], 0, 0, 0);
#pragma unroll
                for (int x = 0; x < SF_RB; ++x)
#pragma unroll
                    for (int hi = 0; hi < NH; ++hi) {
                        const float ha = hv[x] * fb[hi];
#pragma unroll
                        for (int hj = 0; hj < NH; ++hj)
                            H[x][hi][hj] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha, fb[hj], H[x][hi][hj], 0, 0, 0);
                    }
            }
            sf_wave_sync();                                     // the coefficient rows are free for the next row
        }
        if (++vb == a.T) { ++ub; vb = ub; }
    }

    // the wavefront's partials: part[rb][slab][wave][x][1 + dim + dim^2]
    const int64_t E = sf_elems(dim);
    float* base = a.part + (((rb * a.slabs + slab) * SF_NW + wave) * SF_RB) * E;
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
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

__global__ void __launch_bounds__(SF_CH) fit_finish_kernel(FitStatsArgs a) {
    __shared__ float fs[SF_CH][SF_DMAX + 1];
    __shared__ float cs[SF_CH][3];
    const int t = threadIdx.x, dim = a.dim;
    const int64_t j = blockIdx.x;
    if (a.active && a.active[j] == 0) return;                   // uniform
    const int64_t E = sf_elems(dim);
    const int64_t rb = j / SF_RB, x = j - rb * SF_RB;

    float tot[SF_EPT];                                          // output e = t + 256 i: the dense slabs in ascending order
#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) {
        const int64_t e = t + (int64_t)SF_CH * i;
        float s = 0.f;
        if (e < E) {
            const float* p = a.part + ((rb * a.slabs * SF_NW) * SF_RB + x) * E + e;
            for (int64_t q = 0; q < (int64_t)a.slabs * SF_NW; ++q) s += p[q * SF_RB * E];
        }
        tot[i] = s;
    }

    float sparse[SF_EPT];
#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) sparse[i] = 0.f;
    const int64_t p0 = a.pair_ptr[j], p1 = a.pair_ptr[j + 1];
    const float* wr = a.w + j * dim;
    for (int64_t c0 = p0; c0 < p1; c0 += SF_CH) {
        const int cnt = p1 - c0 < SF_CH ? (int)(p1 - c0) : SF_CH;
        __syncthreads();                                        // the previous chunk has been read
        if (t < cnt) {
            int u = a.pair_u[c0 + t], v = a.pair_v[c0 + t];
            u = u < 0 ? 0 : (u >= a.n ? a.n - 1 : u);           // (ids in range are the caller's contract; nothing is
            v = v < 0 ? 0 : (v >= a.n ? a.n - 1 : v);           //  read out of bounds)
            const float* zu = a.z + (int64_t)u * dim;
            const float* zv = a.z + (int64_t)v * dim;
            float s = 0.f;
            for (int k = 0; k < dim; ++k) {
                const float f = zu[k] * zv[k];
                fs[t][k] = f;
                s = fmaf(f, wr[k], s);
            }
            float sp, spn, sig, sigm, h, hm;
            sf_terms(s, sp, sig, h);
            sf_terms(-s, spn, sigm, hm);                        // hm == h
            const float wp = a.pair_wpos[c0 + t], wn = a.pair_wneg[c0 + t];
            cs[t][0] = wp * spn - wn * sp;
            cs[t][1] = -wp * sigm - wn * sig;
            cs[t][2] = (wp - wn) * h;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SF_EPT; ++i) {
            const int64_t e = t + (int64_t)SF_CH * i;
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

#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) {
        const int64_t e = t + (int64_t)SF_CH * i;
        if (e >= E) continue;
        const float val = tot[i] + sparse[i];
        if (e == 0) {
            float ww = 0.f;
            for (int k = 0; k < dim; ++k) ww = fmaf(wr[k], wr[k], ww);
            a.loss[j] = val + 0.5f * a.l2 * ww;
        } else if (e <= dim) {
            a.grad[j * dim + e - 1] = val + a.l2 * wr[e - 1];
        } else {
            const int64_t q = e - 1 - dim;
            a.hess[j * dim * dim + q] = (q / dim == q % dim) ? val + a.l2 : val;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- step
struct StepArgs {
    const float *s_loss, *s_grad, *s_hess;
    float *w, *loss, *grad, *p, *t, *w_trial;
    int32_t *info, *active;
    int64_t n_fit;
    int dim;
    float gtol;
};

__device__ __forceinline__ float sf_wave_sum(float v) {
#pragma unroll
    for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float sf_wave_max(float v) {
#pragma unroll
    for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__global__ void __launch_bounds__(TIPK_WAVE) newton_step_kernel(StepArgs a) {
    __shared__ float L[SF_DMAX][SF_DMAX + 1];
    const int lane = threadIdx.x, dim = a.dim;
    const int64_t j = blockIdx.x;
    int32_t* info = a.info + 4 * j;
    const int status = info[0], evals = info[1];
    if (status != 0) {                                          // finished earlier: nothing further
        if (lane == 0) a.active[j] = 0;
        return;
    }
    const bool first = evals == 0, own = lane < dim;
    const float lt = a.s_loss[j];
    const float gt = own ? a.s_grad[j * dim + lane] : 0.f;
    bool fin = lt - lt == 0.f && gt - gt == 0.f;
    for (int c = 0; c < dim; ++c) {
        const float hv = own ? a.s_hess[(j * dim + lane) * dim + c] : 0.f;
        L[own ? lane : 0][own ? c : SF_DMAX] = hv;              // (lanes behind dim write the spare column of row 0)
        fin = fin && hv - hv == 0.f;
    }
    const bool finite = __all(fin) != 0;
    __syncthreads();

    float w = own ? a.w[j * dim + lane] : 0.f, g = own ? a.grad[j * dim + lane] : 0.f, p = own ? a.p[j * dim + lane] : 0.f;
    float loss = a.loss[j], step = a.t[j];
    const float wt = own ? a.w_trial[j * dim + lane] : 0.f;
    int acc = info[2], rej = info[3], st = 0;

    bool accept = first;
    if (!first && finite) {
        const float gp = sf_wave_sum(g * p);
        accept = lt <= loss + 1e-4f * step * gp + 9.5367431640625e-07f * fabsf(loss);     // 16 * 2^-24
    }
    if (!finite && !first) {
        st = 3;                                                 // the accepted row is kept
        ++rej;
    } else if (accept) {
        w = wt; g = gt; loss = lt; step = 1.0f;
        if (!first) ++acc;
        if (!finite) {
            st = 3;
            p = 0.f;
        } else {
            // Cholesky of the trial Hessian; L[i][k], i >= k
            float hmax = sf_wave_max(own ? L[lane][lane] : -INFINITY);
            const bool ok = ch_factor(L, dim, lane);
            if (ok) {
                float b = -g;                                   // L y = -g, then L^T p = y
                for (int k = 0; k < dim; ++k) {
                    const float yk = __shfl(b / L[k][k], k);
                    if (lane == k) b = yk;
                    else if (own && lane > k) b = fmaf(-L[lane][k], yk, b);
                }
                for (int k = dim - 1; k >= 0; --k) {
                    const float pk = __shfl(b / L[k][k], k);
                    if (lane == k) b = pk;
                    else if (lane < k) b = fmaf(-L[k][lane], pk, b);
                }
                p = own ? b : 0.f;
            } else {
                p = hmax > 0.f ? -g / hmax : -g;
            }
        }
    } else {
        ++rej;
        step *= 0.5f;
    }
    if (st == 0) {
        const float gmax = sf_wave_max(own ? fabsf(g) : 0.f);
        if (gmax <= a.gtol) st = 1;
        else if (step < 9.5367431640625e-07f) st = 2;           // 2^-20
    }
    if (own) {
        a.w[j * dim + lane] = w;
        a.grad[j * dim + lane] = g;
        a.p[j * dim + lane] = p;
        if (st == 0) a.w_trial[j * dim + lane] = fmaf(step, p, w);
    }
    if (lane == 0) {
        a.loss[j] = loss;
        a.t[j] = step;
        info[0] = st; info[1] = evals + 1; info[2] = acc; info[3] = rej;
        a.active[j] = st == 0;
    }
}

struct FitInitArgs {
    const float* init;
    float *w, *w_trial, *loss, *grad, *p, *t;
    int32_t *info, *active;
    int64_t n_fit;
    int dim;
};

__global__ void __launch_bounds__(256) fit_init_kernel(FitInitArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_fit * a.dim) {
        const float v = a.init ? a.init[i] : 0.f;
        a.w[i] = v; a.w_trial[i] = v; a.grad[i] = 0.f; a.p[i] = 0.f;
    }
    if (i < a.n_fit) {
        a.loss[i] = 0.f; a.t[i] = 1.0f; a.active[i] = 1;
        a.info[4 * i] = 0; a.info[4 * i + 1] = 0; a.info[4 * i + 2] = 0; a.info[4 * i + 3] = 0;
    }
}

struct FitShape {
    int T, slabs;
    int64_t n_tiles, tps, n_rb;
};

FitShape sf_shape(int64_t n_nodes, int64_t n_fit) {
    FitShape s;
    s.T = (int)tipk_ceil_div(n_nodes, SF_TILE);
    s.n_tiles = (int64_t)s.T * (s.T + 1) / 2;
    s.n_rb = tipk_ceil_div(n_fit < 1 ? 1 : n_fit, SF_RB);
    int64_t want = tipk_ceil_div(SF_TARGET_WGS, s.n_rb);
    if (want > s.n_tiles) want = s.n_tiles;
    if (want > 65535) want = 65535;
    s.tps = tipk_ceil_div(s.n_tiles, want);
    s.slabs = (int)tipk_ceil_div(s.n_tiles, s.tps);
    return s;
}

// workspace: [dense partials] then the state of tipk_distmult_fit
struct FitLayout {
    int64_t part, p, t, w_trial, active, s_loss, s_grad, s_hess, total;
};

FitLayout sf_layout(int64_t n_nodes, int dim, int64_t n_fit) {
    const FitShape s = sf_shape(n_nodes, n_fit);
    FitLayout l;
    int64_t o = 0;
    l.part = o; o += sf_a256(s.n_rb * s.slabs * SF_NW * SF_RB * sf_elems(dim) * 4);
    l.p = o; o += sf_a256(n_fit * dim * 4);
    l.t = o; o += sf_a256(n_fit * 4);
    l.w_trial = o; o += sf_a256(n_fit * dim * 4);
    l.active = o; o += sf_a256(n_fit * 4);
    l.s_loss = o; o += sf_a256(n_fit * 4);
    l.s_grad = o; o += sf_a256(n_fit * dim * 4);
    l.s_hess = o; o += sf_a256(n_fit * dim * dim * 4);
    l.total = o;
    return l;
}

int sf_stats_check(const float* z, int64_t n_nodes, int dim, const float* w, int64_t n_fit, const float* dense_w,
                   const int64_t* pair_ptr, const int32_t* pair_u, const int32_t* pair_v, const float* pair_wpos,
                   const float* pair_wneg, int64_t n_pairs, float l2, const float* loss, const float* grad, const float* hess,
                   const void* workspace) {
    if (n_nodes < 1 || dim < 1 || n_fit < 0 || n_pairs < 0 || !(l2 >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!z || !w || !dense_w || !pair_ptr || !loss || !grad || !hess || !workspace)) return TIPK_EINVAL;
    if (n_fit > 0 && n_pairs > 0 && (!pair_u || !pair_v || !pair_wpos || !pair_wneg)) return TIPK_EINVAL;
    if (!tipk_distmult_fit_supported(n_nodes, dim, n_fit > 0 ? n_fit : 1)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0) return TIPK_EUNSUPPORTED;
    return TIPK_OK;
}

int sf_stats_launch(FitStatsArgs& a, int64_t n_nodes, hipStream_t st) {
    const FitShape s = sf_shape(n_nodes, a.n_fit);
    a.T = s.T; a.slabs = s.slabs; a.n_tiles = s.n_tiles; a.tps = s.tps;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.n_rb);
    if (a.dim <= 16) hipLaunchKernelGGL(fit_dense_kernel<16>, grid, dim3(SF_NT), 0, st, a);
    else hipLaunchKernelGGL(fit_dense_kernel<32>, grid, dim3(SF_NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(fit_finish_kernel, dim3((unsigned)a.n_fit), dim3(SF_CH), 0, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_distmult_fit_supported(int64_t n_nodes, int dim, int64_t n_fit) {
    return n_nodes >= 1 && n_nodes <= SF_NMAX && dim >= 4 && dim <= SF_DMAX && dim % 4 == 0 && n_fit >= 1 && n_fit <= SF_FITMAX;
}

extern "C" int64_t tipk_distmult_fit_slabs(int64_t n_nodes, int dim, int64_t n_fit) {
    if (!tipk_distmult_fit_supported(n_nodes, dim, n_fit)) return -1;
    return sf_shape(n_nodes, n_fit).slabs;
}

extern "C" int64_t tipk_distmult_fit_max_chain(int64_t n_nodes, int dim, int64_t n_fit) {
    if (!tipk_distmult_fit_supported(n_nodes, dim, n_fit)) return -1;
    const FitShape s = sf_shape(n_nodes, n_fit);
    // dense: 16 rows x 64 pairs per tile and wavefront in one accumulator chain over the slab, then the 4 * slabs partials;
    // sparse: 256 pairs in a chunk, then the chunks of at most n (n + 1) / 2 distinct pairs; + the sparse total, + l2
    const int64_t dense = s.tps * 16 * SF_TILE + 6 + (int64_t)s.slabs * SF_NW;
    const int64_t sparse = SF_CH + tipk_ceil_div(n_nodes * (n_nodes + 1) / 2, SF_CH);
    return (dense > sparse ? dense : sparse) + 2;
}

extern "C" int64_t tipk_distmult_fit_workspace_bytes(int64_t n_nodes, int dim, int64_t n_fit) {
    if (n_fit == 0 && tipk_distmult_fit_supported(n_nodes, dim, 1)) return 0;
    if (!tipk_distmult_fit_supported(n_nodes, dim, n_fit)) return -1;
    return sf_layout(n_nodes, dim, n_fit).total;
}

extern "C" int tipk_distmult_fit_stats(const float* z, int64_t n_nodes, int dim, const float* w, int64_t n_fit,
                                       const float* dense_w, const int64_t* pair_ptr, const int32_t* pair_u,
                                       const int32_t* pair_v, const float* pair_wpos, const float* pair_wneg, int64_t n_pairs,
                                       float l2, const int32_t* active, float* loss, float* grad, float* hess, void* workspace,
                                       tipk_stream_t stream) {
    const int bad = sf_stats_check(z, n_nodes, dim, w, n_fit, dense_w, pair_ptr, pair_u, pair_v, pair_wpos, pair_wneg, n_pairs,
                                   l2, loss, grad, hess, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_fit == 0) return TIPK_OK;
    FitStatsArgs a;
    a.z = z; a.w = w; a.dense_w = dense_w; a.pair_ptr = pair_ptr; a.pair_u = pair_u; a.pair_v = pair_v;
    a.pair_wpos = pair_wpos; a.pair_wneg = pair_wneg; a.active = active; a.l2 = l2; a.n = (int)n_nodes; a.dim = dim;
    a.n_fit = n_fit; a.part = reinterpret_cast<float*>(workspace); a.loss = loss; a.grad = grad; a.hess = hess;
    return sf_stats_launch(a, n_nodes, (hipStream_t)stream);
}

extern "C" int tipk_newton_step(int dim, int64_t n_fit, const float* stat_loss, const float* stat_grad, const float* stat_hess,
                                float gtol, float* w, float* loss, float* grad, float* p, float* t, int32_t* info,
                                float* w_trial, int32_t* active, tipk_stream_t stream) {
    if (dim < 1 || n_fit < 0 || !(gtol >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!stat_loss || !stat_grad || !stat_hess || !w || !loss || !grad || !p || !t || !info || !w_trial || !active))
        return TIPK_EINVAL;
    if (dim > SF_DMAX || n_fit > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if (n_fit == 0) return TIPK_OK;
    StepArgs a;
    a.s_loss = stat_loss; a.s_grad = stat_grad; a.s_hess = stat_hess; a.w = w; a.loss = loss; a.grad = grad; a.p = p; a.t = t;
    a.w_trial = w_trial; a.info = info; a.active = active; a.n_fit = n_fit; a.dim = dim; a.gtol = gtol;
    hipLaunchKernelGGL(newton_step_kernel, dim3((unsigned)n_fit), dim3(TIPK_WAVE), 0, (hipStream_t)stream, a);
    TIPK_RETURN_LAUNCH();
}

extern "C" int tipk_distmult_fit(const float* z, int64_t n_nodes, int dim, int64_t n_fit, const float* dense_w,
                                 const int64_t* pair_ptr, const int32_t* pair_u, const int32_t* pair_v, const float* pair_wpos,
                                 const float* pair_wneg, int64_t n_pairs, float l2, const float* init, int max_iter, float gtol,
                                 float* out_w, float* out_loss, float* out_grad, int32_t* out_info, void* workspace,
                                 tipk_stream_t stream) {
    if (max_iter < 0 || !(gtol >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!out_w || !out_info)) return TIPK_EINVAL;
    const int bad = sf_stats_check(z, n_nodes, dim, out_w, n_fit, dense_w, pair_ptr, pair_u, pair_v, pair_wpos, pair_wneg,
                                   n_pairs, l2, out_loss, out_grad, out_loss, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_fit == 0) return TIPK_OK;
    const FitLayout l = sf_layout(n_nodes, dim, n_fit);
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;

    FitInitArgs ia;
    ia.init = init; ia.w = out_w; ia.w_trial = reinterpret_cast<float*>(ws + l.w_trial); ia.loss = out_loss; ia.grad = out_grad;
    ia.p = reinterpret_cast<float*>(ws + l.p); ia.t = reinterpret_cast<float*>(ws + l.t); ia.info = out_info;
    ia.active = reinterpret_cast<int32_t*>(ws + l.active); ia.n_fit = n_fit; ia.dim = dim;
    hipLaunchKernelGGL(fit_init_kernel, dim3((unsigned)tipk_ceil_div(n_fit * dim, 256)), dim3(256), 0, st, ia);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);

    FitStatsArgs a;
    a.z = z; a.w = ia.w_trial; a.dense_w = dense_w; a.pair_ptr = pair_ptr; a.pair_u = pair_u; a.pair_v = pair_v;
    a.pair_wpos = pair_wpos; a.pair_wneg = pair_wneg; a.active = ia.active; a.l2 = l2; a.n = (int)n_nodes; a.dim = dim;
    a.n_fit = n_fit; a.part = reinterpret_cast<float*>(ws + l.part);
    a.loss = reinterpret_cast<float*>(ws + l.s_loss); a.grad = reinterpret_cast<float*>(ws + l.s_grad);
    a.hess = reinterpret_cast<float*>(ws + l.s_hess);
    StepArgs s;
    s.s_loss = a.loss; s.s_grad = a.grad; s.s_hess = a.hess; s.w = out_w; s.loss = out_loss; s.grad = out_grad; s.p = ia.p;
    s.t = ia.t; s.w_trial = ia.w_trial; s.info = out_info; s.active = ia.active; s.n_fit = n_fit; s.dim = dim; s.gtol = gtol;
    for (int it = 0; it <= max_iter; ++it) {
        const int status = sf_stats_launch(a, n_nodes, st);
        if (status != TIPK_OK) return status;
        hipLaunchKernelGGL(newton_step_kernel, dim3((unsigned)n_fit), dim3(TIPK_WAVE), 0, st, s);
        e = hipGetLastError();
        if (e != hipSuccess) return tipk_hip_status(e);
    }
    return TIPK_OK;
}
