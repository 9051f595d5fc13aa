// What the Newton fits on the frozen model share (include/tipk.h sections 4m, 4q, 4r).  sf_terms -- the terms of a logit --
// serves all three (tipk_side_effect_fit.hip, tipk_drug_fit.hip, tipk_calibrate.hip).  Everything below it is the STATISTICS
// BODY of the two embedding-width fits, which differ only in what a tile is and how it is walked: the sizes, the fields both
// argument structs carry, the slab split, and the device code of a workgroup of the dense launch (activity test, trial rows,
// accumulators, ONE ROW of a tile -- phases A and B --, the partial record) and of the finish launch (the whole body; a fit
// only says which two rows make a listed term's feature).  The arithmetic exists once, so both fits keep their bits together.
#pragma once
#include "tipk_chol.h"
#include <math.h>

typedef float sf_f4 __attribute__((ext_vector_type(4)));

constexpr int SF_NT = 256;                  // threads of a dense workgroup
constexpr int SF_NW = SF_NT / TIPK_WAVE;    // 4 wavefronts: 16 rows of the tile each
constexpr int SF_TILE = 64;
constexpr int SF_RB = 4;                    // unknown rows per workgroup: the register block
constexpr int SF_PAD = 4;                   // floats behind a row of the LDS images
constexpr int SF_CW = 2 * SF_RB + 4;        // floats of a lane's coefficient row: 8 used; 12 words apart, the 16-byte stores of
                                            // 8 consecutive lanes fall on 32 different banks
constexpr int SF_CH = 256;                  // listed terms per chunk of the sparse pass; threads of the finish
constexpr int SF_LB = 16;                   // partials a thread of the finish loads before it adds them
constexpr int SF_DMAX = CH_DMAX;
constexpr int64_t SF_FITMAX = 65536;
constexpr int64_t SF_TARGET_WGS = 1024;     // dense workgroups to aim for: four per CU
constexpr int SF_EPT = (1 + SF_DMAX + SF_DMAX * SF_DMAX + SF_CH - 1) / SF_CH;   // outputs per thread of the finish

__host__ __device__ inline int64_t sf_elems(int dim) { return 1 + dim + (int64_t)dim * dim; }      // loss, gradient, Hessian

// the fields the statistics kernels of both fits read the same way; a fit's own struct adds its frozen tables and its tiling
struct SfStatsArgs {
    const float *x, *dense_w, *prior;       // trial rows [n_fit, dim]; weight of the dense stream; centre of the l2 terms or NULL (0)
    const int64_t* ptr;                     // lists: row j owns the terms ptr[j] .. ptr[j + 1]
    const float *wpos, *wneg;
    const int32_t* active;
    float l2;
    int dim, slabs;
    int64_t n_fit, n_tiles, tps;
    float* part;                            // [row block][slab][wavefront][row][1 + dim + dim^2]
    float *loss, *grad, *hess;
};

// n_tiles tiles in `slabs` contiguous ranges of tps, for n_blocks blocks of SF_RB rows: about SF_TARGET_WGS workgroups
struct SfSlabs {
    int slabs;
    int64_t n_tiles, tps, n_blocks;
};

inline SfSlabs sf_slabs(int64_t n_tiles, int64_t n_fit) {
    SfSlabs s;
    s.n_tiles = n_tiles;
    s.n_blocks = tipk_ceil_div(n_fit < 1 ? 1 : n_fit, SF_RB);
    int64_t want = tipk_ceil_div(SF_TARGET_WGS, s.n_blocks);
    if (want > n_tiles) want = n_tiles;
    if (want > 65535) want = 65535;
    s.tps = tipk_ceil_div(n_tiles, want);
    s.slabs = (int)tipk_ceil_div(n_tiles, s.tps);
    return s;
}

// longest chain of fp32 additions behind an output.  dense: 16 rows x 64 terms per tile and wavefront in one accumulator
// chain over the slab, then the 4 * slabs partials; sparse: 256 terms in a chunk, then the chunks of at most `cells` distinct
// terms; + the sparse total, + l2
inline int64_t sf_max_chain(const SfSlabs& s, int64_t cells) {
    const int64_t dense = s.tps * 16 * SF_TILE + 6 + (int64_t)s.slabs * SF_NW;
    const int64_t sparse = SF_CH + tipk_ceil_div(cells, SF_CH);
    return (dense > sparse ? dense : sparse) + 2;
}

#ifdef __HIPCC__
__device__ __forceinline__ void sf_wave_sync() {               // LDS written by this wavefront is visible to it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// softplus(s), sigma(s) and sigma'(s) from one exponential; all NaN for a NaN logit.  The terms of a listed pair are the same
// function at -s: softplus(-s), sigma(-s)
__device__ __forceinline__ void sf_terms(float s, float& sp, float& sig, float& h) {
    const float e = expf(-fabsf(s));
    const float r = 1.0f / (1.0f + e);
    sp = fmaxf(s, 0.f) + log1pf(e);
    const float er = e * r;
    sig = s >= 0.f ? r : er;
    h = er * r;
    if (s != s) sig = s;
}

// ----------------------------------------------------------------------------------------------- dense launch, per workgroup
// what a wavefront accumulates over its slab, in registers
template <int DP>
struct SfAcc {
    sf_f4 H[SF_RB][DP / 16][DP / 16], G[DP / 16];
    float lacc[SF_RB];
};

template <int DP>
__device__ __forceinline__ void sf_zero(SfAcc<DP>& acc) {
    constexpr int NH = DP / 16;
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        acc.lacc[x] = 0.f;
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int hj = 0; hj < NH; ++hj) acc.H[x][hi][hj] = sf_f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) acc.G[h] = sf_f4{0.f, 0.f, 0.f, 0.f};
}

// dense_w of the rows of block `blk`; false: none of them is active (uniform in the workgroup)
__device__ __forceinline__ bool sf_block_active(const SfStatsArgs& a, int64_t blk, float (&dw)[SF_RB]) {
    bool any = false;
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        const int64_t j = blk * SF_RB + x;
        const bool in = j < a.n_fit;
        dw[x] = in ? a.dense_w[j] : 0.f;
        any = any || (in && (!a.active || a.active[j] != 0));
    }
    return any;
}

// the block's trial rows to LDS, zero-padded to DP (visible behind the caller's next __syncthreads())
template <int DP>
__device__ __forceinline__ void sf_stage_trial(const SfStatsArgs& a, int64_t blk, float* Xs) {
    for (int i = threadIdx.x; i < SF_RB * DP; i += SF_NT) {
        const int x = i / DP, c = i - x * DP;
        const int64_t j = blk * SF_RB + x;
        Xs[i] = (j < a.n_fit && c < a.dim) ? a.x[j * a.dim + c] : 0.f;
    }
}

// the lane-side image of a tile (64 rows of DP + SF_PAD floats) into the lane's registers.  Phase A: the lane's own row
template <int DP>
__device__ __forceinline__ void sf_lane_row(const float* img, float (&ra)[DP]) {
    const float* row = img + tipk_lane() * (DP + SF_PAD);
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
        const float4 x4 = tipk_ld4(row + 4 * q);
        ra[4 * q] = x4.x; ra[4 * q + 1] = x4.y; ra[4 * q + 2] = x4.z; ra[4 * q + 3] = x4.w;
    }
}

// phase B: component c = lane & 15 of the four rows (slot k = lane >> 4) of every step
template <int DP>
__device__ __forceinline__ void sf_lane_operands(const float* img, float (&rb)[16][DP / 16]) {
    const int cc = tipk_lane() & 15, kk = tipk_lane() >> 4;
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int h = 0; h < DP / 16; ++h) rb[s][h] = img[(4 * s + kk) * (DP + SF_PAD) + 16 * h + cc];
}

// ONE ROW of the tile against its 64 lane-side rows, by one wavefront.  `row`: the row in the row-side image; ra, rb: the
// lane-side registers above; Xs: the trial rows; scale: the multiplicity of the lane's term, 0 = the term does not exist;
// coef: the wavefront's coefficient rows.
//   A. lane = lane-side row.  f = row * ra rounded once per component, the logit of trial row x the fmaf chain over k ascending
//      from +0.0f, its terms from one expf (sf_terms).  The lane adds scale dense_w softplus to its loss and leaves
//      (scale dense_w sigma, scale dense_w sigma') per trial row in `coef`.  The feature is computed ONCE for the block.
//   B. lane = (component c, slot k): 16 steps of four terms on v_mfma_f32_16x16x4_f32 with the terms as K.  Gradient of all
//      trial rows in ONE product (row i of A is trial row i), the Hessian of trial row x as (sigma' f) f^T per 16 x 16 tile.
template <int DP>
__device__ __forceinline__ void sf_tile_row(const float* row, const float (&ra)[DP], const float (&rb)[16][DP / 16],
                                            const float* Xs, const float (&dw)[SF_RB], float scale, float (*coef)[SF_CW],
                                            SfAcc<DP>& acc) {
    constexpr int NH = DP / 16;
    const int lane = tipk_lane(), cc = lane & 15, kk = lane >> 4;

    float f[DP];
#pragma unroll
    for (int q = 0; q < DP / 4; ++q) {
        const float4 x4 = tipk_ld4(row + 4 * q);
        f[4 * q] = x4.x * ra[4 * q]; f[4 * q + 1] = x4.y * ra[4 * q + 1];
        f[4 * q + 2] = x4.z * ra[4 * q + 2]; f[4 * q + 3] = x4.w * ra[4 * q + 3];
    }
    float ca[SF_RB], ch[SF_RB];
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
            const float4 w4 = tipk_ld4(Xs + x * DP + 4 * q);
            s = fmaf(f[4 * q], w4.x, s); s = fmaf(f[4 * q + 1], w4.y, s);
            s = fmaf(f[4 * q + 2], w4.z, s); s = fmaf(f[4 * q + 3], w4.w, s);
        }
        float sp, sig, h;
        sf_terms(s, sp, sig, h);
        const float cm = scale * dw[x];
        const bool valid = scale > 0.f;
        if (valid) acc.lacc[x] += cm * sp;
        ca[x] = valid ? cm * sig : 0.f;
        ch[x] = valid ? cm * h : 0.f;
    }
    tipk_st4(&coef[lane][0], make_float4(ca[0], ca[1], ca[2], ca[3]));
    tipk_st4(&coef[lane][4], make_float4(ch[0], ch[1], ch[2], ch[3]));
    sf_wave_sync();

    float rc[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) rc[h] = row[16 * h + cc];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float4 a4 = tipk_ld4(&coef[4 * s + kk][0]);
        const float4 h4 = tipk_ld4(&coef[4 * s + kk][4]);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
        float fb[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) fb[h] = rc[h] * rb[s][h];
        const float ga = cc == 0 ? av[0] : cc == 1 ? av[1] : cc == 2 ? av[2] : cc == 3 ? av[3] : 0.f;
#pragma unroll
        for (int h = 0; h < NH; ++h) acc.G[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, fb[h], acc.G[h], 0, 0, 0);
#pragma unroll
        for (int x = 0; x < SF_RB; ++x)
#pragma unroll
            for (int hi = 0; hi < NH; ++hi) {
                const float ha = hv[x] * fb[hi];
#pragma unroll
                for (int hj = 0; hj < NH; ++hj)
                    acc.H[x][hi][hj] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha, fb[hj], acc.H[x][hi][hj], 0, 0, 0);
            }
    }
    sf_wave_sync();                                             // the coefficient rows are free for the next row
}

// the wavefront's partials: part[blk][slab][wave][x][1 + dim + dim^2]
template <int DP>
__device__ __forceinline__ void sf_write_partial(const SfStatsArgs& a, int64_t blk, int64_t slab, int wave,
                                                 const SfAcc<DP>& acc) {
    constexpr int NH = DP / 16;
    const int lane = tipk_lane(), cc = lane & 15, kk = lane >> 4, dim = a.dim;
    const int64_t E = sf_elems(dim);
    float* base = a.part + (((blk * a.slabs + slab) * SF_NW + wave) * SF_RB) * E;
#pragma unroll
    for (int x = 0; x < SF_RB; ++x) {
        float p = acc.lacc[x];
#pragma unroll
        for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) p += __shfl_down(p, off);
        float* o = base + x * E;
        if (lane == 0) o[0] = p;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (kk == 0 && 16 * h + cc < dim) o[1 + 16 * h + cc] = acc.G[h][x];      // row x of the gradient product
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int hj = 0; hj < NH; ++hj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * hi + 4 * kk + r, col = 16 * hj + cc;
                    if (row < dim && col < dim) o[1 + dim + row * dim + col] = acc.H[x][hi][hj][r];
                }
    }
}

// ---------------------------------------------------------------------------------------------- finish launch, the whole body
// One workgroup of SF_CH threads per row j = blockIdx.x: sums the 4 * slabs partials of every output in ascending (slab,
// wavefront) order (SF_LB loads in flight, then added in that order: one round trip to L2 per batch, not per partial), adds
// the sparse correction over the row's listed terms (chunks of 256: a chain from +0.0f inside the chunk in list order, the
// chunks added in ascending order) and the l2 terms around the prior centre, and writes the outputs.  An inactive row returns
// at once.  feature(p, ra, rb): the two rows of the frozen tables whose product is the feature of list position p.
template <class Feature>
__device__ __forceinline__ void sf_finish(const SfStatsArgs& a, float (*fs)[SF_DMAX + 1], float (*cs)[3], Feature feature) {
    const int t = threadIdx.x, dim = a.dim;
    const int64_t j = blockIdx.x;
    if (a.active && a.active[j] == 0) return;                   // uniform
    const int64_t E = sf_elems(dim);
    const int64_t blk = j / SF_RB, x = j - blk * SF_RB;

    float tot[SF_EPT];                                          // output e = t + 256 i: the dense slabs in ascending order
#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) {
        const int64_t e = t + (int64_t)SF_CH * i;
        float s = 0.f;
        if (e < E) {
            const float* p = a.part + ((blk * a.slabs * SF_NW) * SF_RB + x) * E + e;
            const int64_t np = (int64_t)a.slabs * SF_NW, step = SF_RB * E;
            int64_t q = 0;
            for (; q + SF_LB <= np; q += SF_LB) {
                float v[SF_LB];
#pragma unroll
                for (int u = 0; u < SF_LB; ++u) v[u] = p[(q + u) * step];
#pragma unroll
                for (int u = 0; u < SF_LB; ++u) s += v[u];
            }
            for (; q < np; ++q) s += p[q * step];
        }
        tot[i] = s;
    }

    float sparse[SF_EPT];
#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) sparse[i] = 0.f;
    const int64_t p0 = a.ptr[j], p1 = a.ptr[j + 1];
    const float* xr = a.x + j * dim;
    for (int64_t c0 = p0; c0 < p1; c0 += SF_CH) {
        const int cnt = p1 - c0 < SF_CH ? (int)(p1 - c0) : SF_CH;
        __syncthreads();                                        // the previous chunk has been read
        if (t < cnt) {
            const float *ra, *rb;
            feature(c0 + t, ra, rb);
            float s = 0.f;
            for (int k = 0; k < dim; ++k) {
                const float f = ra[k] * rb[k];
                fs[t][k] = f;
                s = fmaf(f, xr[k], s);
            }
            float sp, spn, sig, sigm, h, hm;
            sf_terms(s, sp, sig, h);
            sf_terms(-s, spn, sigm, hm);                        // hm == h
            const float wp = a.wpos[c0 + t], wn = a.wneg[c0 + t];
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

    const float* pr = a.prior ? a.prior + j * dim : nullptr;    // the l2 terms pull to the prior centre c (NULL: 0)
#pragma unroll
    for (int i = 0; i < SF_EPT; ++i) {
        const int64_t e = t + (int64_t)SF_CH * i;
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
#endif
