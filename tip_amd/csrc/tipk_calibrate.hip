// Per-relation Platt calibration of the DistMult logit (include/tipk.h section 4r): the statistics (loss, gradient, Hessian)
// of the calibration objective at trial maps t = a s + b, and an entry that enqueues max_iter + 1 (statistics,
// tipk_newton_step with dim = 2) pairs: the step, the state layout, the init launch and the loop are tipk_newton.h /
// tipk_newton.hip, shared with the two fits (4m, 4q).
//
// Statistics, launch 1, calib_dense_kernel: the sum over ALL cells u < v of a query's relation as a mask-free stream over
//   the 64 x 64 tiles of the upper triangle.  Workgroup (query, part) takes the part's tiles as WgDeal deals them and scores
//   a tile with wg_score_tile -- the staging and the fma loop of the screen (tipk_wg_topk.h), so s has the screen's bits.
//   Thread (ty, tx) owns 4 x 4 cells of the tile; per cell t = fmaf(a, s, b) and sf_terms(t) (one expf: softplus, sigma,
//   sigma'); the six terms of its 16 cells are added in fp32 in (i, j) order from +0.0f (a cell with u >= v or v >= n adds
//   +0.0f), the tile's six sums then go onto fp64 accumulators that run through the part.  At its end the 64 lanes of a
//   wavefront are summed by the halving tree, the 4 wavefronts in ascending order: part[query][part][6], fp64.
// Launch 2, calib_finish_kernel: one workgroup per query adds the parts in ascending order, then the sparse correction over
//   the query's listed cells (thread x takes the cells x, x + 256, ... in list order; threads, then wavefronts, are summed
//   as above), all in fp64; result = dense_w * dense + sparse + l2 term, rounded to fp32 ONCE.  A weight of exactly 0 makes
//   its term absent (0, whatever the term is): a query with M = 0 has the l2 term alone.
// A workgroup of an inactive query returns at once; its rows of the outputs are not touched.
// No atomics, no workgroup waits for another, every trip count depends on sizes and list lengths only: BITWISE repeatable.
#include "tipk_fit_terms.h"
#include "tipk_newton.h"
#include "tipk_wg_topk.h"

namespace {

constexpr int CAL_DMAX = 256;               // widest z: the screen's
constexpr int64_t CAL_NMAX = 46340;
constexpr int64_t CAL_QMAX = 65536;
constexpr int CAL_NS = 6;                   // loss, g_a, g_b, H_aa, H_ab, H_bb
constexpr int CAL_NW = WG_NT / TIPK_WAVE;
constexpr int CAL_CHAIN = 16 + 2;           // fp32: the 16 cells of a thread in a tile, the final rounding; + 1 for all of fp64

struct CalArgs {
    const float *z, *w, *ab, *dense_w;
    const int32_t* qrel;
    const int64_t* pair_ptr;
    const int32_t *pair_u, *pair_v;
    const float *pair_wpos, *pair_wneg;
    const int32_t* active;
    float l2;
    int n, dim, n_rel, splits;
    int64_t n_q;
    double* part;
    float *loss, *grad, *hess;
};

__device__ __forceinline__ int cal_clamp(int x, int hi) { return x < 0 ? 0 : (x >= hi ? hi - 1 : x); }

// the 256 threads' v[0..5] -> their sum in every slot of `out` read by thread 0 .. 5: halving tree over the lanes, the
// wavefronts in ascending order.  Contains TWO __syncthreads(): before the wavefront rows are written (red is free) and after.
__device__ __forceinline__ void cal_block_sum(double (&v)[CAL_NS], double (*red)[CAL_NS], double* out) {
    const int t = threadIdx.x, lane = tipk_lane(), wave = t >> 6;
#pragma unroll
    for (int e = 0; e < CAL_NS; ++e)
#pragma unroll
        for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) v[e] += __shfl_down(v[e], off);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int e = 0; e < CAL_NS; ++e) red[wave][e] = v[e];
    __syncthreads();
    if (t < CAL_NS) {
        double s = 0.0;
        for (int q = 0; q < CAL_NW; ++q) s += red[q][t];
        out[t] = s;
    }
}

__global__ void __launch_bounds__(WG_NT) calib_dense_kernel(CalArgs a) {
    __shared__ float As[WG_KC * WG_LD];
    __shared__ float Zs[WG_KC * WG_LD];
    __shared__ float wl[CAL_DMAX];
    __shared__ double red[CAL_NW][CAL_NS];

    const int t = threadIdx.x;
    const int64_t qi = blockIdx.x / a.splits;
    const int part = blockIdx.x % a.splits;
    if (a.active && a.active[qi] == 0) return;                  // uniform
    const int n = a.n, dim = a.dim;
    const int r = cal_clamp(a.qrel[qi], a.n_rel);
    const float ca = a.ab[2 * qi], cb = a.ab[2 * qi + 1];
    for (int i = t; i < dim; i += WG_NT) wl[i] = a.w[(int64_t)r * dim + i];   // (read behind wg_score_tile's first barrier)
    const int ty = t >> 4, tx = t & 15;

    double run[CAL_NS];
#pragma unroll
    for (int e = 0; e < CAL_NS; ++e) run[e] = 0.0;

    WgDeal deal(n, part, a.splits);
    for (int64_t tile = deal.t0; tile < deal.t1; ++tile) {
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        wg_score_tile(As, Zs, a.z, wl, n, dim, deal.bu, deal.bv, acc);
        const int u0 = deal.bu * WG_TILE + 4 * ty, v0 = deal.bv * WG_TILE + 4 * tx;
        float f[CAL_NS];
#pragma unroll
        for (int e = 0; e < CAL_NS; ++e) f[e] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = u0 + i < v0 + j && v0 + j < n;
                const float s = acc[i][j];
                float sp, sig, h;
                sf_terms(fmaf(ca, s, cb), sp, sig, h);
                const float hs = h * s;
                f[0] += in ? sp : 0.f;
                f[1] += in ? sig * s : 0.f;
                f[2] += in ? sig : 0.f;
                f[3] += in ? hs * s : 0.f;
                f[4] += in ? hs : 0.f;
                f[5] += in ? h : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < CAL_NS; ++e) run[e] += (double)f[e];
        deal.next();
    }

    cal_block_sum(run, red, a.part + (qi * a.splits + part) * CAL_NS);
}

__global__ void __launch_bounds__(WG_NT) calib_finish_kernel(CalArgs a) {
    __shared__ double red[CAL_NW][CAL_NS];
    __shared__ double sparse[CAL_NS];
    const int t = threadIdx.x, dim = a.dim;
    const int64_t qi = blockIdx.x;
    if (a.active && a.active[qi] == 0) return;                  // uniform
    const int r = cal_clamp(a.qrel[qi], a.n_rel);
    const float* wr = a.w + (int64_t)r * dim;
    const float ca = a.ab[2 * qi], cb = a.ab[2 * qi + 1];

    double v[CAL_NS];
#pragma unroll
    for (int e = 0; e < CAL_NS; ++e) v[e] = 0.0;
    const int64_t p0 = a.pair_ptr[qi], p1 = a.pair_ptr[qi + 1];
    for (int64_t p = p0 + t; p < p1; p += WG_NT) {
        int u = cal_clamp(a.pair_u[p], a.n), vv = cal_clamp(a.pair_v[p], a.n);  // (ids in range are the caller's contract;
        if (u > vv) { const int x = u; u = vv; vv = x; }                        //  nothing is read out of bounds)
        const float* zu = a.z + (int64_t)u * dim;
        const float* zv = a.z + (int64_t)vv * dim;
        float s = 0.f;
        for (int k = 0; k < dim; ++k) {
            const float x = zu[k] * wr[k];
            s = fmaf(x, zv[k], s);
        }
        const float tt = fmaf(ca, s, cb);
        float sp, sig, h, spn, sigm, hm;
        sf_terms(tt, sp, sig, h);
        sf_terms(-tt, spn, sigm, hm);                           // hm == h
        const double wp = a.pair_wpos[p], wn = a.pair_wneg[p], wh = wp + wn;
        const bool hp = wp != 0.0, hn = wn != 0.0, hh = wh != 0.0;      // a weight of exactly 0: the term is absent
        const float hs = h * s;
        v[0] += (hp ? wp * (double)spn : 0.0) + (hn ? wn * (double)sp : 0.0);
        v[1] += (hn ? wn * (double)(sig * s) : 0.0) - (hp ? wp * (double)(sigm * s) : 0.0);
        v[2] += (hn ? wn * (double)sig : 0.0) - (hp ? wp * (double)sigm : 0.0);
        v[3] += hh ? wh * (double)(hs * s) : 0.0;
        v[4] += hh ? wh * (double)hs : 0.0;
        v[5] += hh ? wh * (double)h : 0.0;
    }
    cal_block_sum(v, red, sparse);                              // sparse[e] is read by the thread that wrote it

    if (t < CAL_NS) {
        double d = 0.0;
        const double* p = a.part + qi * a.splits * CAL_NS + t;
        for (int q = 0; q < a.splits; ++q) d += p[(int64_t)q * CAL_NS];
        const double da = (double)ca - 1.0, l2 = a.l2;
        const double dw = a.dense_w[qi];
        double val = (dw != 0.0 ? dw * d : 0.0) + sparse[t];          // dense_w == 0: the stream is absent

        if (t == 0) val += 0.5 * l2 * da * da;
        if (t == 1) val += l2 * da;
        if (t == 3) val += l2;
        const float x = (float)val;
        if (t == 0) a.loss[qi] = x;
        else if (t <= 2) a.grad[2 * qi + t - 1] = x;
        else if (t == 3) a.hess[4 * qi] = x;
        else if (t == 4) { a.hess[4 * qi + 1] = x; a.hess[4 * qi + 2] = x; }
        else a.hess[4 * qi + 3] = x;
    }
}

// workspace: [dense partials, fp64] then the state of tipk_distmult_calibrate
NewtonLayout cal_layout(int64_t n_nodes, int64_t n_q) {
    return newton_layout(n_q * wg_splits(n_nodes, n_q) * CAL_NS * 8, n_q, 2);
}

int cal_stats_check(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel, const int32_t* q_rel,
                    const float* ab, int64_t n_q, const float* dense_w, const int64_t* pair_ptr, const int32_t* pair_u,
                    const int32_t* pair_v, const float* pair_wpos, const float* pair_wneg, int64_t n_pairs, float l2,
                    const float* loss, const float* grad, const float* hess, const void* workspace) {
    if (n_nodes < 1 || dim < 1 || n_rel < 1 || n_q < 0 || n_pairs < 0 || !(l2 >= 0.f)) return TIPK_EINVAL;
    if (n_q > 0 && (!z || !rel_w || !q_rel || !ab || !dense_w || !pair_ptr || !loss || !grad || !hess || !workspace))
        return TIPK_EINVAL;
    if (n_q > 0 && n_pairs > 0 && (!pair_u || !pair_v || !pair_wpos || !pair_wneg)) return TIPK_EINVAL;
    if (!tipk_distmult_calibrate_supported(n_nodes, dim, n_q > 0 ? n_q : 1) || n_rel > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(z) & 15) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return TIPK_EUNSUPPORTED;
    return TIPK_OK;
}

int cal_stats_launch(CalArgs& a, hipStream_t st) {
    a.splits = wg_splits(a.n, a.n_q);
    hipLaunchKernelGGL(calib_dense_kernel, dim3((unsigned)(a.n_q * a.splits)), dim3(WG_NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(calib_finish_kernel, dim3((unsigned)a.n_q), dim3(WG_NT), 0, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_distmult_calibrate_supported(int64_t n_nodes, int dim, int64_t n_q) {
    return n_nodes >= 1 && n_nodes <= CAL_NMAX && dim >= 4 && dim <= CAL_DMAX && dim % 4 == 0 && n_q >= 1 && n_q <= CAL_QMAX;
}

extern "C" int64_t tipk_distmult_calibrate_splits(int64_t n_nodes, int dim, int64_t n_q) {
    if (!tipk_distmult_calibrate_supported(n_nodes, dim, n_q)) return -1;
    return wg_splits(n_nodes, n_q);
}

extern "C" int64_t tipk_distmult_calibrate_max_chain(int64_t n_nodes, int dim, int64_t n_q) {
    if (!tipk_distmult_calibrate_supported(n_nodes, dim, n_q)) return -1;
    return CAL_CHAIN;
}

extern "C" int64_t tipk_distmult_calibrate_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q) {
    if (n_q == 0 && tipk_distmult_calibrate_supported(n_nodes, dim, 1)) return 0;
    if (!tipk_distmult_calibrate_supported(n_nodes, dim, n_q)) return -1;
    return cal_layout(n_nodes, n_q).total;
}

extern "C" int tipk_distmult_calibrate_stats(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                             const int32_t* q_rel, const float* ab, int64_t n_q, const float* dense_w,
                                             const int64_t* pair_ptr, const int32_t* pair_u, const int32_t* pair_v,
                                             const float* pair_wpos, const float* pair_wneg, int64_t n_pairs, float l2,
                                             const int32_t* active, float* loss, float* grad, float* hess, void* workspace,
                                             tipk_stream_t stream) {
    const int bad = cal_stats_check(z, n_nodes, dim, rel_w, n_rel, q_rel, ab, n_q, dense_w, pair_ptr, pair_u, pair_v, pair_wpos,
                                    pair_wneg, n_pairs, l2, loss, grad, hess, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_q == 0) return TIPK_OK;
    CalArgs a;
    a.z = z; a.w = rel_w; a.ab = ab; a.dense_w = dense_w; a.qrel = q_rel; a.pair_ptr = pair_ptr; a.pair_u = pair_u;
    a.pair_v = pair_v; a.pair_wpos = pair_wpos; a.pair_wneg = pair_wneg; a.active = active; a.l2 = l2; a.n = (int)n_nodes;
    a.dim = dim; a.n_rel = (int)n_rel; a.n_q = n_q; a.part = reinterpret_cast<double*>(workspace); a.loss = loss; a.grad = grad;
    a.hess = hess;
    return cal_stats_launch(a, (hipStream_t)stream);
}

extern "C" int tipk_distmult_calibrate(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                       const int32_t* q_rel, int64_t n_q, const float* dense_w, const int64_t* pair_ptr,
                                       const int32_t* pair_u, const int32_t* pair_v, const float* pair_wpos,
                                       const float* pair_wneg, int64_t n_pairs, float l2, const float* init, int max_iter,
                                       float gtol, float* out_ab, float* out_loss, float* out_grad, int32_t* out_info,
                                       void* workspace, tipk_stream_t stream) {
    if (max_iter < 0 || !(gtol >= 0.f)) return TIPK_EINVAL;
    if (n_q > 0 && !out_info) return TIPK_EINVAL;
    // the statistics entry's checks: out_ab stands in for its `ab` and out_loss for its `hess` (the fit's own Hessian lives in
    // the workspace) -- cal_stats_check only asks whether these pointers are NULL
    const int bad = cal_stats_check(z, n_nodes, dim, rel_w, n_rel, q_rel, out_ab, n_q, dense_w, pair_ptr, pair_u, pair_v,
                                    pair_wpos, pair_wneg, n_pairs, l2, out_loss, out_grad, out_loss, workspace);
    if (bad != TIPK_OK) return bad;
    if (n_q == 0) return TIPK_OK;
    const NewtonState s = newton_state(workspace, cal_layout(n_nodes, n_q), n_q, 2, out_ab, out_loss, out_grad, out_info);
    hipStream_t st = (hipStream_t)stream;

    CalArgs a;
    a.z = z; a.w = rel_w; a.ab = s.trial; a.dense_w = dense_w; a.qrel = q_rel; a.pair_ptr = pair_ptr; a.pair_u = pair_u;
    a.pair_v = pair_v; a.pair_wpos = pair_wpos; a.pair_wneg = pair_wneg; a.active = s.active; a.l2 = l2; a.n = (int)n_nodes;
    a.dim = dim; a.n_rel = (int)n_rel; a.n_q = n_q; a.part = reinterpret_cast<double*>(workspace);
    a.loss = s.s_loss; a.grad = s.s_grad; a.hess = s.s_hess;
    return newton_run(s, init, nullptr, 1.f, max_iter, gtol, st, [&] { return cal_stats_launch(a, st); });   // start: (1, 0)
}
