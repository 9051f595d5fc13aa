// Fit of DistMult decoder rows for NEW side effects on the frozen embeddings (include/tipk.h section 4m): the statistics
// (loss, gradient, Hessian) of the expected training objective at trial rows, and an entry that enqueues max_iter + 1
// (statistics, step) pairs.  This file holds what is this fit's own: the triangular tiling of the pairs and its walk, the
// staging of a tile and the multiplicity of a pair.  The arithmetic of a tile row, the partial record and the finish body are
// the statistics body of tipk_fit_terms.h, shared with tipk_drug_fit.hip; the step, the state layout, the init launch and the
// loop are tipk_newton.h / tipk_newton.hip.
//
// Statistics, launch 1, fit_dense_kernel: the negative sum over ALL ordered pairs as a mask-free stream over the unordered
//   pairs u <= v in tiles of 64 x 64 (v-block >= u-block; the diagonal tile masked to u <= v), ordered multiplicity 2 (1 for
//   u == v).  A workgroup (4 wavefronts) takes a SLAB -- a contiguous range of tiles -- and a block of SF_RB relations; both
//   row blocks of a tile rest in LDS (16-byte aligned, row stride width + 4 floats: off every multiple of 32 banks).
//   Wavefront w owns the rows u = 16 w .. 16 w + 15 of the tile; per row sf_tile_row with lane = v and the feature
//   f = z[u] * z[v]; the z[v] operands of its 16 MFMA steps stay in registers for the tile.
//   The accumulators stay in registers over the slab; at its end every wavefront writes its partial (loss, g, H) to the
//   workspace: part[relation block][slab][wavefront][relation][1 + dim + dim^2].
// Launch 2, fit_finish_kernel: sf_finish, one workgroup per relation, over the relation's distinct recorded pairs; the l2
//   terms pull to 0.
// A block whose relations are all inactive returns at once; inactive rows of the outputs are not touched.
// No atomics, no workgroup waits for another, every trip count depends on sizes and list lengths only: BITWISE repeatable.
#include "tipk_fit_terms.h"
#include "tipk_newton.h"

namespace {

constexpr int64_t SF_NMAX = 46340;

struct FitStatsArgs : SfStatsArgs {         // x: the trial decoder rows w; ptr: pair_ptr; prior: NULL
    const float* z;
    const int32_t *pair_u, *pair_v;
    int n, T;
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
    const int64_t rb = blockIdx.y, slab = blockIdx.x;

    float dw[SF_RB];
    if (!sf_block_active(a, rb, dw)) return;                    // uniform in the workgroup
    sf_stage_trial<DP>(a, rb, Ws);
    SfAcc<DP> acc;
    sf_zero(acc);

    const int64_t t0 = slab * a.tps, t1 = t0 + a.tps < a.n_tiles ? t0 + a.tps : a.n_tiles;
    int ub = 0, vb;
    {
        int64_t rest = t0;
        while (rest >= a.T - ub) { rest -= a.T - ub; ++ub; }    // (trip count: tile rows)
        vb = ub + (int)rest;
    }

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

        float zva[DP], zvb[16][NH];
        sf_lane_row<DP>(Zv, zva);
        sf_lane_operands<DP>(Zv, zvb);

        const int64_t v = (int64_t)vb * SF_TILE + lane;
        for (int ur = 0; ur < 16; ++ur) {
            const int uu = wave * 16 + ur;
            const int64_t u = (int64_t)ub * SF_TILE + uu;
            if (u >= n) break;                                  // uniform in the wavefront
            const float mult = (v < n && u <= v) ? (u == v ? 1.f : 2.f) : 0.f;
            sf_tile_row<DP>(&Zu[uu * LD], zva, zvb, Ws, dw, mult, coef[wave], acc);
        }
        if (++vb == a.T) { ++ub; vb = ub; }
    }
    sf_write_partial<DP>(a, rb, slab, wave, acc);
}

__global__ void __launch_bounds__(SF_CH) fit_finish_kernel(FitStatsArgs a) {
    __shared__ float fs[SF_CH][SF_DMAX + 1];
    __shared__ float cs[SF_CH][3];
    sf_finish(a, fs, cs, [&a](int64_t p, const float*& zu, const float*& zv) {
        int u = a.pair_u[p], v = a.pair_v[p];
        u = u < 0 ? 0 : (u >= a.n ? a.n - 1 : u);               // (ids in range are the caller's contract; nothing is
        v = v < 0 ? 0 : (v >= a.n ? a.n - 1 : v);               //  read out of bounds)
        zu = a.z + (int64_t)u * a.dim;
        zv = a.z + (int64_t)v * a.dim;
    });
}

struct FitShape : SfSlabs {
    int T;
};

FitShape sf_shape(int64_t n_nodes, int64_t n_fit) {
    const int T = (int)tipk_ceil_div(n_nodes, SF_TILE);
    return FitShape{sf_slabs((int64_t)T * (T + 1) / 2, n_fit), T};
}

// workspace: [dense partials] then the state of tipk_distmult_fit
NewtonLayout sf_layout(int64_t n_nodes, int dim, int64_t n_fit) {
    const FitShape s = sf_shape(n_nodes, n_fit);
    return newton_layout(s.n_blocks * s.slabs * SF_NW * SF_RB * sf_elems(dim) * 4, n_fit, dim);
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

// the statistics at the rows w into (loss, grad, hess); part: the workspace's partials
FitStatsArgs sf_stats_args(const float* z, int64_t n_nodes, int dim, const float* w, int64_t n_fit, const float* dense_w,
                           const int64_t* pair_ptr, const int32_t* pair_u, const int32_t* pair_v, const float* pair_wpos,
                           const float* pair_wneg, float l2, const int32_t* active, float* loss, float* grad, float* hess,
                           void* part) {
    const FitShape s = sf_shape(n_nodes, n_fit);
    FitStatsArgs a;
    a.x = w; a.dense_w = dense_w; a.prior = nullptr; a.ptr = pair_ptr; a.wpos = pair_wpos; a.wneg = pair_wneg; a.active = active;
    a.l2 = l2; a.dim = dim; a.slabs = s.slabs; a.n_fit = n_fit; a.n_tiles = s.n_tiles; a.tps = s.tps;
    a.part = reinterpret_cast<float*>(part); a.loss = loss; a.grad = grad; a.hess = hess;
    a.z = z; a.pair_u = pair_u; a.pair_v = pair_v; a.n = (int)n_nodes; a.T = s.T;
    return a;
}

int sf_stats_launch(const FitStatsArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.slabs, (unsigned)tipk_ceil_div(a.n_fit, SF_RB));
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
    return sf_max_chain(sf_shape(n_nodes, n_fit), n_nodes * (n_nodes + 1) / 2);     // at most n (n + 1) / 2 distinct pairs
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
    return sf_stats_launch(sf_stats_args(z, n_nodes, dim, w, n_fit, dense_w, pair_ptr, pair_u, pair_v, pair_wpos, pair_wneg, l2,
                                         active, loss, grad, hess, workspace),
                           (hipStream_t)stream);
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
    const NewtonLayout l = sf_layout(n_nodes, dim, n_fit);
    const NewtonState s = newton_state(workspace, l, n_fit, dim, out_w, out_loss, out_grad, out_info);
    hipStream_t st = (hipStream_t)stream;
    const FitStatsArgs a = sf_stats_args(z, n_nodes, dim, s.trial, n_fit, dense_w, pair_ptr, pair_u, pair_v, pair_wpos,
                                         pair_wneg, l2, s.active, s.s_loss, s.s_grad, s.s_hess, workspace);
    return newton_run(s, init, nullptr, 0.f, max_iter, gtol, st, [&] { return sf_stats_launch(a, st); });
}
