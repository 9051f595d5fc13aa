// Fit of the embedding of NEW drugs to their recorded (partner, side effect) reports, embeddings and DistMult decoder frozen
// (include/tipk.h section 4q): the statistics (loss, gradient, Hessian) of the expected training objective at trial rows, and
// an entry that enqueues max_iter + 1 (statistics, step) pairs.  The dual of tipk_side_effect_fit.hip (4m): there the unknown
// is a decoder row and a term is a pair of drugs, here the unknown is an embedding row and a term is a CELL (partner v, side
// effect r) with the feature f = z[v] * rel_w[r].  This file holds what is this fit's own: the rectangular tiling of the
// cells and its walk, and the staging of a tile.  The arithmetic of a tile row, the partial record and the finish body are
// the statistics body of tipk_fit_terms.h, shared with 4m; the step, the state layout, the init launch and the loop are
// tipk_newton.h / tipk_newton.hip.
//
// Statistics, launch 1, drug_dense_kernel: the negative sum as a mask-free stream over ALL n x R cells in RECTANGULAR tiles of
//   64 partners x 64 side effects, numbered partner-block major.  A workgroup (4 wavefronts) takes a SLAB -- a contiguous range
//   of tiles -- and a block of SF_RB new drugs; the tile's z rows and rel_w rows rest in LDS (16-byte aligned, row stride
//   width + 4 floats: off every multiple of 32 banks); the z rows are staged again only when the partner block changes.
//   Wavefront w owns the partners v = 16 w .. 16 w + 15 of the tile; per partner sf_tile_row with lane = side effect r
//   (multiplicity 1; 0 behind the last side effect); the rel_w operands of its 16 MFMA steps stay in registers for the tile.
//   The accumulators stay in registers over the slab; at its end every wavefront writes its partial (loss, g, H) to the
//   workspace: part[drug block][slab][wavefront][drug][1 + dim + dim^2].
// Launch 2, drug_finish_kernel: sf_finish, one workgroup per drug, over the drug's distinct recorded cells; the l2 terms pull
//   to the prior centre.
// A block whose drugs are all inactive returns at once; inactive rows of the outputs are not touched.
// No atomics, no workgroup waits for another, every trip count depends on sizes and list lengths only: BITWISE repeatable.
#include "tipk_fit_terms.h"
#include "tipk_newton.h"

namespace {

constexpr int64_t DF_CELLMAX = 0x7fffffffLL;            // n * R must stay below 2^31

struct DrugStatsArgs : SfStatsArgs {        // x: the trial embedding rows; ptr: rec_ptr
    const float *z, *rel_w;
    const int32_t *rec_v, *rec_r;
    int n, n_rel, TR;
};

// At most 3 wavefronts per SIMD.  Left alone, the allocator squeezes the dim <= 16 kernel into the 128 registers that a
// fourth wavefront needs, and that code measured 8 % slower at 64 drugs (800 workgroups, about three per CU: the fourth
// brings no more work in); with the cap it times as it did before the row body was shared.  The dim 32 kernel has 2
// wavefronts with or without it; the cap only changes how its 238 registers are split.  Both widths are timed in
// profiles/fit_shared.md.  The cap answers one compiler's allocation: measure again when the toolchain changes.
template <int DP>
__global__ void __launch_bounds__(SF_NT) __attribute__((amdgpu_waves_per_eu(2, 3))) drug_dense_kernel(DrugStatsArgs a) {
    constexpr int NH = DP / 16;
    constexpr int LD = DP + SF_PAD;
    __shared__ __attribute__((aligned(16))) float Zp[SF_TILE * LD];         // z rows of the tile's partners
    __shared__ __attribute__((aligned(16))) float Wr[SF_TILE * LD];         // rel_w rows of the tile's side effects
    __shared__ __attribute__((aligned(16))) float Xs[SF_RB * DP];           // the block's trial rows
    __shared__ __attribute__((aligned(16))) float coef[SF_NW][TIPK_WAVE][SF_CW];

    const int t = threadIdx.x, lane = tipk_lane(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n, n_rel = a.n_rel, dim = a.dim;
    const int64_t db = blockIdx.y, slab = blockIdx.x;

    float dw[SF_RB];
    if (!sf_block_active(a, db, dw)) return;                    // uniform in the workgroup
    sf_stage_trial<DP>(a, db, Xs);
    SfAcc<DP> acc;
    sf_zero(acc);

    const int64_t t0 = slab * a.tps, t1 = t0 + a.tps < a.n_tiles ? t0 + a.tps : a.n_tiles;
    int pb = (int)(t0 / a.TR), rb = (int)(t0 - (int64_t)pb * a.TR), staged = -1;

    for (int64_t tt = t0; tt < t1; ++tt) {
        __syncthreads();                                        // the previous tile has been read; Xs is staged
        const bool fresh = staged != pb;                        // uniform
        for (int i = t; i < SF_TILE * (DP / 4); i += SF_NT) {
            const int r = i / (DP / 4), q = i - r * (DP / 4);
            const int64_t rp = (int64_t)pb * SF_TILE + r, rr = (int64_t)rb * SF_TILE + r;
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

        float wra[DP], wrb[16][NH];
        sf_lane_row<DP>(Wr, wra);
        sf_lane_operands<DP>(Wr, wrb);

        const float one = (int64_t)rb * SF_TILE + lane < n_rel ? 1.f : 0.f;
        for (int vr = 0; vr < 16; ++vr) {
            const int vv = wave * 16 + vr;
            if ((int64_t)pb * SF_TILE + vv >= n) break;         // uniform in the wavefront
            sf_tile_row<DP>(&Zp[vv * LD], wra, wrb, Xs, dw, one, coef[wave], acc);
        }
        if (++rb == a.TR) { rb = 0; ++pb; }
    }
    sf_write_partial<DP>(a, db, slab, wave, acc);
}

__global__ void __launch_bounds__(SF_CH) drug_finish_kernel(DrugStatsArgs a) {
    __shared__ float fs[SF_CH][SF_DMAX + 1];
    __shared__ float cs[SF_CH][3];
    sf_finish(a, fs, cs, [&a](int64_t p, const float*& zv, const float*& wr) {
        int v = a.rec_v[p], r = a.rec_r[p];
        v = v < 0 ? 0 : (v >= a.n ? a.n - 1 : v);               // (ids in range are the caller's contract; nothing is
        r = r < 0 ? 0 : (r >= a.n_rel ? a.n_rel - 1 : r);       //  read out of bounds)
        zv = a.z + (int64_t)v * a.dim;
        wr = a.rel_w + (int64_t)r * a.dim;
    });
}

struct DrugShape : SfSlabs {
    int TR;
};

DrugShape df_shape(int64_t n_nodes, int64_t n_rel, int64_t n_fit) {
    const int TR = (int)tipk_ceil_div(n_rel, SF_TILE);
    return DrugShape{sf_slabs(tipk_ceil_div(n_nodes, SF_TILE) * TR, n_fit), TR};
}

// workspace: [dense partials] then the state of tipk_distmult_drug_fit
NewtonLayout df_layout(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    const DrugShape s = df_shape(n_nodes, n_rel, n_fit);
    return newton_layout(s.n_blocks * s.slabs * SF_NW * SF_RB * sf_elems(dim) * 4, n_fit, dim);
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

// the statistics at the rows x into (loss, grad, hess); part: the workspace's partials
DrugStatsArgs df_stats_args(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel, const float* x,
                            int64_t n_fit, const float* dense_w, const int64_t* rec_ptr, const int32_t* rec_v,
                            const int32_t* rec_r, const float* rec_wpos, const float* rec_wneg, const float* prior, float l2,
                            const int32_t* active, float* loss, float* grad, float* hess, void* part) {
    const DrugShape s = df_shape(n_nodes, n_rel, n_fit);
    DrugStatsArgs a;
    a.x = x; a.dense_w = dense_w; a.prior = prior; a.ptr = rec_ptr; a.wpos = rec_wpos; a.wneg = rec_wneg; a.active = active;
    a.l2 = l2; a.dim = dim; a.slabs = s.slabs; a.n_fit = n_fit; a.n_tiles = s.n_tiles; a.tps = s.tps;
    a.part = reinterpret_cast<float*>(part); a.loss = loss; a.grad = grad; a.hess = hess;
    a.z = z; a.rel_w = rel_w; a.rec_v = rec_v; a.rec_r = rec_r; a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.TR = s.TR;
    return a;
}

int df_stats_launch(const DrugStatsArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.slabs, (unsigned)tipk_ceil_div(a.n_fit, SF_RB));
    if (a.dim <= 16) hipLaunchKernelGGL(drug_dense_kernel<16>, grid, dim3(SF_NT), 0, st, a);
    else hipLaunchKernelGGL(drug_dense_kernel<32>, grid, dim3(SF_NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(drug_finish_kernel, dim3((unsigned)a.n_fit), dim3(SF_CH), 0, st, a);
    TIPK_RETURN_LAUNCH();
}

}  // namespace

extern "C" int tipk_distmult_drug_fit_supported(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    return n_nodes >= 1 && n_rel >= 1 && n_nodes <= DF_CELLMAX && n_rel <= DF_CELLMAX && n_nodes * n_rel <= DF_CELLMAX &&
           dim >= 4 && dim <= SF_DMAX && dim % 4 == 0 && n_fit >= 1 && n_fit <= SF_FITMAX;
}

extern "C" int64_t tipk_distmult_drug_fit_slabs(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit)) return -1;
    return df_shape(n_nodes, n_rel, n_fit).slabs;
}

extern "C" int64_t tipk_distmult_drug_fit_max_chain(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit) {
    if (!tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit)) return -1;
    return sf_max_chain(df_shape(n_nodes, n_rel, n_fit), n_nodes * n_rel);          // at most n R distinct cells
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
    return df_stats_launch(df_stats_args(z, n_nodes, dim, rel_w, n_rel, x, n_fit, dense_w, rec_ptr, rec_v, rec_r, rec_wpos,
                                         rec_wneg, prior, l2, active, loss, grad, hess, workspace),
                           (hipStream_t)stream);
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
    const NewtonLayout l = df_layout(n_nodes, dim, n_rel, n_fit);
    const NewtonState s = newton_state(workspace, l, n_fit, dim, out_x, out_loss, out_grad, out_info);
    hipStream_t st = (hipStream_t)stream;
    DrugStatsArgs a = df_stats_args(z, n_nodes, dim, rel_w, n_rel, s.trial, n_fit, dense_w, rec_ptr, rec_v, rec_r, rec_wpos,
                                    rec_wneg, prior, l2, s.active, s.s_loss, s.s_grad, s.s_hess, workspace);
    const int status = newton_run(s, init, prior, 0.f, max_iter, gtol, st, [&] { return df_stats_launch(a, st); });
    if (status != TIPK_OK || !out_hess) return status;
    a.x = out_x; a.active = nullptr; a.hess = out_hess;         // the Hessian of the accepted rows: one more statistics pair
    return df_stats_launch(a, st);                              // (its loss and gradient go to the spent statistics slots)
}
