// The one Cholesky of the wave-per-row kernels (tipk_side_effect_fit.hip `newton_step_kernel`, tipk_pair_conf.hip
// `spd_factor_kernel`; include/tipk.h sections 4m, 4p): both must factor a Hessian to the same bits, so the loop exists once.
#pragma once
#include "tipk_common.h"

constexpr int CH_DMAX = 32;                 // widest matrix: lane i < dim owns row i

#ifdef __HIPCC__
// Right-looking Cholesky in LDS by ONE wavefront that is the whole workgroup (the barriers are __syncthreads()): on entry
// L[i][c], c <= i, holds the lower triangle of the matrix (visible to the wave); on exit its factor, L[i][k], i >= k.  Column
// k: d = sqrtf(pivot), the lanes i > k divide their entry by d, then update their row with one fmaf per entry, c ascending.
// false: a pivot that is not > 0 or not finite (uniform: every lane reads L[k][k]); L is then left half way.
__device__ __forceinline__ bool ch_factor(float (*L)[CH_DMAX + 1], int dim, int lane) {
    const bool own = lane < dim;
    bool ok = true;
    for (int k = 0; k < dim; ++k) {
        const float piv = L[k][k];
        if (!(piv > 0.f) || piv - piv != 0.f) { ok = false; break; }       // uniform: every lane reads L[k][k]
        const float d = sqrtf(piv);
        __syncthreads();
        if (own && lane > k) L[lane][k] = L[lane][k] / d;
        if (lane == k) L[k][k] = d;
        __syncthreads();
        if (own && lane > k) {
            const float lik = L[lane][k];
            for (int c = k + 1; c <= lane; ++c) L[lane][c] = fmaf(-lik, L[c][k], L[lane][c]);
        }
        __syncthreads();
    }
    return ok;
}
#endif
