// What the two Newton fits on the frozen model share (tipk_side_effect_fit.hip, tipk_drug_fit.hip; include/tipk.h sections 4m,
// 4q): the terms of a logit, the size of a statistics record and the wavefront-local LDS hand-over.  Both fits state their
// arithmetic through these, so they exist once.
#pragma once
#include "tipk_common.h"
#include <math.h>

typedef float sf_f4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t sf_elems(int dim) { return 1 + dim + (int64_t)dim * dim; }      // loss, gradient, Hessian

inline int64_t sf_a256(int64_t b) { return (b + 255) / 256 * 256; }

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
#endif
