// The kernels of the damped Newton iteration of tipk_newton.h (include/tipk.h section 4m, `tipk_newton_step`).
//
// Step, newton_step_kernel: one wavefront per row; lane j owns component j.  Armijo test with 16 ulp slack, Cholesky of the
//   trial Hessian in LDS (ch_factor of tipk_chol.h: right-looking, column k by the lanes i > k), the two triangular solves
//   with the vector in registers (one shuffle per column); a pivot that is not > 0 gives the scaled steepest-descent
//   direction.
// Init, newton_init_kernel: one thread per component of the state.
#include "tipk_chol.h"
#include "tipk_newton.h"
#include <math.h>

namespace {

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
    __shared__ float L[CH_DMAX][CH_DMAX + 1];
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
        L[own ? lane : 0][own ? c : CH_DMAX] = hv;              // (lanes behind dim write the spare column of row 0)
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

struct InitArgs {
    const float *init, *fallback;
    float x0;
    NewtonState s;
};

__global__ void __launch_bounds__(256) newton_init_kernel(InitArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const NewtonState& s = a.s;
    if (i < s.n_fit * s.dim) {
        const float v = a.init ? a.init[i] : (a.fallback ? a.fallback[i] : (i % s.dim == 0 ? a.x0 : 0.f));
        s.x[i] = v; s.trial[i] = v; s.grad[i] = 0.f; s.p[i] = 0.f;
    }
    if (i < s.n_fit) {
        s.loss[i] = 0.f; s.t[i] = 1.0f; s.active[i] = 1;
        s.info[4 * i] = 0; s.info[4 * i + 1] = 0; s.info[4 * i + 2] = 0; s.info[4 * i + 3] = 0;
    }
}

}  // namespace

int newton_init(const NewtonState& s, const float* init, const float* fallback, float x0, hipStream_t st) {
    const InitArgs a{init, fallback, x0, s};
    hipLaunchKernelGGL(newton_init_kernel, dim3((unsigned)tipk_ceil_div(s.n_fit * s.dim, 256)), dim3(256), 0, st, a);
    TIPK_RETURN_LAUNCH();
}

extern "C" int tipk_newton_step(int dim, int64_t n_fit, const float* stat_loss, const float* stat_grad, const float* stat_hess,
                                float gtol, float* w, float* loss, float* grad, float* p, float* t, int32_t* info,
                                float* w_trial, int32_t* active, tipk_stream_t stream) {
    if (dim < 1 || n_fit < 0 || !(gtol >= 0.f)) return TIPK_EINVAL;
    if (n_fit > 0 && (!stat_loss || !stat_grad || !stat_hess || !w || !loss || !grad || !p || !t || !info || !w_trial || !active))
        return TIPK_EINVAL;
    if (dim > CH_DMAX || n_fit > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if (n_fit == 0) return TIPK_OK;
    StepArgs a;
    a.s_loss = stat_loss; a.s_grad = stat_grad; a.s_hess = stat_hess; a.w = w; a.loss = loss; a.grad = grad; a.p = p; a.t = t;
    a.w_trial = w_trial; a.info = info; a.active = active; a.n_fit = n_fit; a.dim = dim; a.gtol = gtol;
    hipLaunchKernelGGL(newton_step_kernel, dim3((unsigned)n_fit), dim3(TIPK_WAVE), 0, (hipStream_t)stream, a);
    TIPK_RETURN_LAUNCH();
}
