// The damped Newton iteration every fit on the frozen model runs (tipk_side_effect_fit.hip, tipk_drug_fit.hip,
// tipk_calibrate.hip; include/tipk.h sections 4m, 4q, 4r): where its state lives in the caller's workspace, the launch that
// initialises it, and the driver that enqueues max_iter + 1 (statistics, tipk_newton_step) pairs.  A fit brings its
// statistics launches; the kernels are in tipk_newton.hip.
#pragma once
#include "tipk_common.h"

// workspace of a fit entry: [the statistics' own partials] then the state, every array on a multiple of 256 bytes
struct NewtonLayout {
    int64_t part, p, t, trial, active, s_loss, s_grad, s_hess, total;
};

inline NewtonLayout newton_layout(int64_t part_bytes, int64_t n_fit, int dim) {
    const auto a256 = [](int64_t b) { return (b + 255) / 256 * 256; };
    NewtonLayout l;
    int64_t o = 0;
    l.part = o; o += a256(part_bytes);
    l.p = o; o += a256(n_fit * dim * 4);
    l.t = o; o += a256(n_fit * 4);
    l.trial = o; o += a256(n_fit * dim * 4);
    l.active = o; o += a256(n_fit * 4);
    l.s_loss = o; o += a256(n_fit * 4);
    l.s_grad = o; o += a256(n_fit * dim * 4);
    l.s_hess = o; o += a256(n_fit * dim * dim * 4);
    l.total = o;
    return l;
}

// the arrays of one run: the caller's outputs (accepted rows x, their loss and gradient, info) and the workspace's
struct NewtonState {
    float *x, *loss, *grad;
    int32_t* info;
    float *p, *t, *trial;
    int32_t* active;
    float *s_loss, *s_grad, *s_hess;        // where the statistics of the trial rows go
    int64_t n_fit;
    int dim;
};

inline NewtonState newton_state(void* workspace, const NewtonLayout& l, int64_t n_fit, int dim, float* x, float* loss,
                                float* grad, int32_t* info) {
    char* ws = reinterpret_cast<char*>(workspace);
    const auto f = [ws](int64_t o) { return reinterpret_cast<float*>(ws + o); };
    return NewtonState{x, loss, grad, info, f(l.p), f(l.t), f(l.trial), reinterpret_cast<int32_t*>(ws + l.active),
                       f(l.s_loss), f(l.s_grad), f(l.s_hess), n_fit, dim};
}

// x = trial = the start rows, everything else of the state cleared, all rows active.  The start row is init's, else
// fallback's, else (x0, 0, ..., 0); init, fallback: [n_fit, dim] or NULL.  (Hidden: no entry in the library's dynamic symbols)
__attribute__((visibility("hidden"))) int newton_init(const NewtonState& s, const float* init, const float* fallback, float x0,
                                                      hipStream_t st);

// The init launch, then max_iter + 1 times: stats() -- enqueues the statistics of s.trial into s.s_loss, s.s_grad, s.s_hess,
// skipping the rows with s.active == 0 -- and tipk_newton_step.  The first status that is not TIPK_OK is returned at once.
template <class Stats>
int newton_run(const NewtonState& s, const float* init, const float* fallback, float x0, int max_iter, float gtol,
               hipStream_t st, Stats stats) {
    int status = newton_init(s, init, fallback, x0, st);
    for (int it = 0; it <= max_iter && status == TIPK_OK; ++it) {
        status = stats();
        if (status != TIPK_OK) break;
        status = tipk_newton_step(s.dim, s.n_fit, s.s_loss, s.s_grad, s.s_hess, gtol, s.x, s.loss, s.grad, s.p, s.t, s.info,
                                  s.trial, s.active, (tipk_stream_t)st);
    }
    return status;
}
