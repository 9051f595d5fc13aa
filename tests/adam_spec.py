"""fp64 specification of one Adam step (include/tipk.h section 9) and the acceptance rule `tipk_adam_step` is held to.

Plain numpy on the CPU; nothing of tip_amd is imported here.

The rule, for fp32 state (p, g, m, v), step number t = steps done + 1 and DOUBLE hyper-parameters (`adam_step64`):
    g' = g + wd p;   M = m + (1 - beta1)(g' - m);   V = beta2 v + (1 - beta2) g'^2;
    P  = p - lr / (1 - beta1^t) * M / (sqrt(V) / sqrt(1 - beta2^t) + eps)

The acceptance bound (`adam_bounds`) counts fp32 roundings, u = 2^-24, G = |g| + wd |p|.  It assumes correctly rounded `/`
and `sqrtf` (the hipcc default) and that every hyper-parameter constant the kernel uses -- beta1, beta2, 1 - beta1,
1 - beta2, wd, eps, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) -- is ONE rounding away from its double value:
    dg   = 2u G if wd != 0 else 0               (wd rounded, the fma rounded; G bounds |wd p| and |g'|)
    dM   = u |M| + (1 - beta1)(2u (G + |m|) + dg)
                                                (g' - m rounded, 1 - beta1 rounded, g' off by dg; the final fma rounded)
    dV   = 3u V + 2 (1 - beta2) G dg            (beta2 rounded, beta2 v rounded, g'g' rounded, 1 - beta2 rounded: each
                                                 touches only ITS term of V, two each, <= 2u V; the final fma rounded)
    S    = sqrt(V) / sqrt(1 - beta2^t),  DEN = S + eps
    dDEN = 5u DEN + (dV / 2V) S                 (sqrtf, the bias constant, their product, eps, the sum; V's own error through
                                                 the root; that term is 0 where V == 0)
    Q    = M / DEN
    dQ   = u |Q| + dM / DEN + |Q| dDEN / DEN    (the quotient rounded, numerator and denominator errors)
    dP   = u |P| + lr / (1 - beta1^t) dQ + 2u |P - p|
                                                (the step constant rounded, its product with Q rounded, the difference rounded)
each times 1.01 for the second-order terms.  Contracting `sqrt * c + eps` or `p - s q` to an fma drops a rounding and stays
inside.  Where a bound is 0 the values must be equal (`check` compares with <=).  No constant here was fitted to a kernel's
output.

`emulate_fp32` is the kernel's operation order in numpy fp32, with the complement form ((float)(1 - beta), or
1.0f - (float)beta, which is many u away from 1 - beta: 216 u for beta = 0.999) and the two contractions as flags.  Its
fmas are float32(double product + double addend): the product is exact, the double sum rounds once more before the final
rounding, which can differ from a true fma only on a near-tie of that double rounding.

Largest share of each bound used, all elements of all cases:
    emulate_fp32 with (float)(1 - beta), plain and contracted (tests/test_host_adam_spec.py):  dP 0.986  dM 0.885  dV 0.894
    tipk_adam_step on an MI355X, all 65 cases (tests/test_gpu_adam_edges.py):                 dP 0.989  dM 0.890  dV 0.898
With 1.0f - (float)beta the same GPU cases were outside by up to 919 x dV (beta2 = 0.9999; 72 x for 0.999), 128 x dP, 2.5 x dM.
"""
import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.01

# the hyper-parameter sets and step counts of the rule cases (tests/test_gpu_adam_edges.py, tests/test_host_adam_spec.py)
HYPER = {
    'default': dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0),
    'decay': dict(lr=0.003, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.01),
    'beta2_9999': dict(lr=0.01, beta1=0.9, beta2=0.9999, eps=1e-8, weight_decay=0.0),
    'betas_0': dict(lr=0.01, beta1=0.0, beta2=0.0, eps=1e-8, weight_decay=0.0),
    'eps_0': dict(lr=0.01, beta1=0.9, beta2=0.999, eps=0.0, weight_decay=0.0),
    'lr_0': dict(lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0),
    'decay_0.1': dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1),
}
STEPS_DONE = (0, 6, 999, 10 ** 6 - 1, 2 ** 33 + 4)


def _f64(*xs):
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in xs)


def bias_corrections(t, beta1, beta2):
    """(1 - beta1^t, 1 - beta2^t) in double; t a python int (it may exceed 2^32)."""
    return 1.0 - float(beta1) ** int(t), 1.0 - float(beta2) ** int(t)


def adam_step64(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    """One step of the rule in fp64 from fp32 state -> (P, M, V)."""
    p, g, m, v = _f64(p, g, m, v)
    bc1, bc2 = bias_corrections(t, beta1, beta2)
    with np.errstate(all='ignore'):
        gp = g + weight_decay * p if weight_decay != 0.0 else g
        M = m + (1.0 - beta1) * (gp - m)
        V = beta2 * v + (1.0 - beta2) * gp * gp
        P = p - lr / bc1 * (M / (np.sqrt(V) / np.sqrt(bc2) + eps))
    return P, M, V


def adam_bounds(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    """Per-element acceptance bounds (dP, dM, dV) of the module docstring (non-finite where the spec is)."""
    P, M, V = adam_step64(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay)
    p, g, m, v = _f64(p, g, m, v)
    bc1, bc2 = bias_corrections(t, beta1, beta2)
    with np.errstate(all='ignore'):
        G = np.abs(g) + weight_decay * np.abs(p)
        dg = 2 * U * G if weight_decay != 0.0 else np.zeros_like(G)
        dM = U * np.abs(M) + (1.0 - beta1) * (2 * U * (G + np.abs(m)) + dg)
        dV = 3 * U * V + 2 * (1.0 - beta2) * G * dg
        S = np.sqrt(V) / np.sqrt(bc2)
        DEN = S + eps
        dDEN = 5 * U * DEN + np.where(V == 0.0, 0.0, dV / (2 * np.where(V == 0.0, 1.0, V)) * S)
        Q = M / DEN
        dQ = U * np.abs(Q) + dM / DEN + np.abs(Q) * dDEN / DEN
        dP = U * np.abs(P) + lr / bc1 * dQ + 2 * U * np.abs(P - p)
    return SECOND_ORDER * dP, SECOND_ORDER * dM, SECOND_ORDER * dV


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_fp32(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, float_complements=False, contract=False):
    """The kernel's operation order in fp32 -> (P, M, V) float32.  float_complements: 1.0f - (float)beta in place of
    (float)(1 - beta).  contract: sqrt(v) * c + eps and p - s q as one fma each."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    bc1, bc2 = bias_corrections(t, beta1, beta2)
    b1, b2, wd, e = f(beta1), f(beta2), f(weight_decay), f(eps)
    c1, c2 = (f(1.0) - b1, f(1.0) - b2) if float_complements else (f(1.0 - beta1), f(1.0 - beta2))
    step_size, inv_sqrt_bc2 = f(lr / bc1), f(1.0 / np.sqrt(bc2))
    full = lambda x: np.full(p.shape, x, dtype=f)
    with np.errstate(all='ignore'):
        if wd != 0.0:
            g = _fma32(full(wd), p, g)
        M = _fma32(full(c1), g - m, m)
        V = _fma32(full(c2), g * g, b2 * v)
        r = np.sqrt(V)
        den = _fma32(r, full(inv_sqrt_bc2), full(e)) if contract else r * inv_sqrt_bc2 + e
        q = M / den
        P = _fma32(full(-step_size), q, p) if contract else p - step_size * q
    return P, M, V


def check(got, before, t, hyper, what=''):
    """Hold got = (P, M, V) float32 arrays to the rule, one step from before = (p, g, m, v) -> the largest share of each
    bound used, {'dP', 'dM', 'dV'}.  EVERY element is held: where the spec is finite the error is <= the bound (a bound of
    0 means equality), where it is not the result is non-finite in the same way (NaN, +inf, -inf)."""
    want = adam_step64(*before, t, **hyper)
    bounds = adam_bounds(*before, t, **hyper)
    used, failed = {}, []
    for name, a, w, b in zip(('dP', 'dM', 'dV'), got, want, bounds):
        a = np.asarray(a, dtype=np.float32).astype(np.float64)
        assert a.shape == w.shape, (what, name, 'shape')
        for kind, mask_a, mask_w in (('NaN', np.isnan(a), np.isnan(w)), ('+inf', np.isposinf(a), np.isposinf(w)),
                                     ('-inf', np.isneginf(a), np.isneginf(w))):
            assert np.array_equal(mask_a, mask_w), (what, name, kind + ' at other elements than the rule\'s',
                                                    np.flatnonzero(mask_a != mask_w)[:8].tolist())
        fin = np.isfinite(w)
        assert bool(np.isfinite(b[fin]).all()), (what, name, 'non-finite bound beside a finite value')
        err = np.abs(a[fin] - w[fin])
        bad = err > b[fin]
        share = float((err / np.maximum(b[fin], 1e-300))[b[fin] > 0].max()) if bool((b[fin] > 0).any()) else 0.0
        if bool(bad.any()):
            i = np.flatnonzero(fin)[np.flatnonzero(bad)]
            worst = float((err[bad] / np.maximum(b[fin][bad], 1e-300)).max())
            failed.append('%s: %d of %d elements outside the bound, worst %.3g x the bound (first at %s)'
                          % (name, int(bad.sum()), int(fin.sum()), worst, i[:8].tolist()))
        used[name] = share
    assert not failed, (what, failed)
    return used


def rule_state(n, steps_done, seed, zero_g=True):
    """The state of a rule case -> (p, g, m, v) float32 [n]: |p| over 1e-3 ... 1, |g| over 1e-4 ... 10 (log-uniform, random
    sign), every 7th g zero (zero_g); before the first step m = v = 0, later |m| over 1e-4 ... 10, v over 1e-9 ... 100
    with every 14th m and v zero (so that g = m = v = 0 there)."""
    r = np.random.default_rng(seed)
    mag = lambda lo, hi: 10.0 ** r.uniform(lo, hi, n)
    sign = lambda: r.choice([-1.0, 1.0], n)
    p, g = (sign() * mag(-3, 0)).astype(np.float32), (sign() * mag(-4, 1)).astype(np.float32)
    m, v = (sign() * mag(-4, 1)).astype(np.float32), mag(-9, 2).astype(np.float32)
    if zero_g:
        g[::7] = 0.0
    if steps_done == 0:
        m[:], v[:] = 0.0, 0.0
    m[::14], v[::14] = 0.0, 0.0
    return p, g, m, v
