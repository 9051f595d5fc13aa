"""fp64 specification of the DistMult decoder outside its fused fast path (include/tipk.h section 4) and the acceptance rule
`tipk_distmult_fwd`, `tipk_distmult_bwd` and the generic `tipk_distmult_loss` are held to.

Plain torch on the CPU; nothing of tip_amd is imported here.  The reference is `oracle.tip_oracle` in fp64 (`distmult_fwd`,
`distmult_bwd`, `tip_loss`, `tip_loss_bwd`) from the fp32 inputs.

The bound counts fp32 roundings, u = 2^-24, gamma(m) = m u / (1 - m u).  No constant here was fitted to a kernel's output.

  logit   s = sum_j (z[u,j] z[v,j]) w[r,j]: every term carries two roundings (the two products; an fma drops one), and it passes
          through at most k adds, in any order (the chain of the one-thread kernels, the shuffle tree of the task kernel):
              ds = gamma(k + 2) sum_j |z[u,j] z[v,j] w[r,j]|
  score   sigma(s) = 1 / (1 + e), e = expf(-s).  expf is documented at <= 1 ulp = 2u relative, the add and the divide round once:
              dsigma = sigma (1 - sigma) (ds + 2u) + 2u sigma + TINY
          (d sigma / d e = -sigma^2, so a relative error r of e moves sigma by r sigma (1 - sigma); TINY = 2^-126: where e overflows
          the fp32 score is 0 and the fp64 one a number below the normal range).
  d z, d w (upstream g given)   an element is the sum of its n contributions q t -- q the triple's coefficient, t the product of the
          two other factors (two roundings, or one product and one fma) -- IN ANY ORDER: float atomics, the LDS image and its flush,
          the wave and workgroup reductions are all summation trees in which a term meets at most n adds (n counted per element:
          a self-pair u = v adds to its row twice), plus the flush add into the output:
              d = gamma(n + 3) sum |q t| + sum dq |t|
          q = g without the sigmoid (dq = 0).  With it q = g s (1 - s), s the fp32 score (read back by the generic routes,
          recomputed by the task route from its own dot product -- the same dsigma): 1 - s, the product and the product with g round:
              dq = |g| (|1 - 2 sigma| dsigma + dsigma^2 + 3u sigma (1 - sigma))
  task route   its d z image is fixed point: a contribution is TRUNCATED to a multiple of 2^-ex, ex = 59 - ilogb(B) capped at 180, B the
          workgroup's bound 4 max|z| max|w| sum |g| <= the whole list's, so every contribution adds < max(2^-59 B, 2^-180):
              d += n max(2^-59 B (1 + 2^-20), 2^-180)
          (B itself is an fp32 sum: the factor covers its roundings for fewer than 2^20 positions per workgroup.)  The conversion
          back rounds once per workgroup and the workgroups' floats are added by atomics: inside the n + 3 above.
  objective (generic kernel, accurate expf / logf)   with h(t) = t (1 - t) / (t + eps), eps = 1e-13:
          loss = -1/n sum log(sp + eps) + log(1 - sn + eps),   coefficients cp = -h(sp) / n,  cn = h(1 - sn) / n.
          The fp32 argument t' (sp, or 1 - sn) is off by dt = dsigma + u t; near saturation h and log are NOT flat over that
          interval (h rises from 0 to ~1 within a few eps), so their change is taken over the whole interval [t - dt, t + dt]
          (clipped to [0, 1]; h is unimodal with its peak at t* = -eps + sqrt(eps^2 + eps), log is monotone):
              dlog = max |log(t' + eps) - log(t + eps)| + 2u |log(t + eps)| + 2u      (logf <= 1 ulp; the add of eps)
              dh   = max |h(t') - h(t)| + 6u max h                                     (1 - t, two products, the sum, the quotient,
                                                                                        1/n and its product: <= 7 with the next line)
              dloss = gamma(m) / n sum |log terms| + 1/n sum dlog,   m = per_block / 256 + blocks + 12
          The objective's sum is NOT an any-order sum: it is the kernel's reduction tree, and a log term meets the add of its
          position's two logs, at most per_block / 256 adds in its lane (`loss_launch`: the launch shape of the generic kernel),
          6 in the wave, 3 across the four waves, the product with 1/n (itself rounded) and the atomics of `blocks` workgroups:
          m adds in all, where an any-order count would allow 2n.
              d z, d w: as above with q = c, dq = dh / n + 2u |c|
each times 1.01 for the second-order terms.  Where a bound is 0 the values must be equal.

Non-finite elements: where the fp64 value is NaN or infinite the result must not be a finite number (`check`); the forward is held
to the same KIND (NaN where fp64 is NaN, the same infinity).

`emulate` is the same formulas in plain torch float32 on the CPU, the sums in a seeded random order of the triples.

Largest share of each bound used -- see profiles/distmult_routes_errors.md (an MI355X) and tests/test_host_distmult_cases.py (the emulation).
"""
import math

import torch

from oracle import tip_oracle as O

U = 2.0 ** -24
SECOND_ORDER = 1.01
TINY = 2.0 ** -126
EPS = 1e-13
F32_MAX = 3.4028234663852886e38


def gamma(m):
    m = torch.as_tensor(m, dtype=torch.float64)
    return m * U / (1.0 - m * U)


def _d(*ts):
    return tuple(t.detach().to('cpu', torch.float64) for t in ts)


def _rows(z, w, u, v, r):
    return z[u], z[v], w[r]


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def logit_bound(z, w, u, v, r):
    z, w = _d(z, w)
    zu, zv, wr = _rows(z, w, u, v, r)
    return SECOND_ORDER * gamma(z.shape[1] + 2) * (zu * zv * wr).abs().sum(1)


def _dsigma(s, ds):
    sg = torch.sigmoid(s)
    # (an infinite logit is the same infinity in fp32 -- `check(..., same_kind=True)` -- and its sigma is exactly 0 or 1)
    slope = torch.where(torch.isinf(s), torch.zeros_like(s), sg * (1 - sg) * (ds + 2 * U))
    return slope + 2 * U * sg + TINY


def fwd_reference(z, w, u, v, r, sigmoid):
    """(fp64 score or logit, its bound) for fp32 z, w."""
    z64, w64 = _d(z, w)
    ei = torch.stack([u, v])
    s = O.distmult_fwd(z64, ei, r, w64, sigmoid=False)
    ds = logit_bound(z, w, u, v, r)
    if not sigmoid:
        return s, ds
    return torch.sigmoid(s), SECOND_ORDER * _dsigma(s, ds)


# ---------------------------------------------------------------------------------------------------------------------
# gradients for a given upstream gradient
# ---------------------------------------------------------------------------------------------------------------------
def _scatter_abs(n, R, k, u, v, r, az, aw, at):
    """sum over the contributions of |.|: az [E, k] into rows u, aw [E, k] into rows v, at [E, k] into relation rows."""
    gz = torch.zeros((n, k), dtype=torch.float64)
    gz.index_add_(0, u, az)
    gz.index_add_(0, v, aw)
    gw = torch.zeros((R, k), dtype=torch.float64)
    gw.index_add_(0, r, at)
    return gz, gw


def counts(n, R, u, v, r):
    """contributions per element: (per node row, per relation row) as float64 column vectors."""
    one = torch.ones(u.numel(), dtype=torch.float64)
    cz = torch.zeros(n, dtype=torch.float64).index_add_(0, u, one).index_add_(0, v, one)
    cw = torch.zeros(R, dtype=torch.float64).index_add_(0, r, one)
    return cz.unsqueeze(1), cw.unsqueeze(1)


def _grad_bounds(z64, w64, u, v, r, q, dq, extra_units=0.0):
    n, k, R = z64.shape[0], z64.shape[1], w64.shape[0]
    zu, zv, wr = _rows(z64, w64, u, v, r)
    aq, dq = q.abs().unsqueeze(1), dq.unsqueeze(1)
    tu, tv, tw = (zv * wr).abs(), (zu * wr).abs(), (zu * zv).abs()
    sz, sw = _scatter_abs(n, R, k, u, v, r, aq * tu, aq * tv, aq * tw)
    ez, ew = _scatter_abs(n, R, k, u, v, r, dq * tu, dq * tv, dq * tw)
    cz, cw = counts(n, R, u, v, r)
    bz = gamma(cz + 3) * sz + ez + cz * extra_units
    bw = gamma(cw + 3) * sw + ew
    return SECOND_ORDER * bz, SECOND_ORDER * bw


def fixed_point_unit(z, w, g):
    """what one contribution can lose to the truncation of the task route's fixed point (module docstring)."""
    z, w, g = _d(z, w, g)
    fin = lambda t: t[torch.isfinite(t)]
    zm = float(fin(z).abs().max()) if fin(z).numel() else 0.0
    wm = float(fin(w).abs().max()) if fin(w).numel() else 0.0
    B = 4.0 * zm * wm * float(fin(g).abs().sum())
    return max(2.0 ** -59 * B * (1 + 2.0 ** -20), 2.0 ** -180)


def bwd_reference(g, z, w, u, v, r, sigmoid, task_route=False):
    """((g_z, g_w) in fp64, (their bounds)) for the upstream gradient g of the scores (or of the logits)."""
    g64, z64, w64 = _d(g, z, w)
    ei = torch.stack([u, v])
    want = O.distmult_bwd(g64, z64, ei, r, w64, sigmoid=sigmoid)
    q, dq = g64, torch.zeros_like(g64)
    if sigmoid:
        s = O.distmult_fwd(z64, ei, r, w64, sigmoid=False)
        sg = torch.sigmoid(s)
        dsg = _dsigma(s, logit_bound(z, w, u, v, r))
        q = g64 * sg * (1 - sg)
        dq = g64.abs() * ((1 - 2 * sg).abs() * dsg + dsg * dsg + 3 * U * sg * (1 - sg))
    q = torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0)          # (bounds of non-finite elements are not used)
    dq = torch.nan_to_num(dq, nan=0.0, posinf=0.0, neginf=0.0)
    zb, wb = torch.nan_to_num(z64, nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(w64, nan=0.0, posinf=0.0, neginf=0.0)
    bounds = _grad_bounds(zb, wb, u, v, r, q, dq, fixed_point_unit(z, w, g) if task_route else 0.0)
    return want, bounds


# ---------------------------------------------------------------------------------------------------------------------
# the objective on the generic kernel
# ---------------------------------------------------------------------------------------------------------------------
def _h(t):
    return t * (1 - t) / (t + EPS)


T_PEAK = -EPS + math.sqrt(EPS * EPS + EPS)


def _interval(t, dt):
    lo, hi = (t - dt).clamp(0.0, 1.0), (t + dt).clamp(0.0, 1.0)
    return lo, hi


def _dlog(t, dt):
    lo, hi = _interval(t, dt)
    base = torch.log(t + EPS)
    move = torch.maximum((torch.log(lo + EPS) - base).abs(), (torch.log(hi + EPS) - base).abs())
    return move + 2 * U * base.abs() + 2 * U


def _dh(t, dt):
    lo, hi = _interval(t, dt)
    base = _h(t)
    peak_in = (lo <= T_PEAK) & (T_PEAK <= hi)
    h_peak = _h(torch.tensor(T_PEAK, dtype=torch.float64))
    move = torch.maximum((_h(lo) - base).abs(), (_h(hi) - base).abs())
    move = torch.where(peak_in, torch.maximum(move, (h_peak - base).abs()), move)
    top = torch.maximum(torch.maximum(_h(lo), _h(hi)), torch.where(peak_in, h_peak, base))
    return move + 6 * U * top


def loss_launch(n):
    """(positions per workgroup, workgroups) of the generic kernel for n triples: 256 threads, at least 4 096 positions per
    workgroup, at most ~1 024 workgroups (tipk_distmult.hip, launch_grad).  The loss bound counts the adds of this shape."""
    per_block = max(-(-n // 1024), 4096)
    per_block = -(-per_block // 256) * 256
    return per_block, -(-n // per_block)


def loss_reference(z, w, pu, pv, nu, nv, r):
    """(loss, g_z, g_w) in fp64 and their bounds (d loss, d g_z, d g_w) for the generic objective kernel."""
    z64, w64 = _d(z, w)
    n = pu.numel()
    pos, neg = torch.stack([pu, pv]), torch.stack([nu, nv])
    lp, ln = (O.distmult_fwd(z64, e, r, w64, sigmoid=False) for e in (pos, neg))
    ps, ns = torch.sigmoid(lp), torch.sigmoid(ln)
    loss = O.tip_loss(ps, ns)
    gp, gn = O.tip_loss_bwd(ps, ns)
    gz1, gw1 = O.distmult_bwd(gp, z64, pos, r, w64)
    gz2, gw2 = O.distmult_bwd(gn, z64, neg, r, w64)
    # bounds
    dps = _dsigma(lp, logit_bound(z, w, pu, pv, r))
    dns = _dsigma(ln, logit_bound(z, w, nu, nv, r))
    tp, tn = ps, 1 - ns
    dtp, dtn = dps + U * tp, dns + U * tn
    terms = torch.cat([torch.log(tp + EPS), torch.log(tn + EPS)]).abs()
    per_block, blocks = loss_launch(n)
    m = per_block // 256 + blocks + 12
    dloss = SECOND_ORDER * (float(gamma(m)) * float(terms.sum()) + float(_dlog(tp, dtp).sum() + _dlog(tn, dtn).sum())) / n
    cp, cn = -_h(tp) / n, _h(tn) / n
    dcp, dcn = _dh(tp, dtp) / n + 2 * U * cp.abs(), _dh(tn, dtn) / n + 2 * U * cn.abs()
    u2, v2, r2 = torch.cat([pu, nu]), torch.cat([pv, nv]), torch.cat([r, r])
    bz, bw = _grad_bounds(z64, w64, u2, v2, r2, torch.cat([cp, cn]), torch.cat([dcp, dcn]))
    return (loss, gz1 + gz2, gw1 + gw2), (dloss, bz, bw)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation (plain torch float32 on the CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _logit32(z, w, u, v, r):
    zu, zv, wr = _rows(z, w, u, v, r)
    s = torch.zeros(u.numel(), dtype=torch.float32)
    for j in range(z.shape[1]):
        s = s + (zu[:, j] * zv[:, j]) * wr[:, j]
    return s


def _sigmoid32(s):
    return 1.0 / (1.0 + torch.exp(-s))


def emulate_fwd(z, w, u, v, r, sigmoid):
    z, w = z.float().cpu(), w.float().cpu()
    s = _logit32(z, w, u, v, r)
    return _sigmoid32(s) if sigmoid else s


def _scatter32(z, w, u, v, r, q, order):
    u, v, r, q = u[order], v[order], r[order], q[order].unsqueeze(1)
    zu, zv, wr = _rows(z, w, u, v, r)
    gz = torch.zeros_like(z)
    gz.index_add_(0, u, q * zv * wr)
    gz.index_add_(0, v, q * zu * wr)
    gw = torch.zeros_like(w)
    gw.index_add_(0, r, q * (zu * zv))
    return gz, gw


def emulate_bwd(g, z, w, u, v, r, sigmoid, seed):
    g, z, w = g.float().cpu(), z.float().cpu(), w.float().cpu()
    q = g
    if sigmoid:
        s = _sigmoid32(_logit32(z, w, u, v, r))
        q = g * (s * (1.0 - s))
    order = torch.randperm(u.numel(), generator=torch.Generator().manual_seed(seed))
    return _scatter32(z, w, u, v, r, q, order)


def emulate_loss(z, w, pu, pv, nu, nv, r, seed):
    z, w = z.float().cpu(), w.float().cpu()
    n = pu.numel()
    eps, inv_n = torch.tensor(EPS, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) / float(n)
    sp, sn = _sigmoid32(_logit32(z, w, pu, pv, r)), _sigmoid32(_logit32(z, w, nu, nv, r))
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    terms = (torch.log(sp + eps) + torch.log(1.0 - sn + eps))[order]
    per_block, blocks = loss_launch(n)
    loss = torch.zeros((), dtype=torch.float32)
    for b in range(blocks):                                  # the kernel's tree: lane, wave (butterfly), four waves, atomic
        x = terms[b * per_block:(b + 1) * per_block]
        x = torch.cat([x, torch.zeros(-x.numel() % 256, dtype=torch.float32)]).view(-1, 256)
        lane = torch.zeros(256, dtype=torch.float32)
        for i in range(x.shape[0]):
            lane = lane - x[i]
        wave = lane.view(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            wave = wave[:, :o] + wave[:, o:2 * o]
        loss = loss + (((wave[0, 0] + wave[1, 0]) + wave[2, 0]) + wave[3, 0]) * inv_n
    cp = -inv_n * sp * (1.0 - sp) / (sp + eps)
    cn = inv_n * sn * (1.0 - sn) / (1.0 - sn + eps)
    order2 = torch.cat([order, order + n])[torch.randperm(2 * n, generator=torch.Generator().manual_seed(seed + 1))]
    gz, gw = _scatter32(z, w, torch.cat([pu, nu]), torch.cat([pv, nv]), torch.cat([r, r]), torch.cat([cp, cn]), order2)
    return loss.reshape(1), gz, gw


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def check(got, want, bound, case, quantity, same_kind=False, finite_inside=True, out=print):
    """Hold `got` (fp32) to `want` (fp64) within `bound`, every element -> the largest share of the bound used.
    Where want is not finite got must not be finite (same_kind: NaN where it is NaN, the same infinity).  finite_inside = False:
    the elements want keeps finite are not held (a route that may poison more).  One `DMERR` line per call."""
    got = torch.as_tensor(got).detach().to('cpu', torch.float64).reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(want)
    assert got.shape == want.shape, (case, quantity, 'shape', tuple(got.shape), tuple(want.shape))
    fin = torch.isfinite(want)
    leaked = ~fin & torch.isfinite(got)
    assert not bool(leaked.any()), (case, quantity, '%d elements finite where fp64 is not, first %s'
                                    % (int(leaked.sum()), torch.nonzero(leaked)[:8].flatten().tolist()))
    if same_kind:
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (case, quantity, 'NaN at other elements than fp64')
        assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]), (case, quantity, 'another infinity')
    if not finite_inside or not bool(fin.any()):
        out('DMERR %s %s err=- bound=- share=-' % (case, quantity))
        return 0.0
    err, b = (got[fin] - want[fin]).abs(), bound[fin]
    assert bool(torch.isfinite(b).all()), (case, quantity, 'non-finite bound beside a finite value')
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    bad = err > b
    share = err / b.clamp(min=1e-300)
    share = torch.where((b == 0) & (err == 0), torch.zeros_like(share), share)
    i = int(torch.argmax(share))
    out('DMERR %s %s err=%.3e bound=%.3e share=%.3f' % (case, quantity, float(err[i]), float(b[i]), float(share[i])))
    assert not bool(bad.any()), (case, quantity, '%d of %d elements outside the bound, worst %.3g x the bound (first at %s)'
                                 % (int(bad.sum()), int(fin.sum()), float(share.max()),
                                    torch.nonzero(fin).flatten()[torch.nonzero(bad).flatten()][:8].tolist()))
    return float(share[i])


def check_exact(got, want, case, quantity, out=print):
    """bit for bit: got (fp32) == want (fp64, an exact fp32 number by `exact_ok`)."""
    got = torch.as_tensor(got).detach().to('cpu', torch.float64).reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    diff = got != want
    out('DMERR %s %s err=%.3e bound=0 share=%s' % (case, quantity, float((got - want).abs().max()) if got.numel() else 0.0,
                                                    'inf' if bool(diff.any()) else '0'))
    assert not bool(diff.any()), (case, quantity, 'not bit-equal to fp64: %d elements, max |diff| %g, first at %s'
                                  % (int(diff.sum()), float((got - want).abs().max()), torch.nonzero(diff)[:8].flatten().tolist()))


def exact_ok(g, z, w, u, v, r, prefill=None, unit=None):
    """The exact variant's premise: z, w in {-1, 0, 1}, g (and the prefill) multiples of `unit` (a power of two), and every
    element's sum of |contributions| (+ |prefill|) below 2^24 units -- then every partial sum, in any order, is a multiple of
    the unit below 2^24 units: an exact fp32 number.  The task route's fixed point holds them exactly too: its scale is the power
    of two 2^(59 - ilogb(B)), B = 4 sum |g| <= 2^55 units here, so a unit is at least 2^4 of its integers, the sum of a
    workgroup stays below 2^60 and converts back to the same fp32 number."""
    g, z, w = _d(g, z, w)
    assert bool(((z == 0) | (z.abs() == 1)).all()) and bool(((w == 0) | (w.abs() == 1)).all())
    unit = float(g[g != 0].abs().min()) if unit is None else unit
    assert math.log2(unit) == int(math.log2(unit))
    assert bool((g / unit == torch.round(g / unit)).all())
    zu, zv, wr = _rows(z, w, u, v, r)
    a = g.abs().unsqueeze(1)
    sz, sw = _scatter_abs(z.shape[0], w.shape[0], z.shape[1], u, v, r, a * (zv * wr).abs(), a * (zu * wr).abs(), a * (zu * zv).abs())
    if prefill is not None:
        pz, pw = _d(*prefill)
        assert bool((pz / unit == torch.round(pz / unit)).all()) and bool((pw / unit == torch.round(pw / unit)).all())
        sz, sw = sz + pz.abs(), sw + pw.abs()
    top = max(float(sz.max()), float(sw.max())) / unit
    assert top < 2.0 ** 24, top
    assert 4.0 * float(g.abs().sum()) / unit < 2.0 ** 55                   # the fixed point: unit * 2^ex >= 1
    return top
