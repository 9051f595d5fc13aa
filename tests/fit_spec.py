"""fp64 specification of the side-effect fit (include/tipk.h section 4m) and the acceptance rules its results are held to.

The spec works from the DEFINITION, not from the device's decomposition: `pairs` is the raw input, a list of B lists of (u, v).
For relation b with row w and s(u, v) = sum_k z[u,k] z[v,k] w[k]:

    L_b(w) = 1/P_b sum_{listed} softplus(-s) + rho/N_b sum_{ordered (u, v) in [0, n)^2, not recorded} softplus(s) + l2/2 |w|^2

P_b counts duplicates; recorded = the pair or its mirror is listed; N_b = the ordered pairs that are not recorded (self pairs
are negatives unless listed).  P_b == 0 or N_b == 0 drops that sum.  `spec_stats` evaluates it over the unordered pairs u <= v
with per-pair coefficients cpos = multiplicity / P_b and cneg = rho m / N_b (m = 2, or 1 for u == v; 0 where recorded).

`check_stats` holds every finite fp32 output X32 (loss, each gradient and Hessian entry) to

    |X32 - X64| <= T + (D + C_FIT) * U * A

  A  the sum of |term| over everything the device adds: the terms of the definition, plus TWICE rho m / N_b |term| for every
     recorded pair (section 4m streams the negative term over ALL pairs and takes the recorded ones out again: each such term
     is added once and subtracted once), plus the l2 term.
  T  the logit-sensitivity sum: every term weighted with tau_p = (dim + 2) U sum_k |z_u z_v w| (the form and U of
     tests/partner_rank_spec.py) times the slope bound of the term in s: 1 for softplus, |f_i| / 4 for the gradient,
     0.1 |f_i f_j| for the Hessian (|d/ds sigma (1 - sigma)| <= 1 / (6 sqrt 3) < 0.1).
  D  tipk_distmult_fit_max_chain: the most fp32 additions a term passes through.
  C_FIT covers expf, log1pf, the division and the products of a term.  The project's rule: at most 30 x the largest excess
     (|X32 - X64| - T) / (U A) - D measured on the device, and not below 4.  With TIPK_ERRLOG set every check prints and logs
     the excess it saw.  Measured on an MI355X (profiles/side_effect_fit.md): the largest excess was -984 (the error stayed
     below 52 U A where D was 1036), so C_FIT is the floor of the rule.
NaN must sit exactly where the contract says: a relation with a NaN logit has all-NaN statistics, no other relation has any.
Wherever the fp64 value and its bound are finite and below 2^126, the device's value must be finite too (an overflow or a
division by zero on the device does not slip through as "not a finite output").

`spec_fit` is the step rule of section 4m in fp64; `check_fit` holds a fitted row w to
  (a) status 1  =>  |g64(w)_i| <= gtol + bound_g(w)_i for every i;
  (b) L64(w) <= L64(init) + bound_loss: the device only ever accepts a row whose fp32 loss is at most (1 + 16 U) x the fp32
      loss before, so bound_loss = bound_L(w) + bound_L(init) + 17 U accepted (L64(init) + bound_L(init));
  (c) convexity, exact: L64(w) - L64(w*) <= |g64(w)|_inf |w - w*|_1 with w* from `spec_fit` run to max |g| <= 1e-10
      (tolerance: fp64 rounding only);
  (d) info is consistent: evaluations = accepted + rejected + 1 <= max_iter + 1.
"""
import json
import os

import torch

from partner_rank_spec import U

C_FIT = 4.0         # observed on MI355X: excess < 0 (profiles/side_effect_fit.md); "at most 30 x that and not below 4"


def _softplus(s):
    return torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs()))


def pair_tables(pairs, n, dev='cpu'):
    """(iu, iv, m, count [B, M], P [B], N [B]) over the M = n (n + 1) / 2 unordered pairs u <= v."""
    iu, iv = torch.triu_indices(n, n, device=dev)
    m = torch.where(iu == iv, 1.0, 2.0).double()
    rows = n * (n + 1) // 2
    flat = []
    for b, lst in enumerate(pairs):
        for u, v in lst:
            lo, hi = (u, v) if u <= v else (v, u)
            flat.append(b * rows + lo * n - lo * (lo - 1) // 2 + hi - lo)
    count = torch.bincount(torch.tensor(flat, dtype=torch.int64), minlength=len(pairs) * rows).double()
    count = count.reshape(len(pairs), rows).to(dev)
    p = count.sum(1)
    big_n = float(n) * n - ((count > 0) * m).sum(1)
    return iu, iv, m, count, p, big_n


def spec_stats(z, w, pairs, l2=1e-4, rho=1.0, bounds=True):
    """dict of fp64 tables on z's device: loss [B], g [B, dim], H [B, dim, dim]; with bounds also A_loss, A_g, A_H and T_loss,
    T_g, T_H of the same shapes."""
    dev = z.device
    z64, w64 = z.double(), w.double()
    n, dim = z64.shape
    iu, iv, m, count, p, big_n = pair_tables(pairs, n, dev)
    f = z64[iu] * z64[iv]
    fa = f.abs()
    out = {k: [] for k in ('loss', 'g', 'H', 'A_loss', 'A_g', 'A_H', 'T_loss', 'T_g', 'T_H')}
    eye = torch.eye(dim, dtype=torch.float64, device=dev)
    for b in range(len(pairs)):
        wb = w64[b]
        cpos = count[b] / p[b] if p[b] > 0 else torch.zeros_like(m)
        rec = count[b] > 0
        call = rho * m / big_n[b] if big_n[b] > 0 else torch.zeros_like(m)
        cneg = torch.where(rec, torch.zeros_like(m), call)
        s = f @ wb
        sp, sn = _softplus(s), _softplus(-s)
        sg, sgn = torch.sigmoid(s), torch.sigmoid(-s)
        h = sg * sgn
        h = torch.where(torch.isnan(s), s, h)
        ww = (wb * wb).sum()

        def tsum(c, x):                                                  # sum_p c_p x_p with 0 * inf = 0 for an absent term
            return torch.where(c != 0, c * x, torch.zeros_like(x)).sum()

        out['loss'].append(tsum(cpos, sn) + tsum(cneg, sp) + 0.5 * l2 * ww)
        cg = torch.where(cpos != 0, -cpos * sgn, torch.zeros_like(s)) + torch.where(cneg != 0, cneg * sg, torch.zeros_like(s))
        out['g'].append(cg @ f + l2 * wb)
        chh = (cpos + cneg) * h
        out['H'].append((f * chh[:, None]).t() @ f + l2 * eye)
        if not bounds:
            continue
        extra = torch.where(rec, 2.0 * call, torch.zeros_like(m))       # streamed and taken out again
        wt = cpos + cneg + extra
        tau = (dim + 2) * U * (fa @ wb.abs())
        out['A_loss'].append(tsum(cpos, sn) + tsum(cneg + extra, sp) + 0.5 * l2 * ww)
        ag = cpos * sgn + (cneg + extra) * sg
        out['A_g'].append(ag @ fa + l2 * wb.abs())
        ah = wt * h
        out['A_H'].append((fa * ah[:, None]).t() @ fa + l2 * eye)
        out['T_loss'].append((wt * tau).sum())
        out['T_g'].append((wt * tau) @ fa / 4)
        out['T_H'].append(0.1 * (fa * (wt * tau)[:, None]).t() @ fa)
    shapes = {'loss': (0,), 'g': (0, dim), 'H': (0, dim, dim)}
    res = {}
    for k, v in out.items():
        if v:
            res[k] = torch.stack(v)
        elif bounds or k in shapes:
            res[k] = torch.zeros(shapes[k.split('_')[-1] if '_' in k else k], dtype=torch.float64, device=dev)
    return res


def bound_of(t, name, d_chain, c_fit=C_FIT):
    return t['T_' + name] + (d_chain + c_fit) * U * t['A_' + name]


def check_stats(z, w, pairs, l2, rho, got, d_chain, c_fit=C_FIT, what='', spec=None):
    """Assert the acceptance rule for got = (loss [B], grad [B, dim], hess [B, dim, dim]) fp32 -> the spec's tables with
    'observed_c', the largest excess this result needs (-inf when nothing is finite and positive)."""
    t = spec_stats(z, w, pairs, l2, rho) if spec is None else spec
    worst = float('-inf')
    nan_rel = torch.isnan(t['loss'])
    for name, x in zip(('loss', 'g', 'H'), got):
        x64 = t[name]
        x = x.to(x64.device)
        assert x.dtype == torch.float32 and x.shape == x64.shape, (name, x.dtype, tuple(x.shape), tuple(x64.shape))
        rel_nan = nan_rel.reshape((-1,) + (1,) * (x64.dim() - 1)).expand_as(x64)
        assert bool(torch.isnan(x)[rel_nan].all()), (what, name, 'a relation with a NaN logit must be all NaN')
        assert not bool(torch.isnan(x)[~rel_nan & torch.isfinite(x64)].any()), (what, name, 'NaN in a relation without a NaN logit')
        bound = bound_of(t, name, d_chain, c_fit)
        # a finite fp64 value with a finite bound, well inside the fp32 range, must come out finite: no overflow, no 0 / 0
        inside = torch.isfinite(x64) & torch.isfinite(bound) & (x64.abs() + bound < 2.0 ** 126)
        assert bool(torch.isfinite(x)[inside].all()), (what, name, 'non-finite where fp64 and its bound are finite',
                                                       int((inside & ~torch.isfinite(x)).sum()))
        ok = torch.isfinite(x64) & torch.isfinite(x) & torch.isfinite(t['A_' + name])
        off = (x.double() - x64).abs()
        a = t['A_' + name]
        pos = ok & (a > 0)
        if bool(pos.any()):
            worst = max(worst, float((((off - t['T_' + name]) / (U * a)) - d_chain)[pos].max()))
        good = (x.double() == x64) | (off <= bound)
        assert bool(good[ok].all()), (what, name, 'off fp64', float((off - bound)[ok & ~good].max()), int((ok & ~good).sum()),
                                      'excess over D', float((((off - t['T_' + name]) / (U * a)) - d_chain)[ok & ~good].max()))
    t['observed_c'] = worst
    if os.environ.get('TIPK_ERRLOG') and worst > float('-inf'):
        line = {'what': 'fit stats c', 'case': what, 'observed_c': worst, 'd_chain': int(d_chain), 'c_fit': c_fit}
        print('ERR %s' % json.dumps(line))
        with open(os.environ['TIPK_ERRLOG'], 'a') as f:
            f.write(json.dumps(line) + '\n')
    return t


def newton_direction(g, h):
    """-H^-1 g by Cholesky; a pivot that is not > 0: -g / max_i H_ii (-g when that is not > 0) -> (p, used_fallback)."""
    chol, bad = torch.linalg.cholesky_ex(h)
    if int(bad) == 0 and bool(torch.isfinite(chol).all()):
        return -torch.cholesky_solve(g[:, None], chol)[:, 0], False
    hmax = h.diagonal().max()
    return (-g / hmax if hmax > 0 else -g), True


def spec_fit(z, pairs, l2=1e-4, rho=1.0, init=None, max_iter=16, gtol=1e-5, slack=16 * U):
    """The step rule of section 4m in fp64, one relation at a time -> dict(w [B, dim], loss [B], g [B, dim], info int64
    [B, 4] = (status, evaluations, accepted, rejected))."""
    dev, dim = z.device, z.shape[1]
    ws, ls, gs, infos = [], [], [], []
    for b, lst in enumerate(pairs):
        w = torch.zeros(dim, dtype=torch.float64, device=dev) if init is None else init[b].double().to(dev).clone()
        trial, loss, g, p, t = w.clone(), None, None, None, 1.0
        status = evals = acc = rej = 0
        for _ in range(max_iter + 1):
            st = spec_stats(z, trial[None], [lst], l2, rho, bounds=False)
            lt, gt, ht = st['loss'][0], st['g'][0], st['H'][0]
            finite = bool(torch.isfinite(lt)) and bool(torch.isfinite(gt).all()) and bool(torch.isfinite(ht).all())
            first = evals == 0
            evals += 1
            if not finite and not first:
                status, rej = 3, rej + 1                                 # a trial that cannot be judged is not accepted
            else:
                if first or bool(lt <= loss + 1e-4 * t * (g @ p) + slack * loss.abs()):
                    w, loss, g, t = trial.clone(), lt, gt, 1.0
                    acc += 0 if first else 1
                    if not finite:
                        status, p = 3, torch.zeros_like(g)
                    else:
                        p = newton_direction(g, ht)[0]
                else:
                    rej += 1
                    t = t / 2
            if status == 0:
                if float(g.abs().max()) <= gtol:
                    status = 1
                elif t < 2.0 ** -20:
                    status = 2
            if status != 0:
                break
            trial = w + t * p
        ws.append(w); ls.append(loss); gs.append(g); infos.append([status, evals, acc, rej])
    if not ws:
        return {'w': torch.zeros((0, dim), dtype=torch.float64, device=dev), 'loss': torch.zeros(0, dtype=torch.float64),
                'g': torch.zeros((0, dim), dtype=torch.float64), 'info': torch.zeros((0, 4), dtype=torch.int64)}
    return {'w': torch.stack(ws), 'loss': torch.stack(ls), 'g': torch.stack(gs), 'info': torch.tensor(infos, dtype=torch.int64)}


def check_fit(z, pairs, l2, rho, init, max_iter, gtol, got, d_chain, c_fit=C_FIT, what=''):
    """Assert (a)-(d) for got = (w [B, dim] fp32, info int [B, 4]) -> dict with the fp64 statistics at w and at init."""
    w, info = got[0].to(z.device), got[1].to('cpu').long()
    b, dim = len(pairs), z.shape[1]
    start = torch.zeros((b, dim), dtype=torch.float32, device=z.device) if init is None else init.to(z.device)
    at_w = spec_stats(z, w, pairs, l2, rho)
    at_0 = spec_stats(z, start, pairs, l2, rho)
    best = spec_fit(z, pairs, l2, rho, init=start, max_iter=60, gtol=1e-10)
    at_best = spec_stats(z, best['w'], pairs, l2, rho, bounds=False)
    for r in range(b):
        status, evals, acc, rej = (int(x) for x in info[r])
        assert evals == acc + rej + 1 and evals <= max_iter + 1, (what, r, 'info', info[r].tolist())       # (d)
        if status == 1:                                                                                    # (a)
            bg = gtol + bound_of(at_w, 'g', d_chain, c_fit)[r]
            assert bool((at_w['g'][r].abs() <= bg).all()), (what, r, 'gradient at a converged row',
                                                            float(at_w['g'][r].abs().max()), float(bg.min()))
        bl = bound_of(at_w, 'loss', d_chain, c_fit)[r] + bound_of(at_0, 'loss', d_chain, c_fit)[r]
        bl = bl + 17 * U * acc * (at_0['loss'][r] + bound_of(at_0, 'loss', d_chain, c_fit)[r])
        assert float(at_w['loss'][r]) <= float(at_0['loss'][r] + bl), (what, r, 'loss above the start',                # (b)
                                                                       float(at_w['loss'][r]), float(at_0['loss'][r]), float(bl))
        gap = float(at_w['loss'][r] - at_best['loss'][r])                                                  # (c)
        room = float(at_w['g'][r].abs().max() * (w[r].double() - best['w'][r]).abs().sum())
        assert gap <= room + 1e-12 * (1 + abs(float(at_w['loss'][r]))), (what, r, 'convexity', gap, room)
    return {'at_w': at_w, 'at_init': at_0, 'best': best}
