"""fp64 specification of the new-drug fit (include/tipk.h section 4q) and the acceptance rules its results are held to.

The spec works from the DEFINITION, not from the device's decomposition: `lists` is the raw input, a list of M lists of
(partner v, side effect r).  For new drug a with row x, prior centre c_a and s(v, r) = sum_k x[k] z[v,k] rel_w[r,k]:

    L_a(x) = 1/P_a sum_{listed} softplus(-s) + rho/N_a sum_{(v, r) in [0, n) x [0, R), not recorded} softplus(s) + l2/2 |x - c_a|^2

P_a counts duplicates; N_a = n R minus the DISTINCT recorded cells.  P_a == 0 or N_a == 0 drops that sum.  `spec_stats` walks
ALL n R cells with per-cell coefficients cpos = multiplicity / P_a and cneg = rho / N_a (0 where recorded).

`check_stats` holds every finite fp32 output X32 (loss, each gradient and Hessian entry) to the project's rule

    |X32 - X64| <= T + (D + C_DFIT) * U * A

  A  the sum of |term| over everything the device adds: the terms of the definition, plus TWICE rho / N_a |term| for every
     recorded cell (section 4q streams the negative term over ALL cells and takes the recorded ones out again: each such term
     is added once and subtracted once), plus the l2 term with |x - c|.
  T  the logit-sensitivity sum: every term weighted with tau = (dim + 2) U sum_k |x_k z_vk w_rk| (the form and U of
     tests/partner_rank_spec.py) times the slope bound of the term in s: 1 for softplus, |f_i| / 4 for the gradient,
     0.1 |f_i f_j| for the Hessian.
  D  tipk_distmult_drug_fit_max_chain: the most fp32 additions a term passes through.
  C_DFIT covers expf, log1pf, the division, the products of a term and the rounding of x - c.  The project's rule: at most
     30 x the largest excess (|X32 - X64| - T) / (U A) - D measured on the device, and not below 4.  With TIPK_ERRLOG set every
     check prints and logs the excess it saw.  Measured on an MI355X (profiles/drug_fit.md): the largest excess was -1008.6 (the
     error beyond T stayed below 58 U A where D was 1068), so C_DFIT is the floor of the rule.
NaN must sit exactly where the contract says: every drug streams every cell, so a drug with a NaN logit on ANY cell has
all-NaN statistics, and no other drug has any.  Wherever the fp64 value and its bound are finite and below 2^126, the device's
value must be finite too.

`spec_fit` is the step rule of section 4m in fp64; `check_fit` holds a fitted row x to
  (a) status 1  =>  |g64(x)_i| <= gtol + bound_g(x)_i for every i;
  (b) L64(x) <= L64(start) + bound_loss: the device only ever accepts a row whose fp32 loss is at most (1 + 16 U) x the fp32
      loss before, so bound_loss = bound_L(x) + bound_L(start) + 17 U accepted (L64(start) + bound_L(start));
  (c) convexity, exact: L64(x) - L64(x*) <= |g64(x)|_inf |x - x*|_1 with x* from `spec_fit` run to max |g| <= 1e-10
      (tolerance: fp64 rounding only);
  (d) info is consistent: evaluations = accepted + rejected + 1 <= max_iter + 1.
"""
import torch

import fit_spec
from fit_spec import bound_of, newton_direction
from partner_rank_spec import U

C_DFIT = 4.0        # observed on MI355X: excess < 0 (profiles/drug_fit.md); "at most 30 x that and not below 4"


def _softplus(s):
    return torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs()))


def cell_tables(lists, n, n_rel, dev='cpu'):
    """(iv, ir, count [M, n R], P [M], N [M]) over the n R cells, cell v * R + r."""
    cells = n * n_rel
    idx = torch.arange(cells, device=dev)
    flat = [a * cells + v * n_rel + r for a, lst in enumerate(lists) for v, r in lst]
    count = torch.bincount(torch.tensor(flat, dtype=torch.int64), minlength=len(lists) * cells).double()
    count = count.reshape(len(lists), cells).to(dev)
    return idx // n_rel, idx % n_rel, count, count.sum(1), float(cells) - (count > 0).sum(1).double()


def spec_stats(z, rel_w, x, lists, prior=None, l2=1e-4, rho=1.0, bounds=True):
    """dict of fp64 tables on z's device: loss [M], g [M, dim], H [M, dim, dim]; with bounds also A_loss, A_g, A_H and T_loss,
    T_g, T_H of the same shapes."""
    dev = z.device
    z64, w64, x64 = z.double(), rel_w.double().to(dev), x.double().to(dev)
    n, dim = z64.shape
    n_rel = w64.shape[0]
    c64 = torch.zeros_like(x64) if prior is None else prior.double().to(dev)
    iv, ir, count, p, big_n = cell_tables(lists, n, n_rel, dev)
    f = z64[iv] * w64[ir]                                                # the feature of every cell
    fa = f.abs()
    out = {k: [] for k in ('loss', 'g', 'H', 'A_loss', 'A_g', 'A_H', 'T_loss', 'T_g', 'T_H')}
    eye = torch.eye(dim, dtype=torch.float64, device=dev)
    ones = torch.ones(n * n_rel, dtype=torch.float64, device=dev)
    for a in range(len(lists)):
        xa, d = x64[a], x64[a] - c64[a]
        cpos = count[a] / p[a] if p[a] > 0 else torch.zeros_like(ones)
        rec = count[a] > 0
        call = rho * ones / big_n[a] if big_n[a] > 0 else torch.zeros_like(ones)
        cneg = torch.where(rec, torch.zeros_like(ones), call)
        s = f @ xa
        sp, sn = _softplus(s), _softplus(-s)
        sg, sgn = torch.sigmoid(s), torch.sigmoid(-s)
        h = sg * sgn

        def tsum(c, t):                                                  # sum_p c_p t_p with 0 * inf = 0 for an absent term
            return torch.where(c != 0, c * t, torch.zeros_like(t)).sum()

        loss = tsum(cpos, sn) + tsum(cneg, sp) + 0.5 * l2 * (d * d).sum()
        cg = torch.where(cpos != 0, -cpos * sgn, torch.zeros_like(s)) + torch.where(cneg != 0, cneg * sg, torch.zeros_like(s))
        g = cg @ f + l2 * d
        hess = (f * ((cpos + cneg) * h)[:, None]).t() @ f + l2 * eye
        if bool(torch.isnan(s).any()):                                   # every drug streams every cell
            loss, g, hess = loss * float('nan'), g * float('nan'), hess * float('nan')
        out['loss'].append(loss); out['g'].append(g); out['H'].append(hess)
        if not bounds:
            continue
        extra = torch.where(rec, 2.0 * call, torch.zeros_like(ones))     # streamed and taken out again
        wt = cpos + cneg + extra
        tau = (dim + 2) * U * (fa @ xa.abs())
        out['A_loss'].append(tsum(cpos, sn) + tsum(cneg + extra, sp) + 0.5 * l2 * (d * d).sum())
        out['A_g'].append((cpos * sgn + (cneg + extra) * sg) @ fa + l2 * d.abs())
        out['A_H'].append((fa * (wt * h)[:, None]).t() @ fa + l2 * eye)
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


def check_stats(z, rel_w, x, lists, prior, l2, rho, got, d_chain, c_fit=C_DFIT, what='', spec=None):
    """Assert the acceptance rule for got = (loss [M], grad [M, dim], hess [M, dim, dim]) fp32 -> the spec's tables with
    'observed_c', the largest excess this result needs (-inf when nothing is finite and positive).  The rule is the one of
    tests/fit_spec.py, word for word, applied to this spec's tables (a row is a drug here)."""
    t = spec_stats(z, rel_w, x, lists, prior, l2, rho) if spec is None else spec
    return fit_spec.check_stats(None, None, None, l2, rho, got, d_chain, c_fit, 'drug fit ' + what, spec=t)


def spec_fit(z, rel_w, lists, prior=None, l2=1e-4, rho=1.0, init=None, max_iter=16, gtol=1e-5, slack=16 * U):
    """The step rule of section 4m in fp64, one drug at a time; the start is init, else the prior, else zeros -> dict(x [M, dim],
    loss [M], g [M, dim], info int64 [M, 4] = (status, evaluations, accepted, rejected))."""
    dev, dim = z.device, z.shape[1]
    xs, ls, gs, infos = [], [], [], []
    for a, lst in enumerate(lists):
        c = None if prior is None else prior[a:a + 1]
        start = init if init is not None else prior
        x = torch.zeros(dim, dtype=torch.float64, device=dev) if start is None else start[a].double().to(dev).clone()
        trial, loss, g, p, t = x.clone(), None, None, None, 1.0
        status = evals = acc = rej = 0
        for _ in range(max_iter + 1):
            st = spec_stats(z, rel_w, trial[None], [lst], c, l2, rho, bounds=False)
            lt, gt, ht = st['loss'][0], st['g'][0], st['H'][0]
            finite = bool(torch.isfinite(lt)) and bool(torch.isfinite(gt).all()) and bool(torch.isfinite(ht).all())
            first = evals == 0
            evals += 1
            if not finite and not first:
                status, rej = 3, rej + 1                                 # a trial that cannot be judged is not accepted
            else:
                if first or bool(lt <= loss + 1e-4 * t * (g @ p) + slack * loss.abs()):
                    x, loss, g, t = trial.clone(), lt, gt, 1.0
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
            trial = x + t * p
        xs.append(x); ls.append(loss); gs.append(g); infos.append([status, evals, acc, rej])
    if not xs:
        return {'x': torch.zeros((0, dim), dtype=torch.float64, device=dev), 'loss': torch.zeros(0, dtype=torch.float64),
                'g': torch.zeros((0, dim), dtype=torch.float64), 'info': torch.zeros((0, 4), dtype=torch.int64)}
    return {'x': torch.stack(xs), 'loss': torch.stack(ls), 'g': torch.stack(gs), 'info': torch.tensor(infos, dtype=torch.int64)}


def check_fit(z, rel_w, lists, prior, l2, rho, init, max_iter, gtol, got, d_chain, c_fit=C_DFIT, what=''):
    """Assert (a)-(d) for got = (x [M, dim] fp32, info int [M, 4]) -> dict with the fp64 statistics at x and at the start."""
    x, info = got[0].to(z.device), got[1].to('cpu').long()
    m, dim = len(lists), z.shape[1]
    start = init if init is not None else prior
    start = torch.zeros((m, dim), dtype=torch.float32, device=z.device) if start is None else start.to(z.device)
    at_x = spec_stats(z, rel_w, x, lists, prior, l2, rho)
    at_0 = spec_stats(z, rel_w, start, lists, prior, l2, rho)
    best = spec_fit(z, rel_w, lists, prior, l2, rho, init=start, max_iter=60, gtol=1e-10)
    at_best = spec_stats(z, rel_w, best['x'], lists, prior, l2, rho, bounds=False)
    for r in range(m):
        status, evals, acc, rej = (int(v) for v in info[r])
        assert evals == acc + rej + 1 and evals <= max_iter + 1, (what, r, 'info', info[r].tolist())       # (d)
        if status == 1:                                                                                    # (a)
            bg = gtol + bound_of(at_x, 'g', d_chain, c_fit)[r]
            assert bool((at_x['g'][r].abs() <= bg).all()), (what, r, 'gradient at a converged row',
                                                            float(at_x['g'][r].abs().max()), float(bg.min()))
        bl = bound_of(at_x, 'loss', d_chain, c_fit)[r] + bound_of(at_0, 'loss', d_chain, c_fit)[r]
        bl = bl + 17 * U * acc * (at_0['loss'][r] + bound_of(at_0, 'loss', d_chain, c_fit)[r])
        assert float(at_x['loss'][r]) <= float(at_0['loss'][r] + bl), (what, r, 'loss above the start',                # (b)
                                                                       float(at_x['loss'][r]), float(at_0['loss'][r]), float(bl))
        gap = float(at_x['loss'][r] - at_best['loss'][r])                                                  # (c)
        room = float(at_x['g'][r].abs().max() * (x[r].double() - best['x'][r]).abs().sum())
        assert gap <= room + 1e-12 * (1 + abs(float(at_x['loss'][r]))), (what, r, 'convexity', gap, room)
    return {'at_x': at_x, 'at_init': at_0, 'best': best}
