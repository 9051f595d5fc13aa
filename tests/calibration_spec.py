"""fp64 specification of the per-relation Platt calibration (include/tipk.h section 4r) and the acceptance rules its results are
held to.

The spec works from the DEFINITION -- the three SETS of a query, built by brute force from the raw triples --, not from the
device's decomposition.  For query q on relation r = relations[q], over the cells u < v of [0, n):
    TRAIN  the cells some training triple of r names, in either direction;
    POS    the cells some given triple of r names (u != v) that are not in TRAIN;
    NEG    every other cell;                                              M = |POS| + |NEG|.
With s(u, v) = sum_k z[u,k] w_r[k] z[v,k] and t = a s + b:

    L_q(a, b) = 1/M [ sum_POS softplus(-t) + sum_NEG softplus(t) ] + l2/2 (a - 1)^2          (M == 0 drops the sums)

A NaN logit on ANY cell of a query with M > 0 (a TRAIN cell too: the device streams every cell and takes the listed ones out
again) makes all its statistics NaN; a query with M == 0 has no terms: the l2 term alone, whatever its logits are.

`check_stats` holds every finite fp32 output X32 (loss, the two gradient and the four Hessian entries) to

    |X32 - X64| <= T + (D + C_CAL) * U * A

  A  the sum of |term| over everything the device adds: the terms of the definition, plus TWICE 1/M |term at softplus(t)| for
     every listed cell -- TRAIN and POS cells are streamed as negatives and taken out again --, plus the l2 term.
  T  the logit-sensitivity sum: every term weighted with tau_p = (dim + 2) U sum_k |z_u z_v w| (the form and U of
     tests/partner_rank_spec.py), times |a| (t = a s + b), times the slope bound of the term in t: 1 for softplus,
     |phi_i| / 4 for the gradient, 0.1 |phi_i phi_j| for the Hessian, phi = (s, 1).  (The dependence of phi itself on s is
     not in T: it falls to the (D + C_CAL) U A part, and the measured excess says that it fits.)
  D  tipk_distmult_calibrate_max_chain: the most fp32 additions a term passes through.
  C_CAL covers expf, log1pf, the division, the products of a term and the fp32 dense_w.  The project's rule: at most 30 x the
     largest excess (|X32 - X64| - T) / (U A) - D measured on the device, and not below 4.  With TIPK_ERRLOG set every check
     prints and logs the excess it saw.  Measured on an MI355X (profiles/calibration.md): over the 36 statistics checks of the
     suite the largest excess was -17.3 (the error beyond T stayed below 0.7 U A where D is 18), so C_CAL is the floor of the rule.
NaN must sit exactly where the contract says: a query with a NaN logit has all-NaN statistics, no other query has any.
Wherever the fp64 value and its bound are finite and below 2^126, the device's value must be finite too.

`spec_fit` is the step rule of section 4m in fp64 on the two unknowns; `check_fit` holds a fitted map (a, b) to
  (a) status 1  =>  |g64(a, b)_i| <= gtol + bound_g_i for both i;
  (b) L64(a, b) <= L64(start) + bound_loss, with the 17 U slack per accepted step of tests/fit_spec.py;
  (c) convexity, exact: L64(a, b) - L64(best) <= |g64(a, b)|_inf |(a, b) - best|_1 with best from `spec_fit` run to
      max |g| <= 1e-10 (tolerance: fp64 rounding only);
  (d) info is consistent: evaluations = accepted + rejected + 1 <= max_iter + 1;
  (e) status 1  =>  |sum over POS and NEG of sigma(t) - n_pos| <= M (gtol + bound_g_b): the calibrated model expects as many
      positives as there are.
"""
import json
import os

import torch

from fit_spec import bound_of, newton_direction
from partner_rank_spec import U

C_CAL = 4.0         # observed on MI355X: excess <= -17.3 (profiles/calibration.md); "at most 30 x that and not below 4"


def _softplus(s):
    return torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs()))


def _by_relation(triples, n):
    """{relation: set of (u, v), u < v} of raw triples (edge_index [2, T], edge_type [T]); self pairs are no cells."""
    idx, et = torch.as_tensor(triples[0]).cpu().long(), torch.as_tensor(triples[1]).cpu().long()
    out = {}
    for u, v, r in zip(idx[0].tolist(), idx[1].tolist(), et.tolist()):
        assert 0 <= u < n and 0 <= v < n
        if u != v:
            out.setdefault(r, set()).add((min(u, v), max(u, v)))
    return out


def cell_sets(train, given, n, relations):
    """(iu, iv [C], trn bool [Q, C], pos bool [Q, C], dropped int64 [Q]) over the C = n (n - 1) / 2 cells u < v."""
    iu, iv = torch.triu_indices(n, n, 1)
    cells = iu.numel()
    cid = {(u, v): i for i, (u, v) in enumerate(zip(iu.tolist(), iv.tolist()))}
    tr, gv = _by_relation(train, n), _by_relation(given, n)
    rel = [int(r) for r in torch.as_tensor(relations).reshape(-1).tolist()]
    trn = torch.zeros((len(rel), cells), dtype=torch.bool)
    pos = torch.zeros((len(rel), cells), dtype=torch.bool)
    dropped = torch.zeros(len(rel), dtype=torch.int64)
    for q, r in enumerate(rel):
        t_set, g_set = tr.get(r, set()), gv.get(r, set())
        for c in t_set:
            trn[q, cid[c]] = True
        for c in g_set - t_set:
            pos[q, cid[c]] = True
        dropped[q] = len(g_set & t_set)
    return iu, iv, trn, pos, dropped


def spec_stats(z, w, ab, train, given, relations, l2=1e-6, bounds=True, sets=None):
    """z [n, dim], w [R, dim] (the decoder rows), ab [Q, 2] -> dict of fp64 tables on z's device: loss [Q], g [Q, 2], H
    [Q, 2, 2], expected [Q] (sum of sigma(t) over POS and NEG), n_pos, n_neg, n_dropped int64 [Q]; with bounds also A_loss,
    A_g, A_H and T_loss, T_g, T_H of the same shapes.  sets: the result of `cell_sets`, to share it between calls."""
    dev = z.device
    z64, w64, ab64 = z.double(), w.double(), ab.double().to(dev)
    n, dim = z64.shape
    iu, iv, trn, pos, dropped = cell_sets(train, given, n, relations) if sets is None else sets
    iu, iv, trn, pos = iu.to(dev), iv.to(dev), trn.to(dev), pos.to(dev)
    rel = torch.as_tensor(relations).reshape(-1).long().to(dev)
    q_n = rel.numel()
    neg = ~trn & ~pos
    n_pos, n_neg = pos.sum(1), neg.sum(1)
    big_m = (n_pos + n_neg).double()
    inv_m = torch.where(big_m > 0, 1.0 / big_m.clamp(min=1.0), torch.zeros_like(big_m))[:, None]
    wq = w64[rel]                                                        # [Q, dim]
    zu, zv = z64[iu], z64[iv]                                            # [C, dim]
    s = torch.einsum('ck,qk,ck->qc', zu, wq, zv)                         # [Q, C]
    a, b = ab64[:, :1], ab64[:, 1:]
    t = a * s + b
    sp, sn = _softplus(t), _softplus(-t)
    sg, sgn = torch.sigmoid(t), torch.sigmoid(-t)
    h = torch.where(torch.isnan(t), t, sg * sgn)
    phi = torch.stack([s, torch.ones_like(s)], 2)                        # [Q, C, 2]

    def only(mask, x):                                                   # an absent term is 0, whatever its value
        return torch.where(mask, x, torch.zeros_like(x))

    da = ab64[:, 0] - 1.0
    e_a = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev)
    loss = inv_m[:, 0] * (only(pos, sn).sum(1) + only(neg, sp).sum(1)) + 0.5 * l2 * da * da
    cg = only(neg, sg) - only(pos, sgn)                                  # d term / d t
    g = inv_m * (cg[:, :, None] * only((pos | neg)[:, :, None].expand_as(phi), phi)).sum(1) + l2 * da[:, None] * e_a
    ch = only(pos | neg, h)
    hphi = only((pos | neg)[:, :, None].expand_as(phi), phi)
    hess = inv_m[:, :, None] * torch.einsum('qc,qci,qcj->qij', ch, hphi, hphi) + l2 * torch.outer(e_a, e_a)
    nan_q = (torch.isnan(t).any(1) & (big_m > 0)) if t.shape[1] else torch.zeros(q_n, dtype=torch.bool, device=dev)
    nan = torch.full((), float('nan'), dtype=torch.float64, device=dev)
    res = {'loss': torch.where(nan_q, nan, loss), 'g': torch.where(nan_q[:, None], nan, g),
           'H': torch.where(nan_q[:, None, None], nan, hess),
           'expected': only(pos | neg, sg).sum(1), 'n_pos': n_pos.cpu(), 'n_neg': n_neg.cpu(), 'n_dropped': dropped}
    if not bounds:
        return res
    listed = trn | pos
    w_neg = inv_m * (neg.double() + 2.0 * listed.double())               # weight of |term at softplus(t)|
    w_pos = inv_m * pos.double()
    w_all = w_neg + w_pos
    tau = (dim + 2) * U * torch.einsum('ck,qk,ck->qc', zu.abs(), wq.abs(), zv.abs()) * a.abs()
    pa = phi.abs()
    res['A_loss'] = only(w_pos != 0, w_pos * sn).sum(1) + only(w_neg != 0, w_neg * sp).sum(1) + 0.5 * l2 * da * da
    ag = only(w_pos != 0, w_pos * sgn) + only(w_neg != 0, w_neg * sg)
    res['A_g'] = (ag[:, :, None] * only((w_all != 0)[:, :, None].expand_as(pa), pa)).sum(1) + l2 * da.abs()[:, None] * e_a
    ah = only(w_all != 0, w_all * h)
    pa0 = only((w_all != 0)[:, :, None].expand_as(pa), pa)
    res['A_H'] = torch.einsum('qc,qci,qcj->qij', ah, pa0, pa0) + l2 * torch.outer(e_a, e_a)
    wt = only(w_all != 0, w_all * tau)
    res['T_loss'] = wt.sum(1)
    res['T_g'] = (wt[:, :, None] * pa0).sum(1) / 4
    res['T_H'] = 0.1 * torch.einsum('qc,qci,qcj->qij', wt, pa0, pa0)
    return res


def check_stats(got, spec, d_chain, c_cal=C_CAL, what=''):
    """Assert the acceptance rule for got = (loss [Q], grad [Q, 2], hess [Q, 2, 2]) fp32 against spec = `spec_stats(...)` ->
    the largest excess this result needs (-inf when nothing is finite and positive)."""
    t = spec
    worst = float('-inf')
    nan_q = torch.isnan(t['loss'])
    for name, x in zip(('loss', 'g', 'H'), got):
        x64 = t[name]
        x = x.to(x64.device)
        assert x.dtype == torch.float32 and x.shape == x64.shape, (name, x.dtype, tuple(x.shape), tuple(x64.shape))
        q_nan = nan_q.reshape((-1,) + (1,) * (x64.dim() - 1)).expand_as(x64)
        assert bool(torch.isnan(x)[q_nan].all()), (what, name, 'a query with a NaN logit must be all NaN')
        assert not bool(torch.isnan(x)[~q_nan & torch.isfinite(x64)].any()), (what, name, 'NaN in a query without a NaN logit')
        bound = bound_of(t, name, d_chain, c_cal)
        inside = torch.isfinite(x64) & torch.isfinite(bound) & (x64.abs() + bound < 2.0 ** 126)
        assert bool(torch.isfinite(x)[inside].all()), (what, name, 'non-finite where fp64 and its bound are finite',
                                                       int((inside & ~torch.isfinite(x)).sum()))
        ok = torch.isfinite(x64) & torch.isfinite(x) & torch.isfinite(t['A_' + name])
        off = (x.double() - x64).abs()
        a = t['A_' + name]
        pos = ok & (a > 0)
        excess = ((off - t['T_' + name]) / (U * a)) - d_chain
        if bool(pos.any()):
            worst = max(worst, float(excess[pos].max()))
        good = (x.double() == x64) | (off <= bound)
        print('calibration check %s %s: largest |X32 - X64| %.3e, largest excess over D %s'
              % (what, name, float(off[ok].max()) if bool(ok.any()) else 0.0,
                 '%.2f' % float(excess[pos].max()) if bool(pos.any()) else 'n/a'))
        assert bool(good[ok].all()), (what, name, 'off fp64', float((off - bound)[ok & ~good].max()), int((ok & ~good).sum()),
                                      'excess over D', float(excess[ok & ~good].max()))
    if os.environ.get('TIPK_ERRLOG') and worst > float('-inf'):
        line = {'what': 'calibration stats c', 'case': what, 'observed_c': worst, 'd_chain': int(d_chain), 'c_cal': c_cal}
        print('ERR %s' % json.dumps(line))
        with open(os.environ['TIPK_ERRLOG'], 'a') as f:
            f.write(json.dumps(line) + '\n')
    return worst


def spec_fit(z, w, train, given, relations, l2=1e-6, init=None, max_iter=32, gtol=1e-6, slack=16 * U, sets=None):
    """The step rule of section 4m in fp64 on (a, b), one query at a time -> dict(ab [Q, 2], loss [Q], g [Q, 2], info int64
    [Q, 4] = (status, evaluations, accepted, rejected)).  init: [Q, 2] or None (the identity)."""
    dev = z.device
    n = z.shape[0]
    rel = torch.as_tensor(relations).reshape(-1).long()
    iu, iv, trn, pos, dropped = cell_sets(train, given, n, rel) if sets is None else sets
    abs_, ls, gs, infos = [], [], [], []
    for q in range(rel.numel()):
        one = (iu, iv, trn[q:q + 1], pos[q:q + 1], dropped[q:q + 1])
        x = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev) if init is None else init[q].double().to(dev).clone()
        trial, loss, g, p, t = x.clone(), None, None, None, 1.0
        status = evals = acc = rej = 0
        for _ in range(max_iter + 1):
            st = spec_stats(z, w, trial[None], train, given, rel[q:q + 1], l2, bounds=False, sets=one)
            lt, gt, ht = st['loss'][0], st['g'][0], st['H'][0]
            finite = bool(torch.isfinite(lt)) and bool(torch.isfinite(gt).all()) and bool(torch.isfinite(ht).all())
            first = evals == 0
            evals += 1
            if not finite and not first:
                status, rej = 3, rej + 1
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
        abs_.append(x); ls.append(loss); gs.append(g); infos.append([status, evals, acc, rej])
    return {'ab': torch.stack(abs_), 'loss': torch.stack(ls), 'g': torch.stack(gs),
            'info': torch.tensor(infos, dtype=torch.int64)}


def check_fit(z, w, train, given, relations, l2, init, max_iter, gtol, got, d_chain, c_cal=C_CAL, what='', sets=None):
    """Assert (a)-(e) for got = (ab [Q, 2] fp32, info int [Q, 4]) -> dict with the fp64 statistics at the result and at the
    start.  init: the start [Q, 2] the device was given."""
    ab, info = got[0].to(z.device), got[1].to('cpu').long()
    n = z.shape[0]
    rel = torch.as_tensor(relations).reshape(-1).long()
    sets = cell_sets(train, given, n, rel) if sets is None else sets
    start = init.to(z.device).float()
    at_w = spec_stats(z, w, ab, train, given, rel, l2, sets=sets)
    at_0 = spec_stats(z, w, start, train, given, rel, l2, sets=sets)
    best = spec_fit(z, w, train, given, rel, l2, init=start, max_iter=60, gtol=1e-10, sets=sets)
    at_best = spec_stats(z, w, best['ab'], train, given, rel, l2, bounds=False, sets=sets)
    for r in range(rel.numel()):
        status, evals, acc, rej = (int(x) for x in info[r])
        assert evals == acc + rej + 1 and evals <= max_iter + 1, (what, r, 'info', info[r].tolist())                   # (d)
        bg = gtol + bound_of(at_w, 'g', d_chain, c_cal)[r]
        if status == 1:                                                                                                # (a)
            print('calibration fit %s query %d: |g64| %.3e at (%.6f, %.6f), %d evaluations'
                  % (what, r, float(at_w['g'][r].abs().max()), float(ab[r, 0]), float(ab[r, 1]), evals))
            assert bool((at_w['g'][r].abs() <= bg).all()), (what, r, 'gradient at a converged map',
                                                            float(at_w['g'][r].abs().max()), float(bg.min()))
            big_m = float(at_w['n_pos'][r] + at_w['n_neg'][r])                                                         # (e)
            assert abs(float(at_w['expected'][r]) - float(at_w['n_pos'][r])) <= big_m * float(bg[1]), \
                (what, r, 'expected positives', float(at_w['expected'][r]), int(at_w['n_pos'][r]))
        bl = bound_of(at_w, 'loss', d_chain, c_cal)[r] + bound_of(at_0, 'loss', d_chain, c_cal)[r]
        bl = bl + 17 * U * acc * (at_0['loss'][r] + bound_of(at_0, 'loss', d_chain, c_cal)[r])
        assert float(at_w['loss'][r]) <= float(at_0['loss'][r] + bl), (what, r, 'loss above the start',                # (b)
                                                                       float(at_w['loss'][r]), float(at_0['loss'][r]), float(bl))
        gap = float(at_w['loss'][r] - at_best['loss'][r])                                                              # (c)
        room = float(at_w['g'][r].abs().max() * (ab[r].double() - best['ab'][r]).abs().sum())
        assert gap <= room + 1e-12 * (1 + abs(float(at_w['loss'][r]))), (what, r, 'convexity', gap, room)
    return {'at_w': at_w, 'at_init': at_0, 'best': best}
