"""fp64 specification of the regimen top-k (include/tipk.h section 4e) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1 [n, R], s2 [n, R]) as in tests/pair_topk_spec.py; the
regimens are the CSR pair (drugs [n_entries], ptr [G + 1]); `known` is None or the pair-major lists of
`ops.known_relations_by_pair`.  Regimen g's pairs are its position pairs i < j in lexicographic order, u = d_i, v = d_j.
A triple (pair, r) CONTRIBUTES unless it is known for the pair's unordered key or its logit is NaN; a relation with no
contributing triple is not a candidate; a regimen with fewer than 2 or more than `m_max` entries, or with an id outside
[0, n), has no candidate at all.

`spec_regimen_topk` ranks exactly in fp64 (aggregate descending, relation id ascending; the driver pair is the first pair,
in pair order, with the largest contributing logit): the spec itself, for tiny cases.  `check_regimen_topk` holds returned
rows to the acceptance rule.  With A64 the fp64 aggregate and T its rounding bound, per row:
  1. the returned relations are in [0, R), distinct and candidates;
  2. each returned score is within T of A64;
  3. the row is ordered: descending score, ties by ascending relation id;
  4. no candidate missing from a full row has A64 - T above the k-th returned relation's A64 + T;
  5. padding (-inf, -1, -1, -1) fills exactly the slots beyond the candidate count;
  6. the driver pair is a contributing pair of the regimen for that relation, and its fp64 logit is within its own tau plus
     the best pair's tau of the largest contributing fp64 logit;
  7. (max) the returned score is within the driver triple's tau of that triple's fp64 logit.
T is the rounding bound of the contract, tau being the per-logit bound of tests/pair_topk_spec.py:
  max       the largest tau among the relation's contributing triples (max is exact, so the score is one of the logits);
  noisy-or  sum of the contributing taus (softplus is 1-Lipschitz) + (n_contributing + C_NOISY) * 2^-24 * A64: the ordered
            fp32 sum of n terms costs at most n roundings of a partial sum <= A64 (all terms are >= 0), and C_NOISY covers
            the evaluation of expf / log1pf and the add inside softplus.  C_NOISY is measured on the device
            (profiles/regimen_errors.md): with TIPK_ERRLOG set, every noisy-or check prints and logs the largest
            (|A - A64| - sum tau) / (2^-24 A64) - n_contributing it saw.
"""
import json
import os

import torch

from pair_topk_spec import U, known_mask, logits64

M_MAX = 64
C_NOISY = 4.0      # observed on MI355X: 0.31; "at most 30 x that and not below 4" (profiles/regimen_errors.md)


def softplus64(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def regimen_pairs(drugs, ptr, n, m_max=M_MAX):
    """The pairs of the legal regimens, flat and in pair order -> (reg, i, j, u, v, first [G], m [G], legal [G]): int64
    tensors on drugs' device; first[g] is the flat index of regimen g's pair (0, 1)."""
    dev = drugs.device
    drugs, ptr = drugs.long(), ptr.long()
    G = ptr.numel() - 1
    m = ptr[1:] - ptr[:-1]
    bad = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    if drugs.numel():
        owner = torch.repeat_interleave(torch.arange(G, device=dev), m)
        bad.index_add_(0, owner, ((drugs < 0) | (drugs >= n)).long())
    legal = (m >= 2) & (m <= m_max) & (bad[:G] == 0)
    ml = torch.where(legal, m, torch.zeros_like(m))
    count = ml * (ml - 1) // 2
    first = torch.cumsum(count, 0) - count
    reg = torch.repeat_interleave(torch.arange(G, device=dev), count)
    within = torch.arange(reg.numel(), device=dev) - first[reg]
    # pair number `within` of a list of length m: row i is the largest i with i*m - i(i+1)/2 <= within
    mm = ml[reg]
    i = torch.zeros_like(within)
    for _ in range(int(ml.max()) if G and reg.numel() else 0):
        nxt = i + 1
        i = torch.where((nxt * mm - nxt * (nxt + 1) // 2 <= within) & (nxt < mm - 1), nxt, i)
    j = within - (i * mm - i * (i + 1) // 2) + i + 1
    u, v = drugs[ptr[reg] + i], drugs[ptr[reg] + j]
    return reg, i, j, u, v, first, ml, legal


def _sizes(model):
    return model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])


def _aggregates(model, drugs, ptr, aggregate, known, m_max, c_noisy):
    """fp64 tables of the rule: dict with L, tau, contrib [P, R] per flat pair and A64, T, cand, Lmax, tau_best [G, R]."""
    n, R = _sizes(model)
    dev = model[1].device
    drugs, ptr = torch.as_tensor(drugs).to(dev), torch.as_tensor(ptr).to(dev)
    reg, i, j, u, v, first, m, legal = regimen_pairs(drugs, ptr, n, m_max)
    G = ptr.numel() - 1
    L, tau = logits64(model, u, v)
    contrib = ~known_mask(known, u, v, n, R) & ~torch.isnan(L)
    idx = reg[:, None].expand(-1, R)
    ninf = torch.full((G, R), float('-inf'), dtype=torch.float64, device=dev)
    Lc = torch.where(contrib, L, torch.full_like(L, float('-inf')))
    n_con = torch.zeros((G, R), dtype=torch.float64, device=dev).index_add_(0, reg, contrib.double())
    cand = n_con > 0
    Lmax = ninf.clone().scatter_reduce_(0, idx, Lc, 'amax', include_self=True)
    is_best = contrib & (Lc == Lmax[reg])
    tau_best = ninf.clone().scatter_reduce_(0, idx, torch.where(is_best, tau, torch.full_like(tau, float('-inf'))), 'amax',
                                            include_self=True)
    tau_c = torch.where(contrib, tau, torch.zeros_like(tau))
    if aggregate == 'max':
        A64 = Lmax
        T = torch.zeros((G, R), dtype=torch.float64, device=dev).scatter_reduce_(0, idx, tau_c, 'amax', include_self=True)
        tau_sum = None
    else:
        assert aggregate == 'noisy_or'
        sp = torch.where(contrib, softplus64(L), torch.zeros_like(L))
        A64 = torch.zeros((G, R), dtype=torch.float64, device=dev).index_add_(0, reg, sp)
        tau_sum = torch.zeros((G, R), dtype=torch.float64, device=dev).index_add_(0, reg, tau_c)
        T = tau_sum + (n_con + c_noisy) * U * A64
        A64 = torch.where(cand, A64, ninf)
    return dict(reg=reg, i=i, j=j, first=first, m=m, L=L, tau=tau, contrib=contrib, A64=A64, T=T, cand=cand, Lmax=Lmax,
                tau_best=tau_best, n_con=n_con, tau_sum=tau_sum, G=G, R=R, dev=dev)


def spec_regimen_topk(model, drugs, ptr, k, aggregate, known=None, m_max=M_MAX):
    """The exact fp64 regimen top-k -> (score float64 [G, k], relation, pair_i, pair_j int64 [G, k]), padding
    (-inf, -1, -1, -1)."""
    model = (model[0], model[1].cpu(), model[2].cpu())
    t = _aggregates(model, torch.as_tensor(drugs).cpu(), torch.as_tensor(ptr).cpu(), aggregate, known, m_max, 0.0)
    G, R = t['G'], t['R']
    out_s = torch.full((G, k), float('-inf'), dtype=torch.float64)
    out = [torch.full((G, k), -1, dtype=torch.int64) for _ in range(3)]
    for g in range(G):
        cands = sorted((-float(t['A64'][g, r]), r) for r in range(R) if bool(t['cand'][g, r]))
        rows = torch.nonzero(t['reg'] == g).reshape(-1).tolist()
        for slot, (s, r) in enumerate(cands[:k]):
            best = None
            for p in rows:                                               # pair order; strict >: ties to the first
                if bool(t['contrib'][p, r]) and (best is None or float(t['L'][p, r]) > float(t['L'][best, r])):
                    best = p
            out_s[g, slot], out[0][g, slot], out[1][g, slot], out[2][g, slot] = -s, r, int(t['i'][best]), int(t['j'][best])
    return (out_s, *out)


def check_regimen_topk(model, drugs, ptr, k, aggregate, got, known=None, m_max=M_MAX, c_noisy=C_NOISY, what=''):
    """Assert the acceptance rule for got = (score [G, k], relation, pair_i, pair_j [G, k]) (any device, any int dtype)."""
    t = _aggregates(model, drugs, ptr, aggregate, known, m_max, c_noisy)
    dev, G, R = t['dev'], t['G'], t['R']
    s, r, pi, pj = got[0].to(dev), got[1].to(dev).long(), got[2].to(dev).long(), got[3].to(dev).long()
    for x in (s, r, pi, pj):
        assert x.shape == (G, k), (tuple(x.shape), (G, k))
    if G == 0:
        return
    A64, T, cand = t['A64'], t['T'], t['cand']
    slot = torch.arange(k, device=dev)
    # 5. padding
    nv = (r >= 0).sum(1)
    valid = slot[None, :] < nv[:, None]
    assert bool(((r >= 0) == valid).all()), 'padding: valid entries are not a prefix'
    assert bool((r[~valid] == -1).all()) and bool(torch.isneginf(s[~valid]).all()), 'padding is not (-inf, -1)'
    assert bool((pi[~valid] == -1).all()) and bool((pj[~valid] == -1).all()), 'padding pair is not (-1, -1)'
    assert bool((nv == cand.sum(1).clamp(max=k)).all()), 'returned count is not min(k, candidates)'
    # 1. range, candidates, distinct
    assert bool((r[valid] < R).all()), 'relation out of range'
    rc = r.clamp(min=0, max=R - 1)
    assert bool(cand.gather(1, rc)[valid].all()), 'a relation without a contributing triple returned'
    hits = torch.zeros((G, R), dtype=torch.int32, device=dev).scatter_add_(1, rc, valid.to(torch.int32))
    assert int(hits.max()) <= 1, 'duplicate relation'
    assert not bool(torch.isnan(s).any()), 'NaN returned'
    # 2. scores
    a64, tt = A64.gather(1, rc), T.gather(1, rc)
    off = (s.double() - a64).abs()
    ok = (s.double() == a64) | (off <= tt)                               # (equal infinities have no difference)
    if aggregate == 'noisy_or' and os.environ.get('TIPK_ERRLOG') and bool(valid.any()):
        fin = valid & torch.isfinite(a64) & (a64 > 0)
        if bool(fin.any()):
            seen = ((off - t['tau_sum'].gather(1, rc)) / (U * a64) - t['n_con'].gather(1, rc))[fin]
            line = {'what': 'regimen noisy_or c', 'case': what, 'n': int(fin.sum()), 'observed_c': float(seen.max()),
                    'max_rel_err_in_u': float((off / (U * a64))[fin].max()), 'c_noisy': c_noisy}
            print('ERR %s' % json.dumps(line))
            with open(os.environ['TIPK_ERRLOG'], 'a') as f:
                f.write(json.dumps(line) + '\n')
    assert bool(ok[valid].all()), ('score off fp64', float((off - tt)[valid & ~ok].max()))
    # 3. order
    if k > 1:
        inorder = (s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (r[:, :-1] < r[:, 1:]))
        assert bool(inorder[valid[:, 1:]].all()), 'order'
    # 4. completeness of full rows
    full = nv == k
    if bool(full.any()):
        bound = a64[:, k - 1] + tt[:, k - 1]
        missing = cand & (hits == 0)
        worst = torch.where(missing, A64 - T, torch.full_like(A64, float('-inf'))).amax(1)
        good = (worst <= bound) | (worst == float('-inf'))
        assert bool(good[full].all()), 'a better relation is missing'
    # 6. driver pair
    m = t['m'][:, None].expand(-1, k)
    assert bool(((pi >= 0) & (pi < pj) & (pj < m))[valid].all()), 'driver pair is not a position pair of the regimen'
    flat = (t['first'][:, None] + pi * m - pi * (pi + 1) // 2 + (pj - pi - 1))[valid]
    rv = rc[valid]
    assert bool(t['contrib'][flat, rv].all()), 'driver pair does not contribute'
    ld, td = t['L'][flat, rv], t['tau'][flat, rv]
    lbest, tbest = t['Lmax'].gather(1, rc)[valid], t['tau_best'].gather(1, rc)[valid]
    assert bool(((ld == lbest) | (ld >= lbest - (td + tbest))).all()), 'driver pair is not the best pair'
    # 7. max: the score is the driver triple's logit
    if aggregate == 'max':
        sv = s[valid].double()
        assert bool(((sv == ld) | ((sv - ld).abs() <= td)).all()), 'max score is not the driver triple\'s logit'
