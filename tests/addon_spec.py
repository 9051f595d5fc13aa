"""fp64 specification of the add-on burden (include/tipk.h section 4i) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1 [n, R], s2 [n, R]) as in tests/pair_topk_spec.py.  The
contexts are the CSR pair (ctx_drugs, ctx_ptr [G + 1]); the candidates are (cand, cand_ptr [G + 1]), or (cand, None) for one
list shared by all queries.  A TASK is one (query, candidate entry); tasks are numbered query-major (`task_lists`).  `known` is
None or the pair-major lists of `ops.known_relations_by_pair`; `weights` None (all 1) or [R].

A task (q, c) is NOT APPLICABLE -- burden NaN, never selected -- when c is outside [0, n), c occurs in q's context, the
context has 0 or more than `m_max` entries or an id outside [0, n), or a triple (c, s, r) that is not known has a NaN logit.
Otherwise, over the context drugs s: the logit of (c, s, r) is that of section 4d for the pair (min(c, s), max(c, s)); a
triple CONTRIBUTES unless it is known for the pair's unordered key; per relation
  noisy_or  A_r = sum of softplus(logit) over the contributing triples, P_r = 1 - exp(-A_r)
  max       P_r = sigma(largest contributing logit)
P_r = 0 without a contributing triple, and the burden is B = sum_r weights[r] * P_r.

`spec_addon_burden` gives B64, exactly in fp64, and the tolerance of every task.  `check_addon_burden` holds a result to
the rule:
  (a) NaN sits exactly where the task is not applicable;
  (b) every other burden is within T_B = sum_r w_r * T_P,r + (R + C_BURDEN) * U * B64 of B64, where, tau being the
      per-logit bound of tests/pair_topk_spec.py,
        noisy_or  T_A = sum of the contributing taus + (n_contributing + C_NOISY) * U * A64 (tests/regimen_spec.py), and
                  T_P = exp(-max(A64 - T_A, 0)) * T_A: the mean-value bound of 1 - exp(-A) on [A64 - T_A, A64 + T_A];
        max       T_P = (largest contributing tau) / 4: the slope of sigma is at most 1/4;
      an infinite logit has an exact P (0 or 1) and adds nothing to T_P.  (R + ...) * U * B64 bounds an fp32 sum of R
      non-negative terms in any order; C_BURDEN covers the evaluation of expm1f / expf, the division and the product with
      the weight.  C_BURDEN is measured on the device (profiles/addon_burden.md): with TIPK_ERRLOG set, every check prints
      and logs the largest (|B - B64| - sum_r w_r T_P,r) / (U * B64) - R it saw;
  (c) the selection, EXACTLY, against the returned fp32 burdens: the returned positions are the k lowest non-NaN entries of
      the query's row by (value ascending, position ascending), the returned values are bit-equal to the burdens at those
      positions, and padding (+inf, -1) fills exactly the rest.
"""
import json
import os

import torch

from pair_topk_spec import U, known_mask, logits64
from regimen_spec import C_NOISY, softplus64

M_MAX = 64
C_BURDEN = 4.0     # observed on MI355X: 1.49 (profiles/addon_burden.md); "at most 30 x that and not below 4"


def _sizes(model):
    return model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])


def task_lists(ctx_ptr, cand, cand_ptr):
    """(query [T], candidate [T], task_ptr [G + 1]) of the tasks, query-major (int64, on cand's device)."""
    cand, ctx_ptr = torch.as_tensor(cand).long(), torch.as_tensor(ctx_ptr).long()
    dev = cand.device
    G = ctx_ptr.numel() - 1
    if cand_ptr is None:
        C = cand.numel()
        return (torch.arange(G, device=dev).repeat_interleave(C), cand.repeat(G), C * torch.arange(G + 1, device=dev))
    cand_ptr = torch.as_tensor(cand_ptr).long().to(dev)
    return torch.repeat_interleave(torch.arange(G, device=dev), cand_ptr[1:] - cand_ptr[:-1]), cand, cand_ptr


def spec_addon_burden(model, ctx_drugs, ctx_ptr, cand, cand_ptr, aggregate, weights=None, known=None, m_max=M_MAX,
                      c_burden=C_BURDEN, c_noisy=C_NOISY):
    """fp64 tables of the rule on the model's device: dict with B64 [T] (NaN where not applicable), T_B [T], TP_w [T]
    (sum_r w_r T_P,r), P64 [T, R], applicable [T], query [T], task_ptr [G + 1], R."""
    n, R = _sizes(model)
    dev = model[1].device
    ctx_drugs, ctx_ptr = torch.as_tensor(ctx_drugs).to(dev).long(), torch.as_tensor(ctx_ptr).to(dev).long()
    query, c, task_ptr = task_lists(ctx_ptr, torch.as_tensor(cand).to(dev), cand_ptr)
    G, T = ctx_ptr.numel() - 1, query.numel()
    w = torch.ones(R, dtype=torch.float64, device=dev) if weights is None else torch.as_tensor(weights).to(dev).double()
    m = ctx_ptr[1:] - ctx_ptr[:-1]
    bad = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    if ctx_drugs.numel():
        owner = torch.repeat_interleave(torch.arange(G, device=dev), m)
        bad.index_add_(0, owner, ((ctx_drugs < 0) | (ctx_drugs >= n)).long())
    legal_q = (m >= 1) & (m <= m_max) & (bad[:G] == 0)
    ok = legal_q[query] & (c >= 0) & (c < n)
    # (task, context drug) rows of the tasks that are legal so far
    rows = torch.nonzero(ok).reshape(-1)
    mt = m[query[rows]]
    task = torch.repeat_interleave(rows, mt)
    within = torch.arange(task.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(mt, 0) - mt, mt)
    s = ctx_drugs[ctx_ptr[query[task]] + within]
    member = torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, task, (s == c[task]).long())
    ok = ok & (member == 0)
    keep = ok[task]
    task, s = task[keep], s[keep]
    u, v = torch.minimum(c[task], s), torch.maximum(c[task], s)
    L, tau = logits64(model, u, v)
    free = ~known_mask(known, u, v, n, R)
    nan_rows = (free & torch.isnan(L)).any(1)
    ok = ok & (torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, task, nan_rows.long()) == 0)
    contrib = free & ~torch.isnan(L)
    tau_c = torch.where(contrib & ~torch.isinf(L), tau, torch.zeros_like(tau))       # an infinite logit has an exact P
    zero = torch.zeros((T, R), dtype=torch.float64, device=dev)
    idx = task[:, None].expand(-1, R)
    if aggregate == 'noisy_or':
        A64 = zero.clone().index_add_(0, task, torch.where(contrib, softplus64(L), torch.zeros_like(L)))
        n_con = zero.clone().index_add_(0, task, contrib.double())
        fin = torch.isfinite(A64)
        Af = torch.where(fin, A64, torch.zeros_like(A64))
        T_A = zero.clone().index_add_(0, task, tau_c) + (n_con + c_noisy) * U * Af
        P64 = -torch.expm1(-A64)
        T_P = torch.where(fin, torch.exp(-(Af - T_A).clamp(min=0)) * T_A, torch.zeros_like(A64))
    else:
        assert aggregate == 'max'
        ninf = torch.full((T, R), float('-inf'), dtype=torch.float64, device=dev)
        Lmax = ninf.clone().scatter_reduce_(0, idx, torch.where(contrib, L, torch.full_like(L, float('-inf'))), 'amax',
                                            include_self=True)
        P64 = torch.sigmoid(Lmax)
        T_P = zero.clone().scatter_reduce_(0, idx, tau_c, 'amax', include_self=True) / 4
    B64 = (P64 * w).sum(1)
    TP_w = (T_P * w).sum(1)
    T_B = TP_w + (R + c_burden) * U * B64
    nan = torch.full_like(B64, float('nan'))
    return dict(B64=torch.where(ok, B64, nan), T_B=torch.where(ok, T_B, nan), TP_w=TP_w, P64=P64, applicable=ok, query=query,
                task_ptr=task_ptr, R=R, dev=dev)


def expected_selection(burden, task_ptr, k):
    """The exact selection over fp32 burdens [T] of the queries task_ptr [G + 1] -> (best_burden float32 [G, k], best_pos
    int64 [G, k]): the k lowest non-NaN entries by (value, position), padded with (+inf, -1)."""
    dev = burden.device
    task_ptr = task_ptr.long()
    G = task_ptr.numel() - 1
    size = task_ptr[1:] - task_ptr[:-1]
    width = max(int(size.max()) if G else 0, 1)
    pos = torch.arange(width, device=dev)[None, :].expand(G, -1)
    inside = pos < size[:, None]
    at = (task_ptr[:-1, None] + pos).clamp(max=max(burden.numel() - 1, 0))
    rows = burden.float()[at] if burden.numel() else torch.full((G, width), float('nan'), device=dev)
    rows = torch.where(inside, rows, torch.full_like(rows, float('nan')))
    bits = rows.contiguous().view(torch.int32).long()
    order_key = torch.where(bits >= 0, bits, -(bits & 0x7fffffff))       # monotone in the float value; -0 == +0
    key = torch.where(torch.isnan(rows), torch.full_like(bits, torch.iinfo(torch.int64).max), (order_key + (1 << 31)) * (1 << 31) + pos)
    order = torch.argsort(key, dim=1)
    count = (~torch.isnan(rows)).sum(1)
    if width < k:
        order = torch.cat([order, torch.zeros((G, k - width), dtype=torch.int64, device=dev)], 1)
    order = order[:, :k]
    have = torch.arange(k, device=dev)[None, :] < count[:, None]
    vals = rows.gather(1, order.clamp(max=width - 1))
    return (torch.where(have, vals, torch.full_like(vals, float('inf'))), torch.where(have, order, torch.full_like(order, -1)))


def check_selection(burden, task_ptr, k, best_burden, best_pos):
    """Part (c) of the rule: exact, against the returned fp32 burdens."""
    want_b, want_p = expected_selection(burden.reshape(-1), task_ptr.to(burden.device), k)
    assert best_burden.shape == want_b.shape and best_pos.shape == want_p.shape, (tuple(best_burden.shape), tuple(want_b.shape))
    assert best_burden.dtype == torch.float32
    assert torch.equal(best_pos.long(), want_p), 'selection: positions are not the k lowest by (burden, position)'
    assert torch.equal(best_burden.contiguous().view(torch.int32), want_b.contiguous().view(torch.int32)), \
        'selection: values are not bit-equal to out_burden (or padding is not +inf)'


def check_addon_burden(model, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, got, weights=None, known=None, m_max=M_MAX,
                       c_burden=C_BURDEN, what=''):
    """Assert the acceptance rule for got = (burden [T] or [G, C], best_burden [G, k] or None, best_pos [G, k] or None)."""
    t = spec_addon_burden(model, ctx_drugs, ctx_ptr, cand, cand_ptr, aggregate, weights, known, m_max, c_burden)
    dev = t['dev']
    B = got[0].to(dev).reshape(-1)
    assert B.dtype == torch.float32 and B.numel() == t['B64'].numel(), (B.dtype, B.numel(), t['B64'].numel())
    ok = t['applicable']
    # (a) NaN placement
    assert torch.equal(torch.isnan(B), ~ok), ('NaN placement', int((torch.isnan(B) != ~ok).sum()))
    # (b) tolerance
    off = (B.double() - t['B64']).abs()
    if os.environ.get('TIPK_ERRLOG') and bool(ok.any()):
        pos = ok & (t['B64'] > 0) & torch.isfinite(t['B64'])
        if bool(pos.any()):
            seen = ((off - t['TP_w']) / (U * t['B64']) - t['R'])[pos]
            line = {'what': 'addon burden c', 'case': what, 'aggregate': aggregate, 'n': int(pos.sum()),
                    'observed_c': float(seen.max()), 'max_rel_err_in_u': float((off / (U * t['B64']))[pos].max()),
                    'c_burden': c_burden}
            print('ERR %s' % json.dumps(line))
            with open(os.environ['TIPK_ERRLOG'], 'a') as f:
                f.write(json.dumps(line) + '\n')
    good = (B.double() == t['B64']) | (off <= t['T_B'])
    assert bool(good[ok].all()), ('burden off fp64', float((off - t['T_B'])[ok & ~good].max()), int((ok & ~good).sum()))
    # (c) selection
    if k == 0:
        assert got[1] is None and got[2] is None
    else:
        check_selection(B, t['task_ptr'], k, got[1].to(dev), got[2].to(dev))
    return t
