"""fp64 specification of the partner sum (include/tipk.h section 4l) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1t [R, n], s2t [R, n]) (the RELATION-major tables), as in
tests/partner_rank_spec.py, whose `query_logits64` (fp64 logits and the per-logit bound tau) and `U` are used here.  The
queried drugs are q_drug [Q]; the columns are rel_ids [S] (None: all R relations); partner_w is None (all 1) or [n]; `known`
is None or the relation-major lists (keys int64 u*n+v sorted inside each relation, ptr int64 [R + 1]).

Cell (q, j), u = q_drug[q], r = rel_ids[j]: the candidates are the drugs c in [0, n) with c != u, partner_w[c] != 0 and
u*n+c NOT a key of r -- the FORWARD key only (`forward_mask`: `partner_rank_spec.known_mask` looks up both directions, which
is not this contract); E = sum over the candidates of partner_w[c] * sigma(L[c]), count = their number.  A candidate with a
NaN logit makes the cell NaN; a drug that is no candidate never reaches the sum.  u outside [0, n) or r outside [0, R): (NaN, 0).

`check_partner_sum` holds a result to the rule:
  (a) NaN sits exactly where the contract says, and `count` is exact;
  (b) every other cell satisfies |E - E64| <= sum_c pw_c * tau_c / 4 + (n_contrib + C_PROFILE) * U * E64: the slope of sigma
      is at most 1/4; (n + C) * U * E64 bounds an fp32 sum of n non-negative terms in any order, C covering the evaluation of
      sigma (expf, the add, the division) and the product with the weight; an infinite logit has an exact sigma (0 or 1) and
      adds nothing to the first term.  C_PROFILE is measured on the device (profiles/drug_profile.md): with TIPK_ERRLOG set,
      every check prints and logs the largest (|E - E64| - sum_c pw_c tau_c / 4) / (U * E64) - n_contrib it saw;
  (c) the selection, EXACTLY, against the returned fp32 sums: the returned positions are the k largest non-NaN cells of the
      row by (value descending, position ascending; +0 and -0 tie), the returned values are bit-equal to the sums at those
      positions, and padding (-inf, -1) fills exactly the rest.
"""
import json
import math
import os

import torch

from partner_rank_spec import U, query_logits64, sizes

C_PROFILE = 4.0     # observed on MI355X: 0.35 (profiles/drug_profile.md); "at most 30 x that and not below 4"


def forward_mask(known, r, u, n):
    """bool [P, n]: drug c is recorded for the pair query (r[p], u[p]) in the FORWARD direction: u*n+c is a key of r."""
    dev = u.device
    mask = torch.zeros((u.numel(), n), dtype=torch.bool, device=dev)
    if known is None or known[0].numel() == 0 or u.numel() == 0:
        return mask
    keys, ptr = (t.to(dev).long() for t in known)
    rel = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1])
    comb = rel * (n * n) + keys                                           # ascending: relation-major, sorted inside
    probe = r[:, None] * (n * n) + u[:, None] * n + torch.arange(n, device=dev)[None, :]
    at = torch.searchsorted(comb, probe).clamp(max=comb.numel() - 1)
    return comb[at] == probe


def _columns(model, rel_ids, dev):
    n, n_rel = sizes(model)
    rel = torch.arange(n_rel, device=dev) if rel_ids is None else torch.as_tensor(rel_ids).to(dev).long().reshape(-1)
    return n, n_rel, rel


def spec_partner_sum(model, q_drug, rel_ids=None, partner_w=None, known=None):
    """fp64 tables of the rule on the model's device, one queried drug at a time (so the largest temporary is [S, n]): dict
    with E64 [Q, S] (NaN where the contract says so), count int64 [Q, S], T_tau [Q, S] (sum_c pw_c tau_c / 4), n_contrib
    [Q, S] (= count where the cell is defined)."""
    dev = model[1].device
    n, n_rel, rel = _columns(model, rel_ids, dev)
    q_drug = torch.as_tensor(q_drug).to(dev).long().reshape(-1)
    pw = torch.ones(n, dtype=torch.float64, device=dev) if partner_w is None else torch.as_tensor(partner_w).to(dev).double()
    Q, S = q_drug.numel(), rel.numel()
    E = torch.full((Q, S), float('nan'), dtype=torch.float64, device=dev)
    T = torch.zeros((Q, S), dtype=torch.float64, device=dev)
    count = torch.zeros((Q, S), dtype=torch.int64, device=dev)
    rok = (rel >= 0) & (rel < n_rel)
    rc = rel.clamp(0, n_rel - 1)
    ids = torch.arange(n, device=dev)[None, :]
    for q, u in enumerate(q_drug.tolist()):
        if not (0 <= u < n) or S == 0:
            continue
        uu = torch.full((S,), u, dtype=torch.int64, device=dev)
        L, tau = query_logits64(model, rc, uu)
        cand = (ids != u) & (pw != 0)[None, :] & ~forward_mask(known, rc, uu, n) & rok[:, None]
        term = pw[None, :] * torch.sigmoid(L)
        zero = torch.zeros_like(term)
        E[q] = torch.where(rok, torch.where(cand, term, zero).sum(1), torch.full_like(E[q], float('nan')))
        exact = torch.isinf(L) | torch.isnan(L)
        T[q] = torch.where(cand & ~exact, pw[None, :] * tau / 4, zero).sum(1)
        count[q] = cand.sum(1)
    return dict(E64=E, count=count, T_tau=T, dev=dev)


def loop_partner_sum(model, q_drug, rel_ids=None, partner_w=None, known=None, count_self=False, multiply_zero=False,
                     reverse_only=False):
    """The contract as a plain Python triple loop over (queried drug, column, partner) with `math` arithmetic -> (E [Q, S]
    float64, count [Q, S] int64).  The three flags plant the mistakes the rule must reject: u counted as its own partner, a
    weight of 0 multiplied instead of skipped (its NaN logit then poisons the cell and it is counted), the reverse key c*n+u
    looked up instead of the forward one."""
    kind, a, b = model[0], model[1].double().tolist(), model[2].double().tolist()
    n, n_rel = sizes(model)
    rel = list(range(n_rel)) if rel_ids is None else torch.as_tensor(rel_ids).reshape(-1).tolist()
    pw = [1.0] * n if partner_w is None else torch.as_tensor(partner_w).double().tolist()
    listed = set()
    if known is not None:
        keys, ptr = (t.tolist() for t in known)
        listed = {(r, key) for r in range(n_rel) for key in keys[ptr[r]:ptr[r + 1]]}
    q_drug = torch.as_tensor(q_drug).reshape(-1).tolist()
    E = torch.full((len(q_drug), len(rel)), float('nan'), dtype=torch.float64)
    count = torch.zeros((len(q_drug), len(rel)), dtype=torch.int64)
    for qi, u in enumerate(q_drug):
        for j, r in enumerate(rel):
            if not (0 <= u < n and 0 <= r < n_rel):
                continue
            total, m = 0.0, 0
            for c in range(n):
                if c == u and not count_self:
                    continue
                if pw[c] == 0 and not multiply_zero:
                    continue
                if (r, (c * n + u) if reverse_only else (u * n + c)) in listed:
                    continue
                if kind == 'distmult':
                    s = math.fsum(a[u][i] * b[r][i] * a[c][i] for i in range(len(a[u])))
                else:
                    s = a[r][u] + b[r][c]
                if s != s:
                    sig = float('nan')
                elif s >= 0:
                    sig = 1.0 / (1.0 + math.exp(-s))
                else:
                    e = math.exp(s)
                    sig = e / (1.0 + e)
                total += pw[c] * sig
                m += 1
            E[qi, j], count[qi, j] = total, m
    return E, count


def expected_top(sums, k):
    """The exact selection over the fp32 sums [Q, S] -> (top_val float32 [Q, k], top_pos int64 [Q, k]): the k largest non-NaN
    cells of each row by (value descending, position ascending), padded with (-inf, -1)."""
    sums = sums.float()
    dev = sums.device
    Q, S = sums.shape
    if S == 0:
        return (torch.full((Q, k), float('-inf'), dtype=torch.float32, device=dev),
                torch.full((Q, k), -1, dtype=torch.int64, device=dev))
    nan = torch.isnan(sums)
    key = torch.where(nan, torch.zeros_like(sums), -sums)                # -(+0) == -(-0): they tie; stable: by position
    order = torch.argsort(key, dim=1, stable=True)
    order = order.gather(1, torch.argsort(nan.gather(1, order).long(), dim=1, stable=True))     # NaN cells last
    n_have = (~nan).sum(1)
    if S < k:
        order = torch.cat([order, torch.zeros((Q, k - S), dtype=torch.int64, device=dev)], 1)
    order = order[:, :k]
    have = torch.arange(k, device=dev)[None, :] < n_have[:, None]
    vals = sums.gather(1, order)
    return torch.where(have, vals, torch.full_like(vals, float('-inf'))), torch.where(have, order, torch.full_like(order, -1))


def check_top(sums, k, top_val, top_pos):
    """Part (c) of the rule: exact, against the returned fp32 sums."""
    want_v, want_p = expected_top(sums, k)
    assert top_val.shape == want_v.shape and top_pos.shape == want_p.shape, (tuple(top_val.shape), tuple(want_v.shape))
    assert top_val.dtype == torch.float32
    assert torch.equal(top_pos.long(), want_p), 'selection: positions are not the k largest by (sum descending, position)'
    assert torch.equal(top_val.contiguous().view(torch.int32), want_v.contiguous().view(torch.int32)), \
        'selection: values are not bit-equal to out_sum (or padding is not -inf)'


def check_partner_sum(model, q_drug, k, got, rel_ids=None, partner_w=None, known=None, c_profile=C_PROFILE, what=''):
    """Assert the acceptance rule for got = (sum [Q, S], count [Q, S], top_val [Q, k] or None, top_pos [Q, k] or None) -> the
    spec's tables (with 'observed_c': the largest C this result needs, -inf without a positive cell)."""
    t = spec_partner_sum(model, q_drug, rel_ids, partner_w, known)
    dev = t['dev']
    E, cnt = got[0].to(dev), got[1].to(dev).long()
    E64 = t['E64']
    assert E.dtype == torch.float32 and E.shape == E64.shape and cnt.shape == E64.shape, (E.dtype, tuple(E.shape), tuple(E64.shape))
    # (a) NaN placement and the counts
    assert torch.equal(torch.isnan(E), torch.isnan(E64)), ('NaN placement', int((torch.isnan(E) != torch.isnan(E64)).sum()))
    assert torch.equal(cnt, t['count']), ('count', int((cnt != t['count']).sum()))
    # (b) tolerance
    ok = ~torch.isnan(E64)
    off = (E.double() - E64).abs()
    n_con = t['count'].double()
    pos = ok & (E64 > 0) & torch.isfinite(E64)
    t['observed_c'] = float(((off - t['T_tau']) / (U * E64) - n_con)[pos].max()) if bool(pos.any()) else float('-inf')
    if os.environ.get('TIPK_ERRLOG') and bool(pos.any()):
        line = {'what': 'partner sum c', 'case': what, 'n': int(pos.sum()), 'observed_c': t['observed_c'],
                'max_rel_err_in_u': float((off / (U * E64))[pos].max()), 'c_profile': c_profile}
        print('ERR %s' % json.dumps(line))
        with open(os.environ['TIPK_ERRLOG'], 'a') as f:
            f.write(json.dumps(line) + '\n')
    bound = t['T_tau'] + (n_con + c_profile) * U * E64
    good = (E.double() == E64) | (off <= bound)
    assert bool(good[ok].all()), ('sum off fp64', float((off - bound)[ok & ~good].max()), int((ok & ~good).sum()))
    # (c) selection
    if k == 0:
        assert got[2] is None or got[2].numel() == 0
    else:
        check_top(E, k, got[2].to(dev), got[3].to(dev))
    return t
