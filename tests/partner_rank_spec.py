"""fp64 specification of the partner rank (include/tipk.h section 4g) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1t [R, n], s2t [R, n]) (the RELATION-major tables); `known`
is None or the relation-major lists (keys int64 u*n+v sorted inside each relation, ptr int64 [R + 1]) of the screen.  The
targets are query-major: query q = (q_rel[q], q_drug[q]) owns tgt_node[tgt_ptr[q]:tgt_ptr[q + 1]].

`spec_partner_rank` is the contract in exact fp64, with Python loops: for a target t of query (r, u), over the candidates c
in [0, n) with c != u and neither u*n+c nor c*n+u a key of r,
    rank = 1 + #{c != t : L[c] > L[t] or (L[c] == L[t] and c < t)};
0 where the contract says "not ranked" (r outside [0, R), u or t outside [0, n), t == u, a NaN logit); a NaN candidate beats
nothing.  `check_partner_rank` is the interval rule of tests/pair_rank_spec.py carried over, with L and tau from
`query_logits64`: over the same candidates c != t
    lo = 1 + #{c : L[c] - tau[c] > L[t] + tau[t]}            (these beat t whatever the rounding did)
    hi = 1 + #{c : L[c] + tau[c] >= L[t] - tau[t]}           (only these can)
    lo <= rank <= hi   and   |logit - L[t]| <= tau[t];
rank 0 / logit NaN exactly where the contract says so.  It returns the share of ranked targets with lo < hi; a case whose
share exceeds `CAP` is too degenerate to prove anything and fails: the cap is a condition, not a measurement.
tau is the rounding bound of the contract's arithmetic, not a tuned number:
  DistMult  (dim + 2) * 2^-24 * sum_k |z_u w_r z_c|: a_k = z_u w_r is rounded once, each of the dim ordered fma's rounds once,
            so a term passes at most dim + 1 roundings; the + 2 covers the second-order terms (the bound of pair_topk_spec);
  table     2^-24 * |s1t + s2t|: one fp32 add.
"""
import torch

U = 2.0 ** -24
CAP = 0.01


def sizes(model):
    """(n, n_rel) of a model."""
    return (model[1].shape[0], model[2].shape[0]) if model[0] == 'distmult' else (model[1].shape[1], model[1].shape[0])


def query_logits64(model, r, u):
    """(fp64 logits [Q, n], tau [Q, n]) of every drug for the queries (r, u) (int64 tensors on the model's device)."""
    kind, a, b = model
    if kind == 'distmult':
        q = a.double()[u] * b.double()[r]
        z = a.double()
        return q @ z.t(), (a.shape[1] + 2) * U * (q.abs() @ z.abs().t())
    assert kind == 'table'
    L = a.double()[r, u][:, None] + b.double()[r]
    return L, U * L.abs()


def known_mask(known, r, u, n):
    """bool [Q, n]: drug c is listed for query (r, u): u*n+c or c*n+u is a key of relation r."""
    dev = u.device
    c = torch.arange(n, device=dev)[None, :]
    mask = torch.zeros((u.numel(), n), dtype=torch.bool, device=dev)
    if known is None or known[0].numel() == 0 or u.numel() == 0:
        return mask
    keys, ptr = (t.to(dev).long() for t in known)
    rel = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1])
    comb = rel * (n * n) + keys                                           # ascending: relation-major, sorted inside
    for probe in (u[:, None] * n + c, c * n + u[:, None]):
        probe = r[:, None] * (n * n) + probe
        at = torch.searchsorted(comb, probe).clamp(max=comb.numel() - 1)
        mask |= comb[at] == probe
    return mask


def _lists(model, q_rel, q_drug, tgt_ptr, tgt_node, dev):
    q_rel, q_drug, tgt_ptr, tgt_node = (torch.as_tensor(t).to(dev).long().reshape(-1) for t in (q_rel, q_drug, tgt_ptr, tgt_node))
    assert q_rel.numel() == q_drug.numel() == tgt_ptr.numel() - 1
    owner = torch.repeat_interleave(torch.arange(q_rel.numel(), device=dev), tgt_ptr[1:] - tgt_ptr[:-1])
    assert owner.numel() == tgt_node.numel()
    return q_rel, q_drug, tgt_node, owner


def spec_partner_rank(model, q_rel, q_drug, tgt_ptr, tgt_node, known=None):
    """The exact fp64 partner rank -> (rank int64 [T], logit float64 [T]); (0, NaN) where a target is not ranked."""
    model = (model[0], model[1].cpu(), model[2].cpu())
    q_rel, q_drug, tgt_node, owner = _lists(model, q_rel, q_drug, tgt_ptr, tgt_node, 'cpu')
    n, n_rel = sizes(model)
    listed = set()
    if known is not None:
        keys, ptr = (t.cpu().tolist() for t in known)
        listed = {(r, k) for r in range(n_rel) for k in keys[ptr[r]:ptr[r + 1]]}
    rank = torch.zeros(tgt_node.numel(), dtype=torch.int64)
    logit = torch.full((tgt_node.numel(),), float('nan'), dtype=torch.float64)
    for i, (q, t) in enumerate(zip(owner.tolist(), tgt_node.tolist())):
        r, u = int(q_rel[q]), int(q_drug[q])
        if not (0 <= r < n_rel and 0 <= u < n and 0 <= t < n) or t == u:
            continue
        L = query_logits64(model, torch.tensor([r]), torch.tensor([u]))[0][0].tolist()
        lt = L[t]
        if lt != lt:
            continue
        better = 0
        for c in range(n):
            if c == u or c == t or (r, u * n + c) in listed or (r, c * n + u) in listed:
                continue
            if L[c] > lt or (L[c] == lt and c < t):
                better += 1
        rank[i], logit[i] = 1 + better, lt
    return rank, logit


def check_partner_rank(model, q_rel, q_drug, tgt_ptr, tgt_node, got, known=None, chunk=4096, cap=CAP):
    """Assert the acceptance rule for got = (rank [T], logit [T] or None) (any device, any int dtype) -> the share of
    ranked targets whose interval holds more than one rank (asserted <= cap; cap=None: not asserted).  got=None: nothing
    to hold, the share alone (how the host test vets the seeds of the device cases)."""
    dev = model[1].device
    q_rel, q_drug, tgt_node, owner = _lists(model, q_rel, q_drug, tgt_ptr, tgt_node, dev)
    n, n_rel = sizes(model)
    T = tgt_node.numel()
    rank = None if got is None else got[0].to(dev).long().reshape(-1)
    logit = None if got is None or got[1] is None else got[1].to(dev).double().reshape(-1)
    assert (rank is None or rank.numel() == T) and (logit is None or logit.numel() == T), T
    ids = torch.arange(n, device=dev)[None, :]
    wide = ranked = 0
    for i0 in range(0, T, chunk):
        sl = slice(i0, i0 + chunk)
        r, u, t = q_rel[owner[sl]], q_drug[owner[sl]], tgt_node[sl]
        inside = (r >= 0) & (r < n_rel) & (u >= 0) & (u < n) & (t >= 0) & (t < n) & (t != u)
        rc, uc, tc = r.clamp(0, n_rel - 1), u.clamp(0, n - 1), t.clamp(0, n - 1)
        L, tau = query_logits64(model, rc, uc)
        Lt, taut = L.gather(1, tc[:, None]), tau.gather(1, tc[:, None])
        due = inside & ~torch.isnan(Lt[:, 0])
        cand = ~known_mask(known, rc, uc, n) & (ids != uc[:, None])
        cand.scatter_(1, tc[:, None], False)                              # c != t; the target is never a candidate of itself
        lo = 1 + (cand & (L - tau > Lt + taut)).sum(1)
        hi = 1 + (cand & (L + tau >= Lt - taut)).sum(1)
        if rank is not None:
            k = rank[sl]
            assert bool((k[~due] == 0).all()), (i0, 'a rank where the contract says not ranked')
            assert bool((k[due] > 0).all()), (i0, 'rank 0 where a rank is due')
            bad = due & ((k < lo) | (k > hi))
            if bool(bad.any()):
                j = int(torch.nonzero(bad)[0])
                raise AssertionError((i0 + j, 'rank outside its interval', int(k[j]), int(lo[j]), int(hi[j])))
        if logit is not None:
            g = logit[sl]
            assert bool(torch.isnan(g[~due]).all()), (i0, 'a logit where the contract says NaN')
            off = (g - Lt[:, 0]).abs()
            assert bool((off <= taut[:, 0])[due].all()), (i0, 'logit off fp64')
        wide += int((due & (lo < hi)).sum())
        ranked += int(due.sum())
    share = wide / ranked if ranked else 0.0
    if cap is not None:
        assert share <= cap, ('too many targets with more than one admissible rank: the case proves nothing', share)
    return share
