"""fp64 specification of the pair rank (include/tipk.h section 4f) and the acceptance rule its results are held to.

A `model` and `known` are those of tests/pair_topk_spec.py; the targets are pair-major: pair p of `pairs` [2, P] owns
tgt_rel[tgt_ptr[p]:tgt_ptr[p + 1]].

`spec_pair_rank` is the contract in exact fp64: rank = 1 + #{c not known, c != t : L[c] > L[t] or (L[c] == L[t] and c < t)};
0 where the contract says "not ranked" (a pair index outside [0, n), a target outside [0, R), a NaN logit); a NaN candidate
beats nothing.  `check_pair_rank` holds returned ranks to the interval the rounding bound allows, with L and tau from
`logits64` (tau is the derived bound of pair_topk_spec, not a tuned number): over the candidates c (not known, c != t)
    lo = 1 + #{c : L[c] - tau[c] > L[t] + tau[t]}            (these beat t whatever the rounding did)
    hi = 1 + #{c : L[c] + tau[c] >= L[t] - tau[t]}           (only these can)
    lo <= rank <= hi   and   |logit - L[t]| <= tau[t];
rank 0 / logit NaN exactly where the contract says so.  It returns the share of ranked targets with lo < hi; a case whose
share exceeds `CAP` is too degenerate to prove anything and fails.
"""
import torch

from pair_topk_spec import known_mask, logits64

CAP = 0.01


def _lists(model, pairs, tgt_ptr, tgt_rel, dev):
    pairs = torch.as_tensor(pairs).to(dev).long().reshape(2, -1)
    tgt_ptr = torch.as_tensor(tgt_ptr).to(dev).long().reshape(-1)
    tgt_rel = torch.as_tensor(tgt_rel).to(dev).long().reshape(-1)
    n, n_rel = model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])
    assert tgt_ptr.numel() == pairs.shape[1] + 1
    owner = torch.repeat_interleave(torch.arange(pairs.shape[1], device=dev), tgt_ptr[1:] - tgt_ptr[:-1])
    assert owner.numel() == tgt_rel.numel()
    return pairs, tgt_rel, owner, n, n_rel


def spec_pair_rank(model, pairs, tgt_ptr, tgt_rel, known=None):
    """The exact fp64 pair rank -> (rank int64 [T], logit float64 [T]); (0, NaN) where a target is not ranked."""
    model = (model[0], model[1].cpu(), model[2].cpu())
    pairs, tgt_rel, owner, n, n_rel = _lists(model, pairs, tgt_ptr, tgt_rel, 'cpu')
    rank = torch.zeros(tgt_rel.numel(), dtype=torch.int64)
    logit = torch.full((tgt_rel.numel(),), float('nan'), dtype=torch.float64)
    for i, (p, t) in enumerate(zip(owner.tolist(), tgt_rel.tolist())):
        u, v = int(pairs[0, p]), int(pairs[1, p])
        if not (0 <= u < n and 0 <= v < n and 0 <= t < n_rel):
            continue
        uu, vv = torch.tensor([u]), torch.tensor([v])
        L = logits64(model, uu, vv)[0][0]
        km = known_mask(known, uu, vv, n, n_rel)[0]
        lt = float(L[t])
        if lt != lt:
            continue
        better = 0
        for c in range(n_rel):
            lc = float(L[c])
            if c != t and not bool(km[c]) and (lc > lt or (lc == lt and c < t)):
                better += 1
        rank[i], logit[i] = 1 + better, lt
    return rank, logit


def check_pair_rank(model, pairs, tgt_ptr, tgt_rel, got, known=None, chunk=4096, cap=CAP):
    """Assert the acceptance rule for got = (rank [T], logit [T] or None) (any device, any int dtype) -> the share of
    ranked targets whose interval holds more than one rank (asserted <= cap; cap=None: not asserted).  got=None: nothing
    to hold, the share alone (how the host test vets the seeds of the device cases)."""
    dev = model[1].device
    pairs, tgt_rel, owner, n, n_rel = _lists(model, pairs, tgt_ptr, tgt_rel, dev)
    T = tgt_rel.numel()
    rank = None if got is None else got[0].to(dev).long().reshape(-1)
    logit = None if got is None or got[1] is None else got[1].to(dev).double().reshape(-1)
    assert (rank is None or rank.numel() == T) and (logit is None or logit.numel() == T), T
    wide = ranked = 0
    for i0 in range(0, T, chunk):
        sl = slice(i0, i0 + chunk)
        u, v, t = pairs[0, owner[sl]], pairs[1, owner[sl]], tgt_rel[sl]
        inside = (u >= 0) & (u < n) & (v >= 0) & (v < n) & (t >= 0) & (t < n_rel)
        uc, vc, tc = u.clamp(0, n - 1), v.clamp(0, n - 1), t.clamp(0, n_rel - 1)
        L, tau = logits64(model, uc, vc)
        Lt, taut = L.gather(1, tc[:, None]), tau.gather(1, tc[:, None])
        due = inside & ~torch.isnan(Lt[:, 0])
        cand = ~known_mask(known, uc, vc, n, n_rel)
        cand.scatter_(1, tc[:, None], False)                              # c != t; the target is never a candidate of itself
        lo = 1 + (cand & (L - tau > Lt + taut)).sum(1)
        hi = 1 + (cand & (L + tau >= Lt - taut)).sum(1)
        if rank is not None:
            r = rank[sl]
            assert bool((r[~due] == 0).all()), (i0, 'a rank where the contract says not ranked')
            assert bool((r[due] > 0).all()), (i0, 'rank 0 where a rank is due')
            bad = due & ((r < lo) | (r > hi))
            if bool(bad.any()):
                j = int(torch.nonzero(bad)[0])
                raise AssertionError((i0 + j, 'rank outside its interval', int(r[j]), int(lo[j]), int(hi[j])))
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
