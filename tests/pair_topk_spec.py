"""fp64 specification of the pair top-k (include/tipk.h section 4d) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1 [n, R], s2 [n, R]); `known` is None or the pair-major
lists (pair_keys, pair_ptr, rel) of `ops.known_relations_by_pair`.

`spec_pair_topk` ranks the relations of every pair exactly (fp64 logit descending, relation id ascending): the spec itself,
for tiny cases.  `check_pair_topk` holds returned rows to the acceptance rule against fp64, chunked over the pairs, on
whatever device the model's tensors are on.  Per row:
  1. the returned relations are in [0, R), distinct and not known for the pair (in either pair direction);
  2. each returned logit is within tau of the triple's fp64 logit;
  3. the row is ordered: descending logit, ties by ascending relation id;
  4. no unfiltered relation missing from a full row has an fp64 logit above the k-th returned relation's fp64 logit + the
     two taus;
  5. padding (-inf, -1) fills exactly the slots beyond the candidate count.
tau is the rounding bound of the contract's arithmetic, not a tuned number:
  DistMult  (dim + 2) * 2^-24 * sum_k |z_u z_v w_r|: h_k = z_u z_v is rounded once, each of the dim ordered fma's rounds once,
            so a term passes at most dim + 1 roundings; the + 2 covers the second-order terms;
  table     2^-24 * |s1 + s2|: one fp32 add.
"""
import torch

U = 2.0 ** -24


def logits64(model, u, v):
    """(fp64 logits [P, R], tau [P, R]) of the pairs (u, v) (int64 tensors on the model's device)."""
    kind, a, b = model
    if kind == 'distmult':
        h = a.double()[u] * a.double()[v]
        w = b.double()
        return h @ w.t(), (a.shape[1] + 2) * U * (h.abs() @ w.abs().t())
    assert kind == 'table'
    L = a.double()[u] + b.double()[v]
    return L, U * L.abs()


def known_mask(known, u, v, n, n_rel):
    """bool [P, R]: relation r is listed for the unordered key of pair p."""
    dev = u.device
    mask = torch.zeros((u.numel(), n_rel), dtype=torch.bool, device=dev)
    if known is None or known[0].numel() == 0 or u.numel() == 0:
        return mask
    keys, ptr, rel = (t.to(dev).long() for t in known)
    pk = torch.minimum(u, v) * n + torch.maximum(u, v)
    at = torch.searchsorted(keys, pk).clamp(max=keys.numel() - 1)
    found = keys[at] == pk
    rows = torch.nonzero(found).reshape(-1)
    first, count = ptr[at[rows]], ptr[at[rows] + 1] - ptr[at[rows]]
    owner = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), count)
    within = torch.arange(owner.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(count, 0) - count, count)
    mask[rows[owner], rel[first[owner] + within]] = True
    return mask


def known_from_dict(d, n):
    """{(u, v): [relations]} (any pair direction, any order) -> (pair_keys, pair_ptr, rel) on the host."""
    merged = {}
    for (u, v), rels in d.items():
        merged.setdefault(min(u, v) * n + max(u, v), set()).update(int(r) for r in rels)
    keys = sorted(k for k in merged if merged[k])
    ptr, rel = [0], []
    for k in keys:
        rel += sorted(merged[k])
        ptr.append(len(rel))
    return (torch.tensor(keys, dtype=torch.int64), torch.tensor(ptr, dtype=torch.int64), torch.tensor(rel, dtype=torch.int32))


def spec_pair_topk(model, pairs, k, known=None):
    """The exact fp64 pair top-k -> (logit float64 [P, k], relation int64 [P, k]), padding (-inf, -1)."""
    model = (model[0], model[1].cpu(), model[2].cpu())
    pairs = torch.as_tensor(pairs).cpu().long().reshape(2, -1)
    n, n_rel = model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])
    L, _ = logits64(model, pairs[0], pairs[1])
    km = known_mask(known, pairs[0], pairs[1], n, n_rel)
    out_s = torch.full((pairs.shape[1], k), float('-inf'), dtype=torch.float64)
    out_r = torch.full((pairs.shape[1], k), -1, dtype=torch.int64)
    for p in range(pairs.shape[1]):
        cands = sorted((-float(L[p, r]), r) for r in range(n_rel) if not bool(km[p, r]))
        for j, (s, r) in enumerate(cands[:k]):
            out_s[p, j], out_r[p, j] = -s, r
    return out_s, out_r


def check_pair_topk(model, pairs, k, got, known=None, chunk=8192):
    """Assert the acceptance rule for got = (logits [P, k], relation [P, k]) (any device, any int dtype)."""
    dev = model[1].device
    pairs = torch.as_tensor(pairs).to(dev).long().reshape(2, -1)
    n, n_rel = model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])
    P = pairs.shape[1]
    s_all, r_all = got[0].to(dev), got[1].to(dev).long()
    assert s_all.shape == (P, k) and r_all.shape == (P, k), (tuple(s_all.shape), tuple(r_all.shape), (P, k))
    slot = torch.arange(k, device=dev)
    for p0 in range(0, P, chunk):
        u, v = pairs[0, p0:p0 + chunk], pairs[1, p0:p0 + chunk]
        s, r = s_all[p0:p0 + chunk], r_all[p0:p0 + chunk]
        L, T = logits64(model, u, v)
        km = known_mask(known, u, v, n, n_rel)
        n_cand = (~km).sum(1)
        # 5. padding
        nv = (r >= 0).sum(1)
        valid = slot[None, :] < nv[:, None]
        assert bool(((r >= 0) == valid).all()), (p0, 'padding: valid entries are not a prefix')
        assert bool((r[~valid] == -1).all()) and bool(torch.isneginf(s[~valid]).all()), (p0, 'padding is not (-inf, -1)')
        assert bool((nv == n_cand.clamp(max=k)).all()), (p0, 'returned count is not min(k, candidates)')
        # 1. range, known, distinct
        assert bool((r[valid] < n_rel).all()), (p0, 'relation out of range')
        rc = r.clamp(min=0, max=n_rel - 1)
        assert not bool(km.gather(1, rc)[valid].any()), (p0, 'known relation returned')
        hits = torch.zeros((u.numel(), n_rel), dtype=torch.int32, device=dev)
        hits.scatter_add_(1, rc, valid.to(torch.int32))
        assert int(hits.max()) <= 1 if hits.numel() else True, (p0, 'duplicate relation')
        # 2. logits
        l64, tau = L.gather(1, rc), T.gather(1, rc)
        off = (s.double() - l64).abs()
        assert bool((off <= tau)[valid].all()), (p0, 'logit off fp64', float((off - tau)[valid].max()))
        # 3. order
        if k > 1:
            ok = (s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (r[:, :-1] < r[:, 1:]))
            assert bool(ok[valid[:, 1:]].all()), (p0, 'order')
        # 4. completeness of full rows
        full = nv == k
        if bool(full.any()):
            bound = l64[:, k - 1] + tau[:, k - 1]
            missing = ~km & (hits == 0)
            worst = (L - T).masked_fill(~missing, float('-inf')).amax(1)
            assert bool((worst <= bound)[full].all()), (p0, 'a better relation is missing', float((worst - bound)[full].max()))
