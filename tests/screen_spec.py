"""fp64 specification of the DistMult screen (include/tipk.h section 4c) and the acceptance rule its results are held to.

`spec_screen` ranks every candidate of a query exactly (fp64 logit descending, key u*n+v ascending): the spec itself, for
tiny graphs.  `check_screen` holds a returned list to the acceptance rule against fp64, chunked, on whatever device z is on:
  tau = 1e-5 * (1 + sum_k |z_u z_v w_r|) of a pair;
  1. each returned pair is a candidate of the query (u < v for a relation query, u = the drug and v != u for a drug query),
     not a known pair in either direction, and no pair appears twice;
  2. each returned logit is within tau of the pair's fp64 logit;
  3. the list is ordered: descending logit, ties by ascending key;
  4. no unfiltered candidate missing from a full list has an fp64 logit above the k-th returned pair's fp64 logit + the
     two pairs' tau;
  5. padding (-inf, -1, -1) fills exactly the slots beyond the candidate count.
`exact_screen` is the spec again, vectorised and rounded to fp32, for inputs whose fp32 logits are exact: the contract's
order with no tolerance, NaN logits never returned, +-inf ranked as values.  `assert_screen_exact` compares with it bit for
bit (tests/screen_cases.py holds the inputs).
"""
import torch


def known_mask(keys, ptr, r, n, device):
    """bool [n, n], symmetric: the known pairs of relation r (keys u*n+v sorted inside each relation; ptr [n_rel + 1])."""
    if keys is None:
        return None
    ptr = [int(x) for x in torch.as_tensor(ptr).tolist()]
    ks = keys[ptr[r]:ptr[r + 1]].to(device=device, dtype=torch.int64)
    m = torch.zeros((n, n), dtype=torch.bool, device=device)
    a, b = ks // n, ks % n
    m[a, b] = True
    m[b, a] = True
    return m


def keys_from_pairs(pairs_by_rel, n):
    """[(u, v), ...] per relation -> (keys int64 sorted inside each relation, ptr int64 [n_rel + 1]) on the host."""
    keys, ptr = [], [0]
    for pairs in pairs_by_rel:
        ks = sorted(int(u) * n + int(v) for u, v in pairs)
        keys += ks
        ptr.append(len(keys))
    return torch.tensor(keys, dtype=torch.int64), torch.tensor(ptr, dtype=torch.int64)


def spec_screen(z, w, queries, k, known=None):
    """The exact fp64 screen -> (logit float64 [Q, k], u int64 [Q, k], v int64 [Q, k]), padding (-inf, -1, -1)."""
    z64, w64 = z.double().cpu(), w.double().cpu()
    n = z64.shape[0]
    qs = torch.as_tensor(queries).reshape(-1, 2).tolist()
    out_s = torch.full((len(qs), k), float('-inf'), dtype=torch.float64)
    out_u = torch.full((len(qs), k), -1, dtype=torch.int64)
    out_v = torch.full((len(qs), k), -1, dtype=torch.int64)
    for i, (r, du) in enumerate(qs):
        km = known_mask(known[0], known[1], r, n, 'cpu') if known is not None else None
        cands = []
        for u in (range(n) if du < 0 else [du]):
            for v in (range(u + 1, n) if du < 0 else range(n)):
                if v == u or (km is not None and bool(km[u, v])):
                    continue
                cands.append((float((z64[u] * z64[v] * w64[r]).sum()), u * n + v, u, v))
        cands.sort(key=lambda c: (-c[0], c[1]))
        for j, (s, _, u, v) in enumerate(cands[:k]):
            out_s[i, j], out_u[i, j], out_v[i, j] = s, u, v
    return out_s, out_u, out_v


def _known_row(keys, ptr, r, n, du, device):
    """bool [n]: the partners v of drug du with du*n+v or v*n+du a key of relation r (no n x n mask: n may be 46 340)."""
    m = torch.zeros(n, dtype=torch.bool, device=device)
    if keys is None:
        return m
    ptr = [int(x) for x in torch.as_tensor(ptr).tolist()]
    ks = keys[ptr[r]:ptr[r + 1]].to(device=device, dtype=torch.int64)
    a, b = ks // n, ks % n
    m[b[a == du]] = True
    m[a[b == du]] = True
    return m


def _first_k(logits32, cand, k):
    """The first k of a stable descending sort over the candidates in ascending position -> (score fp32 [<= k], position)."""
    pos = cand.nonzero().flatten()
    top = torch.sort(logits32[pos], descending=True, stable=True)
    return top.values[:k], pos[top.indices[:k]]


def exact_screen(z, w, queries, k, known=None):
    """The screen with NO tolerance, vectorised, on z's device -> (score float32 [Q, k], u int32 [Q, k], v int32 [Q, k]),
    padding (-inf, -1, -1).  The logits are fp64, (z * w_r) @ z.T, rounded to fp32: for inputs whose fp32 logits equal the
    fp64 ones (tests/test_host_screen_cases.py shows it for every case of tests/screen_cases.py) the rounding changes nothing,
    and a sum beyond the fp32 range becomes +-inf as it does in the kernel.  Candidates: u < v for a relation query, v != u
    for a drug query; known pairs in either direction and NaN logits are masked; the answer is the first k of a stable
    descending sort over the candidates laid out in ascending key u*n+v.  A relation query forms its relation's n x n
    matrix, once per distinct relation; a drug query forms its own row only, so it runs at n = 46 340."""
    dev = z.device
    z64, w64 = z.double(), w.double().to(dev)
    n = z64.shape[0]
    qs = [tuple(q) for q in torch.as_tensor(queries).reshape(-1, 2).tolist()]
    out_s = torch.full((len(qs), k), float('-inf'), dtype=torch.float32, device=dev)
    out_u = torch.full((len(qs), k), -1, dtype=torch.int32, device=dev)
    out_v = torch.full((len(qs), k), -1, dtype=torch.int32, device=dev)
    rows_of = {}
    for i, q in enumerate(qs):
        rows_of.setdefault(q, []).append(i)
    ar = torch.arange(n, device=dev)
    for (r, du), rows in rows_of.items():
        if du < 0:
            L = ((z64 * w64[r]) @ z64.t()).float()
            cand = (ar[None, :] > ar[:, None]) & ~torch.isnan(L)
            if known is not None:
                cand &= ~known_mask(known[0], known[1], r, n, dev)
            s, key = _first_k(L.flatten(), cand.flatten(), k)                # row-major positions ARE the keys u*n+v
            u, v = key // n, key % n
        else:
            L = ((z64[du] * w64[r]) @ z64.t()).float()
            cand = (ar != du) & ~torch.isnan(L)
            if known is not None:
                cand &= ~_known_row(known[0], known[1], r, n, du, dev)
            s, v = _first_k(L, cand, k)
            u = torch.full_like(v, du)
        rows = torch.tensor(rows, device=dev)
        out_s[rows, :s.numel()] = s
        out_u[rows, :s.numel()] = u.int()
        out_v[rows, :s.numel()] = v.int()
    return out_s, out_u, out_v


def assert_screen_exact(got, want):
    """got == want, all three tensors, bit for bit (`torch.equal`: no tolerance); reports the first differing (query, slot)."""
    names = ('score', 'u', 'v')
    for g, x, name in zip(got, want, names):
        assert g.shape == x.shape and g.dtype == x.dtype, (name, g.shape, x.shape, g.dtype, x.dtype)
    if all(torch.equal(g, x.to(g.device)) for g, x in zip(got, want)):
        return
    diff = torch.zeros(got[0].shape, dtype=torch.bool, device=got[0].device)
    for g, x in zip(got, want):
        x = x.to(g.device)
        diff |= (g != x) | (g.isnan() if g.is_floating_point() else torch.zeros_like(diff))
    at = diff.flatten().nonzero().flatten()
    q, j = divmod(int(at[0]), got[0].shape[1])
    raise AssertionError('screen differs from the exact order in %d slots, first at query %d slot %d: got (%r, %d, %d), want '
                         '(%r, %d, %d)' % (at.numel(), q, j, float(got[0][q, j]), int(got[1][q, j]), int(got[2][q, j]),
                                           float(want[0][q, j]), int(want[1][q, j]), int(want[2][q, j])))


def _pair64(z64, w64, r, u, v):
    t = z64[u] * z64[v] * w64[r]
    return t.sum(1), t.abs().sum(1)


def check_screen(z, w, queries, k, got, known=None, row_chunk=2048):
    """Assert the acceptance rule for got = (logits [Q, k], u [Q, k], v [Q, k]) (any device); known = (keys, ptr) or None.
    The fp64 reference runs on z's device, `row_chunk` rows of the logit matrix at a time."""
    dev = z.device
    z64, w64 = z.double(), w.double().to(dev)
    n = z64.shape[0]
    qs = torch.as_tensor(queries).reshape(-1, 2).tolist()
    s_all, u_all, v_all = (t.to(dev) for t in got)
    assert s_all.shape == (len(qs), k) and u_all.shape == (len(qs), k) and v_all.shape == (len(qs), k)
    zabs = z64.abs()
    cols = torch.arange(n, device=dev)
    for i, (r, du) in enumerate(qs):
        km = known_mask(known[0], known[1], r, n, dev) if known is not None else None
        s, u, v = s_all[i], u_all[i].long(), v_all[i].long()
        nv = int((u >= 0).sum())
        assert bool((u[:nv] >= 0).all()) and bool((u[nv:] == -1).all()) and bool((v[nv:] == -1).all()), (i, 'padding')
        assert bool(torch.isneginf(s[nv:]).all()), (i, 'padding score')
        su, uu, vu = s[:nv], u[:nv], v[:nv]
        # 1. valid, unfiltered, distinct
        assert bool((vu >= 0).all()) and bool((vu < n).all()) and bool((uu < n).all()), (i, 'range')
        if du < 0:
            assert bool((uu < vu).all()), (i, 'relation pairs are u < v')
        else:
            assert bool((uu == du).all()) and bool((vu != du).all()), (i, 'drug pairs are (drug, v != drug)')
        if km is not None and nv:
            assert not bool(km[uu, vu].any()), (i, 'known pair returned')
        key = uu * n + vu
        assert torch.unique(key).numel() == nv, (i, 'duplicate pair')
        # 2. logits
        l64, a64 = _pair64(z64, w64, r, uu, vu)
        tau = 1e-5 * (1.0 + a64)
        assert bool(((su.double() - l64).abs() <= tau).all()), (i, 'logit off fp64', float((su.double() - l64).abs().max()))
        # 3. order
        if nv > 1:
            ok = (su[:-1] > su[1:]) | ((su[:-1] == su[1:]) & (key[:-1] < key[1:]))
            assert bool(ok.all()), (i, 'order')
        # 4. / 5. completeness and padding
        n_cand = 0
        bound = None if nv < k else float(l64[-1] + tau[-1])
        rows_all = torch.arange(n, device=dev) if du < 0 else torch.tensor([du], device=dev)
        for a in range(0, rows_all.numel(), row_chunk):
            rows = rows_all[a:a + row_chunk]
            A = z64[rows] * w64[r]
            cand = (cols[None, :] > rows[:, None]) if du < 0 else (cols[None, :] != rows[:, None])
            if km is not None:
                cand &= ~km[rows]
            n_cand += int(cand.sum())
            if bound is None:
                continue
            missing = cand & ~torch.isin(rows[:, None] * n + cols[None, :], key)
            if not bool(missing.any()):
                continue
            L = A @ z64.t()
            T = 1e-5 * (1.0 + (A.abs() @ zabs.t()))
            worst = float((L - T)[missing].max())
            assert worst <= bound, (i, 'a better candidate is missing', worst, bound)
        assert nv == min(k, n_cand), (i, 'returned %d of %d candidates (k = %d)' % (nv, n_cand, k))
