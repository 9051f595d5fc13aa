"""fp64 specification of the screen rank (include/tipk.h section 4h): the filtered rank of target pairs among all unordered
pairs of a relation query, under the screen's total order (logit descending, key min*n+max ascending).

`spec_screen_rank` is the contract in exact fp64 with Python loops, for tiny graphs.  `dense_screen_rank` is the same on
whatever device z is on: per relation the dense fp64 logits L = (z * w_r) @ z.T, computed `row_chunk` rows at a time, the
candidates masked, and the number of better candidates of a target counted by comparing (L, key) pairs -- every distinct
logit gets its position among the distinct values, (that position, key) becomes one integer, and the count is a
`searchsorted` in the sorted candidates.  No tolerance anywhere: the device tests feed inputs for which fp32 and fp64 agree
exactly (`emulated_fp32_logits` shows it), so ranks and logits must match to the bit."""
import torch


def _lists(q_rel, tgt_ptr, n_tgt):
    q = [int(x) for x in torch.as_tensor(q_rel).tolist()]
    p = [min(max(int(x), 0), n_tgt) for x in torch.as_tensor(tgt_ptr).tolist()]
    return q, p


def _known_pairs(known, r, n):
    """{(a, b), a <= b} listed for relation r in either direction; keys outside [0, n^2) are ignored."""
    if known is None:
        return set()
    keys, ptr = known
    ptr = [int(x) for x in torch.as_tensor(ptr).tolist()]
    out = set()
    for k in torch.as_tensor(keys)[ptr[r]:ptr[r + 1]].tolist():
        if 0 <= k < n * n:
            out.add((min(k // n, k % n), max(k // n, k % n)))
    return out


def spec_screen_rank(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, known=None):
    """-> (rank int64 [T], logit float64 [T]); (0, NaN): not ranked."""
    z64, w64 = torch.as_tensor(z).double().cpu(), torch.as_tensor(w).double().cpu()
    n, n_rel = z64.shape[0], w64.shape[0]
    tu, tv = torch.as_tensor(tgt_u).tolist(), torch.as_tensor(tgt_v).tolist()
    q, p = _lists(q_rel, tgt_ptr, len(tu))
    rank = torch.zeros(len(tu), dtype=torch.int64)
    logit = torch.full((len(tu),), float('nan'), dtype=torch.float64)
    for qi, r in enumerate(q):
        if not 0 <= r < n_rel:
            continue
        listed = _known_pairs(known, r, n)
        L = {(a, b): float((z64[a] * w64[r] * z64[b]).sum()) for a in range(n) for b in range(a + 1, n)}
        cands = [(s, a * n + b) for (a, b), s in L.items() if (a, b) not in listed and s == s]
        for i in range(p[qi], p[qi + 1]):
            u, v = tu[i], tv[i]
            if not (0 <= u < n and 0 <= v < n) or u == v:
                continue
            a, b = min(u, v), max(u, v)
            s, key = L[(a, b)], a * n + b
            if s != s:
                continue
            rank[i] = 1 + sum(1 for cs, ck in cands if ck != key and (cs > s or (cs == s and ck < key)))
            logit[i] = s
    return rank, logit


def known_mask(known, r, n, device):
    """bool [n, n], symmetric: the known pairs of relation r; keys outside [0, n^2) are ignored."""
    m = torch.zeros((n, n), dtype=torch.bool, device=device)
    if known is None:
        return m
    keys, ptr = known
    ptr = [int(x) for x in torch.as_tensor(ptr).tolist()]
    ks = keys[ptr[r]:ptr[r + 1]].to(device=device, dtype=torch.int64)
    ks = ks[(ks >= 0) & (ks < n * n)]
    m[ks // n, ks % n] = True
    m[ks % n, ks // n] = True
    return m


def _relation_order(z64, wr, km, row_chunk):
    """(L [n, n] fp64, NaN mask, code [n, n] int64, sorted codes of the candidates): code = (position of the logit among the
    distinct logits, best first) * n^2 + key, so code order is the total order of the contract."""
    n = z64.shape[0]
    A = z64 * wr
    L = torch.cat([A[i:i + row_chunk] @ z64.t() for i in range(0, n, row_chunk)]) if n else A @ z64.t()
    nan = torch.isnan(L)
    vals, inv = torch.unique(torch.where(nan, torch.zeros_like(L), L), return_inverse=True)
    ar = torch.arange(n, device=z64.device)
    code = (vals.numel() - 1 - inv) * (n * n) + (ar[:, None] * n + ar[None, :])
    cand = (ar[None, :] > ar[:, None]) & ~km & ~nan
    return L, nan, code, torch.sort(code[cand]).values


def dense_screen_rank(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, known=None, row_chunk=1024):
    """The exact ranks on z's device -> (rank int64 [T], logit float64 [T]); (0, NaN): not ranked."""
    dev = z.device
    z64, w64 = z.double(), w.double().to(dev)
    n, n_rel = z64.shape[0], w64.shape[0]
    tu, tv = torch.as_tensor(tgt_u).to(dev).long(), torch.as_tensor(tgt_v).to(dev).long()
    q, p = _lists(q_rel, tgt_ptr, tu.numel())
    rank = torch.zeros(tu.numel(), dtype=torch.int64, device=dev)
    logit = torch.full((tu.numel(),), float('nan'), dtype=torch.float64, device=dev)
    cache = {}
    for qi, r in enumerate(q):
        tb, te = p[qi], p[qi + 1]
        if te <= tb or not 0 <= r < n_rel:
            continue
        if r not in cache:
            cache[r] = _relation_order(z64, w64[r], known_mask(known, r, n, dev), row_chunk)
        L, nan, code, cands = cache[r]
        u, v = tu[tb:te], tv[tb:te]
        ok = (u >= 0) & (u < n) & (v >= 0) & (v < n) & (u != v)
        a, b = torch.minimum(u, v).clamp(0, n - 1), torch.maximum(u, v).clamp(0, n - 1)
        ok &= ~nan[a, b]
        better = torch.searchsorted(cands, code[a, b].contiguous(), right=False)    # strictly better: never the target itself
        rank[tb:te] = torch.where(ok, better + 1, torch.zeros_like(better))
        logit[tb:te] = torch.where(ok, L[a, b], torch.full_like(L[a, b], float('nan')))
    return rank, logit


def on_exact_grid(z, w):
    """z in {-2, -1.75, ..., 2}, w in {-2, -1.5, ..., 2}, dim <= 256: every term z_a w z_b is a multiple of 2^-5 of size <= 8
    and every partial sum a multiple of 2^-5 of size <= 2 048 -- 17 significant bits, exact in fp32 in any order."""
    zf, wf = z[~torch.isnan(z)], w
    return bool(((zf * 4).frac() == 0).all()) and bool((zf.abs() <= 2).all()) and bool(((wf * 2).frac() == 0).all()) \
        and bool((wf.abs() <= 2).all()) and z.shape[1] <= 256


def emulated_fp32_logits(z, w, r, rows=None):
    """The kernel's fp32 arithmetic on the host: x_k = fl32(z[a,k] * w[r,k]), acc = fl32(x_k * z[b,k] + acc), k ascending (the
    fp64 product of two fp32 numbers is exact, so each step rounds as fmaf does but for double rounding) -> [rows, n] fp32."""
    z = z.float()
    za = z if rows is None else z[rows]
    acc = torch.zeros((za.shape[0], z.shape[0]), dtype=torch.float32)
    for k in range(z.shape[1]):
        x = (za[:, k] * w[r, k].float())
        acc = (x.double()[:, None] * z[:, k].double()[None, :] + acc.double()).float()
    return acc
