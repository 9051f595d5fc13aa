"""The seeded inputs of the partner rank tests (include/tipk.h section 4g), built on the host so that
tests/test_host_partner_rank.py can hold every random-input case of tests/test_gpu_partner_rank.py to the degeneracy cap of
tests/partner_rank_spec.py without a device.  A case is (model, q_rel [Q], q_drug [Q], tgt_ptr [Q + 1], tgt_node [T], known or
None), all CPU tensors; `known` is the screen's relation-major (keys, ptr)."""
import torch

R = 6
SMALL_N = (2, 63, 64, 65, 130)
SMALL_DIM = (4, 16, 128)
COUNTS = (0, 1, 63, 64, 65, 130)
COUNTS_N = 200
ROUTES = ((700, 16, 400), (700, 32, 400), (2600, 16, 150))     # (n_nodes, dim, queries); the last cannot take the LDS route


def model_of(kind, n, n_rel, dim, g, pad=0):
    if kind == 'distmult':
        return ('distmult', torch.randn(n, dim, generator=g) / dim ** 0.25, torch.randn(n_rel, dim, generator=g) / dim ** 0.25)
    wide = torch.randn(2, n_rel, n + pad, generator=g)                    # row stride n + pad
    return ('table', wide[0, :, :n], wide[1, :, :n])


def csr(lists):
    ptr = [0]
    for t in lists:
        ptr.append(ptr[-1] + len(t))
    return torch.tensor(ptr, dtype=torch.int64), torch.tensor([c for t in lists for c in t], dtype=torch.int32)


def known_from_dict(d, n, n_rel):
    """{relation: [(u, v), ...]} (directed, any order, repeats collapse) -> (keys, ptr) on the host."""
    keys, ptr = [], [0]
    for r in range(n_rel):
        keys += sorted({u * n + v for u, v in d.get(r, ())})
        ptr.append(len(keys))
    return torch.tensor(keys, dtype=torch.int64), torch.tensor(ptr, dtype=torch.int64)


def random_known(n, n_rel, g, per_rel, mirror=0.5):
    """per_rel random directed pairs u != v below n per relation; a share `mirror` of them is listed in both directions."""
    d = {}
    if n < 2:
        return d
    for r in range(n_rel):
        uv = torch.randint(0, n, (per_rel, 2), generator=g)
        both = torch.rand(per_rel, generator=g) < mirror
        d[r] = [(u, v) for (u, v) in uv.tolist() if u != v]
        d[r] += [(v, u) for (u, v), b in zip(uv.tolist(), both.tolist()) if b and u != v]
    return d


def small_case(kind, n, dim=0):
    """40 queries -- (2, 0), (2, 1), (2, 0) again, (5, n - 1) whose drug is in no key (n > 2), then random ones -- with 0..6
    random targets each (repeats and target == drug allowed) and random known lists over the drugs below n - 1."""
    g = torch.Generator().manual_seed(1013 * n + dim + (7 if kind == 'table' else 0))
    model = model_of(kind, n, R, dim, g, pad=5)
    q = torch.cat([torch.tensor([[2, 0], [2, 1], [2, 0], [5, n - 1]]),
                   torch.stack([torch.randint(0, R, (36,), generator=g), torch.randint(0, n, (36,), generator=g)], 1)])
    d = random_known(n - 1, R, g, per_rel=max(1, n * n // 8)) if n > 2 else {0: [(0, 1)]}
    lists = [torch.randint(0, n, (int(c),), generator=g).tolist() for c in torch.randint(0, 7, (40,), generator=g)]
    lists[0] = lists[0] + [1, n - 1]
    lists[2] = list(lists[0])
    lists[3] = lists[3] + [0]
    tgt_ptr, tgt_node = csr(lists)
    return model, q[:, 0].contiguous(), q[:, 1].contiguous(), tgt_ptr, tgt_node, known_from_dict(d, n, R)


def counts_case(kind):
    """One query per target count in COUNTS (random targets, repeats allowed), then every other drug once for a query of
    relation R - 1, whose block is empty: its ranks are a permutation of 1..n-1.  n = 200."""
    n = COUNTS_N
    g = torch.Generator().manual_seed(4242 + (1 if kind == 'table' else 0))
    model = model_of(kind, n, R, 16, g)
    q_rel = torch.randint(0, R - 1, (len(COUNTS) + 1,), generator=g)
    q_drug = torch.randint(0, n, (len(COUNTS) + 1,), generator=g)
    q_rel[-1], q_drug[-1] = R - 1, 11
    lists = [torch.randint(0, n, (c,), generator=g).tolist() for c in COUNTS]
    lists[3][5] = lists[3][40]                                            # a repeated target
    lists.append([c for c in torch.randperm(n, generator=g).tolist() if c != 11])
    d = random_known(n, R - 1, g, per_rel=n * n // 6)
    tgt_ptr, tgt_node = csr(lists)
    return model, q_rel, q_drug, tgt_ptr, tgt_node, known_from_dict(d, n, R)


def corner_case(kind, n):
    """The known filter's corners, 4 relations (n = 4 500 spans three bitmap windows of 2 048 drugs).  `some` is a random half
    of the drugs plus the window edges.  Queries, in order:
      0 (0, 0)      `some` listed forward, among them the first key of the first relation, 0*n+1
      1 (0, 9)      `some` listed only in reverse, as c*n+9
      2 (1, 5)      every partner listed forward
      3 (1, 6)      every partner listed in reverse only
      4 (2, 7)      relation 2 has an empty block
      5 (3, n - 1)  `some` listed forward, among them the last key of the last relation, (n-1)*n + n-2
      6 (3, 12)     a relation with keys, none of drug 12
      7 (0, 20)     `some` listed in both directions
    Every query has the same targets, listed and free ones on both sides of the window edges.  -> (case, some)."""
    g = torch.Generator().manual_seed(n + (1 if kind == 'table' else 0))
    n_rel = 4
    model = model_of(kind, n, n_rel, 8, g)
    edge = {1, 2047, 2048, n - 2} & set(range(n))
    some = sorted(set(torch.randint(0, n, (n // 2,), generator=g).tolist()) | edge)
    skip = {0, 9, 5, 6, 7, n - 1, 12, 20}
    some = [c for c in some if c not in skip]
    every = lambda u: [c for c in range(n) if c != u]
    d = {0: [(0, c) for c in some] + [(c, 9) for c in some] + [(20, c) for c in some] + [(c, 20) for c in some],
         1: [(5, c) for c in every(5)] + [(c, 6) for c in every(6)],
         3: [(n - 1, c) for c in some]}
    q_rel = torch.tensor([0, 0, 1, 1, 2, 3, 3, 0])
    q_drug = torch.tensor([0, 9, 5, 6, 7, n - 1, 12, 20])
    free = sorted(set(range(n)) - set(some) - skip)
    both = sorted(edge) + some[::max(1, len(some) // 20)][:20] + free[::max(1, len(free) // 20)][:20]
    tgt_ptr, tgt_node = csr([both] * q_rel.numel())
    return (model, q_rel, q_drug, tgt_ptr, tgt_node, known_from_dict(d, n, n_rel)), some


def routes_case(n, dim, n_q):
    """Random queries over 3 relations with 0..9 random targets each; every query's drug has about half of all drugs listed,
    a third of them forward only, a third in reverse only, a third in both directions."""
    g = torch.Generator().manual_seed(31 * n + dim)
    n_rel = 3
    model = model_of('distmult', n, n_rel, dim, g)
    q_rel = torch.randint(0, n_rel, (n_q,), generator=g)
    q_drug = torch.randint(0, n, (n_q,), generator=g)
    count = torch.randint(0, 10, (n_q,), generator=g)
    tgt_ptr = torch.zeros(n_q + 1, dtype=torch.int64)
    tgt_ptr[1:] = torch.cumsum(count, 0)
    tgt_node = torch.randint(0, n, (int(tgt_ptr[-1]),), generator=g).to(torch.int32)
    keys = []
    for r in range(n_rel):
        us = torch.unique(q_drug[q_rel == r])
        how = torch.randint(0, 6, (us.numel(), n), generator=g)            # 0: forward, 1: reverse, 2: both, 3..5: free
        u = us[:, None].expand(-1, n)
        c = torch.arange(n)[None, :].expand(us.numel(), -1)
        ok = c != u
        fwd, rev = ok & ((how == 0) | (how == 2)), ok & ((how == 1) | (how == 2))
        keys.append(torch.unique(torch.cat([(u * n + c)[fwd], (c * n + u)[rev]])))
    kptr = torch.zeros(n_rel + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(torch.tensor([k.numel() for k in keys]), 0)
    return model, q_rel, q_drug, tgt_ptr, tgt_node, (torch.cat(keys), kptr)


def screen_case(n, one_direction=False):
    """24 DistMult queries (dim 16, 4 relations) whose targets are NOT on the known list: up to 12 random free partners each.
    one_direction: every known pair is listed once, as (min, max) for even relations and as (max, min) for odd ones."""
    g = torch.Generator().manual_seed(77 * n + int(one_direction))
    n_rel = 4
    model = model_of('distmult', n, n_rel, 16, g)
    d = random_known(n, n_rel, g, per_rel=n * n // 5, mirror=0.5)
    if one_direction:
        d = {r: [((min(u, v), max(u, v)) if r % 2 == 0 else (max(u, v), min(u, v))) for u, v in uv] for r, uv in d.items()}
    q_rel = torch.randint(0, n_rel, (24,), generator=g)
    q_drug = torch.randint(0, n, (24,), generator=g)
    lists = []
    for r, u in zip(q_rel.tolist(), q_drug.tolist()):
        listed = {v for (a, v) in d[r] if a == u} | {a for (a, v) in d[r] if v == u}
        free = [c for c in torch.randperm(n, generator=g).tolist() if c != u and c not in listed]
        lists.append(free[:12])
    tgt_ptr, tgt_node = csr(lists)
    return model, q_rel, q_drug, tgt_ptr, tgt_node, known_from_dict(d, n, n_rel)


def biosnap_weights(n, n_rel, dim=16):
    g = torch.Generator().manual_seed(645)
    return ('distmult', torch.randn(n, dim, generator=g) / 2, torch.randn(n_rel, dim, generator=g) / 2)
