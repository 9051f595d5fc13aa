"""The seeded inputs of the partner sum tests (include/tipk.h section 4l), built on the host so that
tests/test_host_partner_sum.py can run the fp64 spec on them without a device.  A case is a dict of CPU tensors: model
(tests/partner_rank_spec.py), q_drug [Q], rel_ids [S] or None, partner_w [n] or None, known (keys, ptr) or None."""
import torch

from partner_rank_cases import biosnap_weights, known_from_dict, model_of, random_known

REL_BLOCK = 4                                   # columns per work item of the kernel (tipk_partner_sum.hip PS_RB)
R = 7
SMALL_N = (1, 2, 63, 64, 65, 130)
SMALL_DIM = (4, 16, 20, 128)
SEL_COUNTS = tuple(range(1, 2 * REL_BLOCK + 2)) + (63, 64, 65, 257)
QUERY_COUNTS = (0, 1, 17, 300)
ROUTES = ((700, 16), (700, 32), (2600, 16))     # (n_nodes, dim) of partner_rank_cases.ROUTES; the last cannot take the LDS route
KINDS = ('distmult', 'table')


def symmetric(d):
    """{relation: [(u, v), ...]} with every pair in both directions."""
    return {r: list(uv) + [(v, u) for u, v in uv] for r, uv in d.items()}


def queries(n, count, g, out_of_range=True):
    """`count` random drugs below n; from 3 entries on the first repeats the second, and with out_of_range two of them are
    -1 and n."""
    q = torch.randint(0, n, (count,), generator=g)
    if count >= 3:
        q[0] = q[1]
    if out_of_range and count >= 5:
        q[2], q[4] = -1, n
    return q


def columns(n_rel, mode, g, count=None):
    """rel_ids: None ('all'), a permuted subset ('subset'), or `count` ids with repeats and, from 4 on, one id out of range
    ('repeats')."""
    if mode == 'all':
        return None
    if mode == 'subset':
        return torch.randperm(n_rel, generator=g)[:max(1, (2 * n_rel) // 3)]
    count = n_rel + 3 if count is None else count
    rel = torch.randint(0, n_rel, (count,), generator=g)
    if count >= 2:
        rel[-1] = rel[0]
    if count >= 4:
        rel[2] = n_rel if count % 2 else -1
    return rel


def weights(n, mode, g):
    """partner_w: None ('none'), random in [0, 2) with about a third zeros ('zeros'), all zero ('all_zero')."""
    if mode == 'none':
        return None
    if mode == 'all_zero':
        return torch.zeros(n)
    w = 2 * torch.rand(n, generator=g)
    w[torch.rand(n, generator=g) < 0.33] = 0.0
    return w


def small_case(kind, n, dim, col_mode='all', w_mode='zeros', n_q=17, n_rel=R):
    """Random queries (repeated and out-of-range drugs), symmetric random known lists over about a sixth of all pairs."""
    g = torch.Generator().manual_seed(977 * n + dim + 13 * len(col_mode) + (5 if kind == 'table' else 0) + n_rel)
    model = model_of(kind, n, n_rel, dim, g, pad=3)
    d = symmetric(random_known(n, n_rel, g, per_rel=max(1, n * n // 12), mirror=0.0)) if n >= 2 else {}
    return dict(model=model, q_drug=queries(n, n_q, g), rel_ids=columns(n_rel, col_mode, g), partner_w=weights(n, w_mode, g),
                known=known_from_dict(d, n, n_rel))


def sel_case(kind, n_sel):
    """n = 65, 300 relations, exactly n_sel columns (repeats; one id out of range from 4 columns on)."""
    g = torch.Generator().manual_seed(31 * n_sel + (1 if kind == 'table' else 0))
    n, n_rel = 65, 300
    model = model_of(kind, n, n_rel, 16, g)
    d = symmetric(random_known(n, n_rel, g, per_rel=40, mirror=0.0))
    return dict(model=model, q_drug=queries(n, 9, g), rel_ids=columns(n_rel, 'repeats', g, count=n_sel),
                partner_w=weights(n, 'zeros', g), known=known_from_dict(d, n, n_rel))


def known_case(kind, how, n=130):
    """The known filter's corners, 5 relations, all drugs queried (drug 3 twice):
      'none'       no lists
      'symmetric'  random pairs in both directions
      'one_way'    random pairs listed once, as (min, max) for even relations and (max, min) for odd ones: only the listed
                   direction may be dropped
      'every'      relation 1 lists every partner of drug 5 (forward): that cell has no candidates; relation 2 lists every
                   partner of drug 6 in reverse only: that cell keeps all of them
      'self'       self keys u*n+u among random pairs: they change nothing
    """
    g = torch.Generator().manual_seed(n + len(how) + (1 if kind == 'table' else 0))
    n_rel = 5
    model = model_of(kind, n, n_rel, 16, g)
    base = random_known(n, n_rel, g, per_rel=n * n // 8, mirror=0.0)
    if how == 'none':
        known = None
    elif how == 'symmetric':
        known = known_from_dict(symmetric(base), n, n_rel)
    elif how == 'one_way':
        d = {r: [((min(u, v), max(u, v)) if r % 2 == 0 else (max(u, v), min(u, v))) for u, v in uv] for r, uv in base.items()}
        known = known_from_dict(d, n, n_rel)
    elif how == 'every':
        d = dict(base)
        d[1] = [(u, v) for u, v in d[1] if u != 5] + [(5, c) for c in range(n) if c != 5]
        d[2] = [(u, v) for u, v in d[2] if 6 not in (u, v)] + [(c, 6) for c in range(n) if c != 6]
        known = known_from_dict(d, n, n_rel)
    else:
        assert how == 'self'
        d = {r: uv + [(u, u) for u in range(0, n, 3)] for r, uv in base.items()}
        known = known_from_dict(d, n, n_rel)
    q = torch.cat([torch.arange(n), torch.tensor([3])])
    return dict(model=model, q_drug=q, rel_ids=None, partner_w=None, known=known)


def routes_case(n, dim):
    """40 queried drugs over 3 relations; about a third of every queried drug's partners is recorded."""
    g = torch.Generator().manual_seed(17 * n + dim)
    n_rel = 3
    model = model_of('distmult', n, n_rel, dim, g)
    q = queries(n, 40, g)
    keys = []
    for r in range(n_rel):
        us = torch.unique(q[(q >= 0) & (q < n)])
        listed = torch.rand(us.numel(), n, generator=g) < 0.33
        u = us[:, None].expand(-1, n)
        c = torch.arange(n)[None, :].expand(us.numel(), -1)
        keys.append(torch.unique((u * n + c)[listed & (c != u)]))
    kptr = torch.zeros(n_rel + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(torch.tensor([k.numel() for k in keys]), 0)
    return dict(model=model, q_drug=q, rel_ids=None, partner_w=weights(n, 'zeros', g), known=(torch.cat(keys), kptr))


def biosnap_case(kind, n_q=64, n=645, n_rel=1097, per_rel=4200):
    """BioSNAP size: 645 drugs, 1 097 relations, width 16, lists of BioSNAP density (4.6 M directed training keys over
    1 097 relations), 64 queried drugs."""
    g = torch.Generator().manual_seed(1097 + (1 if kind == 'table' else 0))
    model = biosnap_weights(n, n_rel) if kind == 'distmult' else model_of('table', n, n_rel, 0, g)
    uv = torch.randint(0, n, (n_rel, per_rel // 2, 2), generator=g)
    rel = torch.arange(n_rel)[:, None].expand(-1, per_rel // 2)
    ok = uv[..., 0] != uv[..., 1]
    comb = torch.cat([(rel * n * n + uv[..., 0] * n + uv[..., 1])[ok], (rel * n * n + uv[..., 1] * n + uv[..., 0])[ok]])
    comb = torch.unique(comb)
    kptr = torch.zeros(n_rel + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(torch.bincount(torch.div(comb, n * n, rounding_mode='floor'), minlength=n_rel), 0)
    q = torch.randperm(n, generator=g)[:n_q]
    return dict(model=model, q_drug=q, rel_ids=None, partner_w=None, known=(comb % (n * n), kptr))
