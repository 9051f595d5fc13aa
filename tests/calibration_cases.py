"""Seeded cases of the per-relation calibration shared by the host and the GPU tests (tests/calibration_spec.py holds the rules).

A case is a dict: z [n, dim], w [R, dim] fp32 on the CPU, train and given = (edge_index int64 [2, T], edge_type int64 [T]) in
shuffled order, relations int64 [Q] (query q works on side effect relations[q]; the ids run DOWN so that q != r).  The shapes
are the smallest at which the kernels can still go wrong: n = 2, 3 (one tile, nearly empty), 63, 64, 65 (the tile edge, a
second block), 130 (six tiles, three of them diagonal); dim = 4, 16, 20 (the widened width), 36 (crosses the 32-column staging
chunk); Q = 1 (more parts than tiles at small n), 5, 70 (above 64: one part per query).

The list KIND of a side effect cycles through
  mixed      random training pairs; given pairs in both directions, with repeats, self pairs and training pairs among them
  untrained  no training pair at all
  full       every cell trained (M = 0); the given pairs are all dropped
  nopos      training pairs, nothing given (status 4 in TIP.calibrate)
  separable  no training pairs; ONE positive, the cell with the top logit
  planted    training pairs; every other cell given with probability sigma(a* s + b*)
Q = 1 takes `mixed`.  The fit cases use `planted` and `separable` lists only (both classes present); the condition on them,
which the host test asserts, is that the fp64 spec reaches max |g| <= gtol within 16 evaluations from the prevalence start.
"""
import math

import torch

from drug_fit_cases import relations as decoder_rows
from fit_cases import embeddings

KINDS = ('mixed', 'untrained', 'full', 'nopos', 'separable', 'planted')
PLANTS = ((1.5, -3.0), (0.7, -2.0), (2.5, -4.0), (1.0, -1.0))            # (a*, b*) of the planted lists, cycled

# n, dim, Q
STATS_SHAPES = [(2, 16, 5), (3, 16, 1), (3, 4, 5), (63, 16, 5), (64, 20, 5), (65, 16, 1), (65, 36, 5), (65, 4, 70),
                (130, 16, 5), (130, 20, 1), (130, 36, 70)]
# name, n, dim, Q, kinds cycled over the queries
FIT_SHAPES = [('n65_d16_q5', 65, 16, 5, ('planted', 'planted', 'separable', 'planted', 'planted')),
              ('n64_d36_q1', 64, 36, 1, ('planted',)),
              ('n63_d20_q5', 63, 20, 5, ('planted', 'separable')),
              ('n130_d20_q70', 130, 20, 70, ('planted',)),
              ('n130_d4_q1', 130, 4, 1, ('separable',))]
L2 = 1e-6
GTOL = 1e-6
MAX_EVALUATIONS = 16


def _logits(z, w_r):
    n = z.shape[0]
    iu, iv = torch.triu_indices(n, n, 1)
    return iu, iv, ((z[iu].double() * w_r.double()) * z[iv].double()).sum(1)


def _random_cells(n, count, g):
    cells = n * (n - 1) // 2
    iu, iv = torch.triu_indices(n, n, 1)
    pick = torch.randperm(cells, generator=g)[:min(count, cells)]
    return list(zip(iu[pick].tolist(), iv[pick].tolist()))


def relation_lists(kind, z, w_r, seed, plant=PLANTS[0]):
    """(train, given): two lists of raw (u, v) of ONE side effect."""
    g = torch.Generator().manual_seed(seed)
    n = z.shape[0]
    iu, iv, s = _logits(z, w_r)
    cells = iu.numel()
    every = list(zip(iu.tolist(), iv.tolist()))
    n_train = max(1, cells // 12)
    if kind == 'mixed':
        train = _random_cells(n, n_train, g)
        fresh = _random_cells(n, max(2, cells // 20), g)
        given = fresh + [(v, u) for u, v in fresh[:3]] + fresh[:2] + [(0, 0), (n - 1, n - 1)] + train[:2] \
            + [(v, u) for u, v in train[2:3]]
        return train + [(v, u) for u, v in train[:4]], given
    if kind == 'untrained':
        return [], _random_cells(n, max(1, cells // 20), g)
    if kind == 'full':
        return every + [(v, u) for u, v in every[:3]], every[:2]
    if kind == 'nopos':
        return _random_cells(n, n_train, g), []
    if kind == 'separable':
        top = int(torch.argmax(s))
        return [], [every[top]]
    assert kind == 'planted'
    train = _random_cells(n, n_train, g)
    p = torch.sigmoid(plant[0] * s + plant[1])
    hit = torch.rand(cells, generator=g, dtype=torch.float64) < p
    taken = set(train)
    given = [c for c, h in zip(every, hit.tolist()) if h and c not in taken]
    if not given:                                                        # both classes present: the likeliest free cell
        order = torch.argsort(s, descending=True).tolist()
        free = next((every[i] for i in order if every[i] not in taken), None)
        given = [] if free is None else [free]
    return train, given


def _triples(lists, rels, seed):
    """Per-relation lists of (u, v) -> (edge_index [2, T], edge_type [T]) in shuffled order."""
    u, v, r = [], [], []
    for rel, lst in zip(rels, lists):
        for a, b in lst:
            u.append(a); v.append(b); r.append(rel)
    idx = torch.tensor([u, v], dtype=torch.int64).reshape(2, -1)
    et = torch.tensor(r, dtype=torch.int64)
    order = torch.randperm(et.numel(), generator=torch.Generator().manual_seed(seed))
    return idx[:, order], et[order]


def make_case(name, n, dim, n_q, kinds, seed, scale=1.0):
    z = embeddings(n, dim, 2100 + n + 7 * dim, scale)
    n_rel = n_q + 1                                                      # one side effect is never queried
    w = decoder_rows(n_rel, dim, 2200 + n_rel + 7 * dim)
    rel = torch.arange(n_rel - 1, n_rel - 1 - n_q, -1, dtype=torch.int64)
    trains, givens, used = [], [], []
    for q in range(n_q):
        kind = kinds[q % len(kinds)]
        tr, gv = relation_lists(kind, z, w[int(rel[q])], seed + 31 * q, PLANTS[q % len(PLANTS)])
        trains.append(tr); givens.append(gv); used.append(kind)
    # the side effect nobody queries has lists too: they must not leak into a query
    tr, gv = relation_lists('mixed', z, w[0], seed + 977)
    rels = rel.tolist() + [0]
    return {'name': name, 'z': z, 'w': w, 'relations': rel, 'kinds': used, 'train': _triples(trains + [tr], rels, seed + 1),
            'given': _triples(givens + [gv], rels, seed + 2)}


def stats_cases():
    return [make_case('n%d_d%d_q%d' % (n, dim, q), n, dim, q, ('mixed',) if q == 1 else KINDS, 3000 + 17 * i)
            for i, (n, dim, q) in enumerate(STATS_SHAPES)]


def fit_cases():
    return [make_case(name, n, dim, q, kinds, 4000 + 17 * i) for i, (name, n, dim, q, kinds) in enumerate(FIT_SHAPES)]


def prevalence_start(n_pos, n_neg):
    """(1, log((n_pos + .5) / (n_neg + .5))) per query, fp32 [Q, 2]."""
    b = torch.log((n_pos.double() + .5) / (n_neg.double() + .5))
    return torch.stack([torch.ones_like(b), b], 1).float()


def trial_points(n_pos, n_neg):
    """{'identity', 'prevalence', 'large'} -> ab fp32 [Q, 2]."""
    q = n_pos.numel()
    ident = torch.tensor([[1.0, 0.0]]).repeat(q, 1)
    large = torch.tensor([[40.0, -2.0], [-40.0, 2.0]]).repeat((q + 1) // 2, 1)[:q]
    return {'identity': ident, 'prevalence': prevalence_start(n_pos, n_neg), 'large': large}


def with_nan_row(z, row):
    z = z.clone()
    z[row] = math.nan
    return z


def with_inf_entry(z, row, col):
    z = z.clone()
    z[row, col] = math.inf
    return z
