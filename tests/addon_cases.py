"""Inputs of the add-on burden tests (include/tipk.h section 4i), N = 70 drugs, built on the host from a seed.

Two recipes.
  mixed-sign   z, w = randn / dim**0.25 as in tests/test_gpu_regimen.py (tables: randn): both softplus branches; noisy-or
               saturates with long contexts, so a dropped context drug may hide inside the tolerance.
  unsaturated  every logit is negative and the mean level of a relation runs from about -0.5 to -6:
                   z = (0.5 + rand) / dim**0.25,  w[r] = -a_r * rand(dim),  a_r = (0.5 + 5.5 * rand) / (0.54 * sqrt(dim))
               (E[(0.5 + U)^2 U'] = 0.54, so the mean logit of r is -(0.5 + 5.5 * rand_r)); tables: s1, s2 =
               -(level_r / 2) * (0.5 + rand); weights 3 * rand.  `input_conditions` states what such a case must satisfy so
               that a dropped or doubled relation or context drug cannot hide: the median fp64 P_r lies in [0.02, 0.5] and
               the tolerance T_B is under a quarter of an average relation's contribution, T_B * R / B64 <= 0.25, for every
               task.  tests/test_host_addon.py asserts them for every unsaturated case below.
"""
import torch

from addon_spec import spec_addon_burden

N = 70
AGGS = ('max', 'noisy_or')

# (dim, R) of the DistMult lane and window edge cases (the relation window is 256 = 64 lanes x 4) and R of the table ones
DM_EDGES = [(16, 1), (16, 63), (16, 64), (16, 65), (16, 130), (8, 65), (20, 65), (4, 257), (16, 257)]
TABLE_EDGES = [1, 64, 65, 257]
# (R, dim, context length) the recipe was checked for beyond the edge cases: wide dims and the global route's shape
DM_WIDE = [(640, 64, 4), (320, 128, 4), (160, 256, 4)]


def mixed_dm(n_rel, dim, g, n=N):
    return ('distmult', torch.randn(n, dim, generator=g) / dim ** 0.25, torch.randn(n_rel, dim, generator=g) / dim ** 0.25)


def mixed_table(n_rel, g, n=N):
    wide = torch.randn(2, n, n_rel + 5, generator=g)                     # row stride n_rel + 5
    return ('table', wide[0, :, :n_rel], wide[1, :, :n_rel])


def unsat_dm(n_rel, dim, g, n=N):
    z = (0.5 + torch.rand(n, dim, generator=g)) / dim ** 0.25
    a = (0.5 + 5.5 * torch.rand(n_rel, 1, generator=g)) / (0.54 * dim ** 0.5)
    return ('distmult', z, -a * torch.rand(n_rel, dim, generator=g))


def unsat_table(n_rel, g, n=N):
    level = 0.5 + 5.5 * torch.rand(1, n_rel, generator=g)
    wide = torch.zeros(2, n, n_rel + 5)
    wide[:, :, :n_rel] = -(level / 2) * (0.5 + torch.rand(2, n, n_rel, generator=g))
    return ('table', wide[0, :, :n_rel], wide[1, :, :n_rel])


def weights_for(n_rel, g):
    return 3 * torch.rand(n_rel, generator=g)


def csr(lists):
    ptr = [0]
    for x in lists:
        ptr.append(ptr[-1] + len(x))
    return torch.tensor([v for x in lists for v in x], dtype=torch.int32), torch.tensor(ptr, dtype=torch.int64)


def random_queries(count, g, lo=1, hi=9, n_cand=60, n=N):
    """`count` contexts of distinct drugs in random order, lengths uniform in [lo, hi], and one list of `n_cand` distinct
    candidates per query (some of them members of the context) -> (contexts, candidate lists)."""
    ctx = [torch.randperm(n, generator=g)[:int(torch.randint(lo, hi + 1, (1,), generator=g))].tolist() for _ in range(count)]
    cands = [torch.randperm(n, generator=g)[:n_cand].tolist() for _ in range(count)]
    return ctx, cands


def known_for(ctx, cands, n_rel, g, n=N, share=0.3):
    """Random known relations for about half the (candidate, context drug) pairs -- listed in either direction -- plus keys
    of pairs that occur nowhere -> {(u, v): [relations]} for `pair_topk_spec.known_from_dict`."""
    d = {}
    for lst, cs in zip(ctx, cands):
        for c in cs[::3]:
            for i, s in enumerate(lst):
                if c != s and float(torch.rand(1, generator=g)) < 0.5:
                    rels = torch.nonzero(torch.rand(n_rel, generator=g) < share).reshape(-1).tolist()
                    d[(c, s) if i % 2 else (s, c)] = rels
    for u, v in torch.randint(0, n, (30, 2), generator=g).tolist():
        d.setdefault((u, v), [0, n_rel - 1])
    return d


def edge_case(kind, n_rel, dim, recipe, count=40):
    """The model, queries, weights and known dict of one lane / window edge case, from a seed fixed by its shape.  The
    unsaturated case of R = 1 has one-drug contexts: a single relation's level is one draw, and a noisy-or over nine drugs
    of a shallow one saturates (the median condition has no other relation to lean on)."""
    g = torch.Generator().manual_seed(1000 * n_rel + 10 * dim + (kind == 'table') + 2 * (recipe == 'unsat'))
    if kind == 'distmult':
        model = unsat_dm(n_rel, dim, g) if recipe == 'unsat' else mixed_dm(n_rel, dim, g)
    else:
        model = unsat_table(n_rel, g) if recipe == 'unsat' else mixed_table(n_rel, g)
    ctx, cands = random_queries(count, g, hi=1 if recipe == 'unsat' and n_rel == 1 else 9)
    return model, ctx, cands, weights_for(n_rel, g), known_for(ctx, cands, n_rel, g)


def input_conditions(model, ctx, cands, weights, aggregate, known=None):
    """(median fp64 P_r over the applicable tasks, largest T_B * R / B64 over them) of a case.  A task whose every triple
    is known has B64 = 0 and T_B = 0 -- it is held to 0 exactly -- and is left out of the ratio."""
    drugs, ptr = csr(ctx)
    cand, cptr = csr(cands)
    t = spec_addon_burden(model, drugs, ptr, cand, cptr, aggregate, weights, known)
    ok = t['applicable']
    assert bool((t['T_B'][ok & (t['B64'] == 0)] == 0).all())
    return float(t['P64'][ok].median()), float((t['T_B'] * t['R'] / t['B64'])[ok & (t['B64'] > 0)].max())
