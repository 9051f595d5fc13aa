"""Inputs of the combination-burden tests (include/tipk.h section 4n), N = 70 drugs, built on the host from a seed.

The models are the two recipes of tests/addon_cases.py, unchanged (`mixed_dm` / `mixed_table`: both softplus branches,
noisy-or saturates in large regimens; `unsat_dm` / `unsat_table`: every logit negative, relation levels from -0.5 to -6).
A query is (fixed, slots) as in tests/combo_spec.py.
  mixed queries        0 to 9 fixed drugs, 0 to 3 slots of 1 to 4 alternatives, with -1 alternatives, alternatives that repeat
                       across slots and alternatives that are fixed drugs (NaN combinations) mixed in.
  unsaturated queries  1 to 3 slots of 1 to 3 alternatives and as many fixed drugs as make the regimen 2 to 4 drugs, all
                       distinct, no -1: with `unsat_*` as they are, whole regimens of 2 to 4 drugs keep the median P_r inside
                       [0.02, 0.5] (6 drugs do not), so a dropped or doubled pair, level or relation cannot hide inside the
                       tolerance.  `input_conditions` states the two conditions; tests/test_host_combo.py asserts them for
                       every unsaturated case below, both aggregates, with and without the known list.
"""
import torch

import addon_cases as ac
from addon_cases import AGGS, DM_EDGES, N, TABLE_EDGES, weights_for      # noqa: F401  (the tests read them from here)
from combo_spec import spec_combo_burden


def mixed_queries(count, g, n=N):
    out = []
    for _ in range(count):
        perm = torch.randperm(n, generator=g).tolist()
        m, S = int(torch.randint(0, 10, (1,), generator=g)), int(torch.randint(0, 4, (1,), generator=g))
        fixed, rest = perm[:m], perm[m:]
        slots = []
        for _ in range(S):
            a = int(torch.randint(1, 5, (1,), generator=g))
            slot, rest = rest[:a], rest[a:]
            roll = float(torch.rand(1, generator=g))
            if roll < 0.25:
                slot[int(torch.randint(0, a, (1,), generator=g))] = -1
            elif roll < 0.4 and slots:
                slot[0] = slots[0][0]                                     # the same drug in two slots (it may be -1: legal)
            elif roll < 0.55 and m:
                slot[-1] = fixed[0]                                       # an alternative that is a fixed drug
            slots.append(slot)
        out.append((fixed, slots))
    return out


def unsat_queries(count, g, n=N, drugs=(2, 4)):
    out = []
    for _ in range(count):
        perm = torch.randperm(n, generator=g).tolist()
        total = int(torch.randint(drugs[0], drugs[1] + 1, (1,), generator=g))
        S = int(torch.randint(1, min(3, total) + 1, (1,), generator=g))
        fixed, rest = perm[:total - S], perm[total - S:]
        slots = []
        for _ in range(S):
            a = int(torch.randint(1, 4, (1,), generator=g))
            slots.append(rest[:a])
            rest = rest[a:]
        out.append((fixed, slots))
    return out


def query_drugs(query):
    fixed, slots = query
    return sorted(set(fixed) | set(d for s in slots for d in s if d >= 0))


def known_for(queries, n_rel, g, n=N, share=0.3):
    """Random known relations for about half the pairs of every query's drugs -- listed in either direction --, one pair per
    third query with EVERY relation known, and keys of pairs that occur nowhere -> {(u, v): [relations]} for
    `pair_topk_spec.known_from_dict`."""
    d = {}
    for qi, q in enumerate(queries):
        drugs = query_drugs(q)
        for i, a in enumerate(drugs):
            for j, b in enumerate(drugs[i + 1:]):
                if float(torch.rand(1, generator=g)) < 0.5:
                    rels = torch.nonzero(torch.rand(n_rel, generator=g) < share).reshape(-1).tolist()
                    d[(a, b) if (i + j) % 2 else (b, a)] = rels
        if qi % 3 == 0 and len(drugs) >= 2:
            d[(drugs[1], drugs[0])] = list(range(n_rel))
    for u, v in torch.randint(0, n, (30, 2), generator=g).tolist():
        d.setdefault((u, v), [0, n_rel - 1])
    return d


def edge_case(kind, n_rel, dim, recipe, count=24):
    """The model, queries, weights and known dict of one lane / window edge case, from a seed fixed by its shape.  The
    unsaturated case of R = 1 keeps to regimens of two drugs: a single relation's level is one draw, and a noisy-or over
    the six pairs of four drugs of a shallow one leaves the median condition (it has no other relation to lean on)."""
    g = torch.Generator().manual_seed(7000 + 1000 * n_rel + 10 * dim + (kind == 'table') + 2 * (recipe == 'unsat'))
    if kind == 'distmult':
        model = ac.unsat_dm(n_rel, dim, g) if recipe == 'unsat' else ac.mixed_dm(n_rel, dim, g)
    else:
        model = ac.unsat_table(n_rel, g) if recipe == 'unsat' else ac.mixed_table(n_rel, g)
    queries = unsat_queries(count, g, drugs=(2, 2 if n_rel == 1 else 4)) if recipe == 'unsat' else mixed_queries(count, g)
    return model, queries, weights_for(n_rel, g), known_for(queries, n_rel, g)


def input_conditions(model, queries, weights, aggregate, limits, known=None):
    """(median fp64 P_r over the applicable combinations, largest T_B * R / B64 over them) of a case.  A combination whose
    every triple is known has B64 = 0 and T_B = 0 -- it is held to 0 exactly -- and is left out of the ratio."""
    t = spec_combo_burden(model, queries, aggregate, limits, weights, known)
    ok = t['applicable']
    assert bool((t['T_B'][ok & (t['B64'] == 0)] == 0).all())
    return float(t['P64'][ok].median()), float((t['T_B'] * t['R'] / t['B64'])[ok & (t['B64'] > 0)].max())
