"""Seeded cases of the new-drug fit shared by the host and the GPU tests (tests/drug_fit_spec.py holds the rules).

A convergence case is (name, z [n, dim], rel_w [R, dim] fp32 on the CPU, lists: ONE list of (partner, side effect), prior,
init, l2).  z comes from `fit_cases.embeddings`, rel_w is a seeded randn rounded to fp32; both are seeded by the shape, so the
cases of one shape share them and can be fitted in one call.  The lists are PLANTED unless the name
says random: the P cells a hidden row scores highest under unit Gumbel noise over the n R features, so the data has a signal
to fit.  The condition on a case (the host test asserts it) is that the fp64 spec converges within 8 evaluations.
"""
import torch

from fit_cases import embeddings, trial_rows                              # noqa: F401  (trial_rows: for the tests)

# name, n, R, dim, P, kind, l2, z scale, prior scale
CONVERGENCE = [('n65_r8_d16_p40', 65, 8, 16, 40, 'planted', 1e-4, 1.0, 0.0),
               ('n65_r8_d16_p3', 65, 8, 16, 3, 'planted', 1e-4, 1.0, 0.0),
               ('n65_r8_d16_p1', 65, 8, 16, 1, 'planted', 1e-4, 1.0, 0.0),
               ('n130_r20_d16_p300_random', 130, 20, 16, 300, 'random', 1e-4, 1.0, 0.0),
               ('n645_r32_d16_p300', 645, 32, 16, 300, 'planted', 1e-4, 1.0, 0.0),
               ('n65_r8_d4_p40', 65, 8, 4, 40, 'planted', 1e-4, 1.0, 0.0),
               ('n65_r8_d16_p40_z3', 65, 8, 16, 40, 'planted', 1e-4, 3.0, 0.0),
               ('n65_r8_d16_p40_prior', 65, 8, 16, 40, 'planted', 1e-2, 1.0, 0.5),
               ('n65_r130_d16_p200', 65, 130, 16, 200, 'planted', 1e-4, 1.0, 0.0)]


def relations(n_rel, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n_rel, dim), generator=g).float()


def random_cells(n, n_rel, count, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, n, (count,), generator=g)
    r = torch.randint(0, n_rel, (count,), generator=g)
    return list(zip(v.tolist(), r.tolist()))


def planted_cells(z, rel_w, count, seed):
    """The `count` cells (v, r) that a hidden row scores highest under unit Gumbel noise."""
    g = torch.Generator().manual_seed(seed)
    n_rel = rel_w.shape[0]
    hidden = torch.randn(z.shape[1], generator=g).double() * 2.0
    s = ((z.double() * hidden) @ rel_w.double().t()).reshape(-1)         # cell v * R + r
    noise = -torch.log(-torch.log(torch.rand(s.shape, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)))
    top = torch.topk(s + noise, min(count, s.numel())).indices
    return list(zip((top // n_rel).tolist(), (top % n_rel).tolist()))


def convergence_cases():
    out = []
    for i, (name, n, n_rel, dim, count, kind, l2, scale, pscale) in enumerate(CONVERGENCE):
        z, rel_w = embeddings(n, dim, 1100 + n + 7 * dim, scale), relations(n_rel, dim, 1200 + n_rel + 7 * dim)
        cells = planted_cells(z, rel_w, count, 1300 + i) if kind == 'planted' else random_cells(n, n_rel, count, 1300 + i)
        prior = init = None
        if pscale:                                                       # a random centre; the start stays at zero
            prior = (torch.randn((1, dim), generator=torch.Generator().manual_seed(1400 + i)) * pscale).float()
            init = torch.zeros((1, dim))
        out.append((name, z, rel_w, [cells], prior, init, l2))
    return out


def list_kinds(n, n_rel, seed):
    """The list shapes of the statistics tests: empty, one cell, every cell, a long list with repeats."""
    every = [(v, r) for v in range(n) for r in range(n_rel)]
    long = random_cells(n, n_rel, 3 * max(n, n_rel) + 7, seed)
    long = long + long[:max(n, n_rel)] + long[:5]
    return {'empty': [], 'one': [(n - 1, n_rel - 1)], 'every': every, 'long': long}
