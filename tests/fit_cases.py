"""Seeded cases of the side-effect fit shared by the host and the GPU tests (tests/fit_spec.py holds the rules).

A case is (name, z [n, dim] fp32 on the CPU, pairs: a list of B lists of (u, v)).  The CONVERGENCE cases are the shapes the
fit is specified on -- (n, dim, pairs) = (65, 16, 40), (65, 16, 5), (65, 16, 1), (130, 16, 300 random), (645, 16, 2 000),
(645, 16, 300), (65, 4, 40) and (65, 16, 40) with z scaled by 3 -- one new side effect each; the lists are PLANTED unless the
name says random: the P pairs a hidden row scores highest, under noise, so the data has a signal to fit.
"""
import torch

CONVERGENCE = [('n65_d16_p40', 65, 16, 40, 'planted', 1.0), ('n65_d16_p5', 65, 16, 5, 'planted', 1.0),
               ('n65_d16_p1', 65, 16, 1, 'planted', 1.0), ('n130_d16_p300_random', 130, 16, 300, 'random', 1.0),
               ('n645_d16_p2000', 645, 16, 2000, 'planted', 1.0), ('n645_d16_p300', 645, 16, 300, 'planted', 1.0),
               ('n65_d4_p40', 65, 4, 40, 'planted', 1.0), ('n65_d16_p40_z3', 65, 16, 40, 'planted', 3.0)]


def embeddings(n, dim, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, dim), generator=g) * (scale / dim ** 0.5 * 2.0)).float()


def random_pairs(n, count, seed, selfs=False):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, n, (count,), generator=g)
    v = torch.randint(0, n, (count,), generator=g)
    if not selfs and n > 1:
        v = torch.where(u == v, (v + 1) % n, v)
    return list(zip(u.tolist(), v.tolist()))


def pair_features(z):
    """(iu, iv, f [M, dim] fp64) of the pairs u < v: what `planted_pairs` scores (pass it on when one z serves many lists)."""
    iu, iv = torch.triu_indices(z.shape[0], z.shape[0], offset=1)
    return iu, iv, z.double()[iu] * z.double()[iv]


def planted_pairs(z, count, seed, feats=None):
    """The `count` pairs u < v that a hidden row scores highest under unit Gumbel noise."""
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(z.shape[1], generator=g).double() * 2.0
    iu, iv, f = pair_features(z) if feats is None else feats
    s = f @ hidden
    noise = -torch.log(-torch.log(torch.rand(s.shape, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)))
    top = torch.topk(s + noise, min(count, s.numel())).indices
    return list(zip(iu[top].tolist(), iv[top].tolist()))


def convergence_cases():
    out = []
    for i, (name, n, dim, count, kind, scale) in enumerate(CONVERGENCE):
        z = embeddings(n, dim, 100 + i, scale)
        pairs = planted_pairs(z, count, 200 + i) if kind == 'planted' else random_pairs(n, count, 200 + i)
        out.append((name, z, [pairs]))
    return out


def list_kinds(n, seed):
    """The list shapes of the statistics tests for n drugs: empty, one pair, self pairs only, every pair, a long list with
    repeats and mirrored repeats."""
    every = [(u, v) for u in range(n) for v in range(u, n)]
    long = random_pairs(n, 3 * n + 7, seed, selfs=True)
    long = long + [(v, u) for u, v in long[:n]] + long[:5]
    return {'empty': [], 'one': [(0, n - 1)], 'selfs': [(u, u) for u in range(0, n, 2)], 'every': every, 'long': long}


def trial_rows(b, dim, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'zero':
        return torch.zeros((b, dim))
    w = torch.randn((b, dim), generator=g)
    return (w * 40.0 if kind == 'large' else w * 0.5).float()
