"""Seeded cases of the decoder-row posterior and the confidence top-k shared by the host and the GPU tests
(tests/conf_spec.py holds the rules).

END TO END cases (statistics -> factor -> query): the embeddings, lists and trial rows of tests/fit_cases.py -- three
relations with the lists 'long', 'one' and 'selfs' -- at
    rows 'zero' and 'random', l2 = 1e-4, n = 65 and 129, dim = 4, 16, 32      (dim U kappa_2 of the fp64 Hessians: at most 1.1e-4)
    rows 'large',             l2 = 1e-2, n = 65,         dim = 16             (5.3e-6)
'large' at l2 = 1e-4 is NOT a case: rows that saturate the sigmoids leave the prior alone to bound the smallest eigenvalue;
dim U kappa_2 is then 4.3e-4 with these seeds and reaches 1e-3 to 3e-3 with others -- at or above the cap of 2^-10 that keeps
the end-to-end bound from going vacuous (tests/test_host_pair_conf.py asserts half the cap for every case here).
"""
import torch

import fit_cases

END_TO_END = [('n%d_d%d_%s' % (n, dim, kind), n, dim, kind, 1e-4) for n in (65, 129) for dim in (4, 16, 32)
              for kind in ('zero', 'random')] + [('n65_d16_large', 65, 16, 'large', 1e-2)]
LISTS = ('long', 'one', 'selfs')


def end_to_end_case(n, dim, kind):
    """(z [n, dim], lists, w [3, dim]) on the host."""
    z = fit_cases.embeddings(n, dim, 300 + n + dim, 2.0)
    kinds = fit_cases.list_kinds(n, n + dim)
    return z, [kinds[k] for k in LISTS], fit_cases.trial_rows(len(LISTS), dim, kind, 400 + n + dim)


def spd_matrices(b, dim, seed):
    """(H [b, dim, dim] fp32 = A A^T + lambda I, built in fp64 on the host) with condition numbers spread from 1 to 1e4."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(b):
        kappa = 10.0 ** (4.0 * (i % 5) / 4.0)                            # 1, 10, 100, 1e3, 1e4
        q, _ = torch.linalg.qr(torch.randn((dim, dim), generator=g, dtype=torch.float64))
        ev = torch.logspace(0, -torch.log10(torch.tensor(kappa)).item(), dim, dtype=torch.float64) if dim > 1 \
            else torch.ones(1, dtype=torch.float64)
        a = q * ev.sqrt() * (0.5 + 2.0 * torch.rand(1, generator=g, dtype=torch.float64))
        lam = float(ev[-1]) * 1e-3
        out.append(a @ a.t() + lam * torch.eye(dim, dtype=torch.float64))
    return torch.stack(out).float() if out else torch.zeros((0, dim, dim))


def query_case(n, dim, n_rel, seed, scale=1.0):
    """(z [n, dim], rel_w [R, dim], W physical [R, dim, dim]) on the host: random embeddings and rows, and the factor of a
    random SPD matrix per relation with a row scale in {1, 3^(-1/2), 7600^(-1/2)}, computed in fp64 and rounded."""
    g = torch.Generator().manual_seed(seed)
    z = fit_cases.embeddings(n, dim, seed, scale)
    rel_w = torch.randn((n_rel, dim), generator=g).float()
    h = spd_matrices(n_rel, dim, seed + 1).double()
    chol = torch.linalg.cholesky(h)
    inv = torch.linalg.solve_triangular(chol, torch.eye(dim, dtype=torch.float64).expand_as(h), upper=False)
    scale_r = torch.tensor([1.0, 3.0 ** -0.5, 7600.0 ** -0.5], dtype=torch.float64)[torch.arange(n_rel) % 3]
    w_log = inv * scale_r.reshape(-1, 1, 1)
    return z, rel_w, w_log.transpose(1, 2).contiguous().float()
