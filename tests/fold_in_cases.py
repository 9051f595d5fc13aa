"""Inputs of the drug fold-in tests (include/tipk.h section 4k): ONE seeded generator of M = 37 new drugs (no multiple of the
kernel's tile of 16) over N = 61 existing drugs, R = 7 relations and 40 proteins, with every kind of new drug the kernel treats
differently, and the frozen model's tables and parameters that go with them."""
import collections

import torch

M, N, R, N_PROT = 37, 61, 7, 40
HUB_EDGES, HUB_PAIRS = 5000, 200
# new drugs with a fixed role
BARE, FEATURES_ONLY, TARGETS_ONLY, ONE_TARGET, EDGES_ONLY, ONE_EDGE, HUB, ENDS, LAST_REL = range(9)
UNTARGETED = N_PROT - 1                          # the protein no existing drug targets (only TARGETS_ONLY lists it)
UNUSED_REL = R - 2                               # never used, while R - 1 is

# (ne, pd, d1, d2, B, cat, p): the dims of tip.py in both modes, and widths that are multiples of nothing
DIMS = [(48, 16, 32, 16, 32, True, 16), (5, 3, 7, 4, 3, True, 6), (16, 16, 32, 16, 32, False, 16)]

Case = collections.namedtuple('Case', ['h_prot', 'hgcn_w', 'x0', 'h1', 'layer1', 'layer2', 'xd', 'targets', 'interactions', 'cat'])


def csr(lists, width):
    """A list of per-drug lists (ints, or tuples of `width` ints) -> (ptr int64 [len + 1], `width` int32 tensors)."""
    ptr, cols = [0], [[] for _ in range(width)]
    for row in lists:
        for item in row:
            for c, v in enumerate((item,) if width == 1 else item):
                cols[c].append(int(v))
        ptr.append(len(cols[0]))
    return (torch.tensor(ptr, dtype=torch.int64),) + tuple(torch.tensor(c, dtype=torch.int32) for c in cols)


def new_drug_lists(seed=0):
    """(targets, interactions, has_features): per new drug its protein ids, its (partner, relation) pairs, in the order the
    kernel will walk them, and whether it has a drug feature."""
    g = torch.Generator().manual_seed(seed + 50)
    rels = [r for r in range(R) if r != UNUSED_REL]

    def pairs(n):
        return [(int(torch.randint(0, N, (1,), generator=g)), rels[int(torch.randint(0, len(rels), (1,), generator=g))])
                for _ in range(n)]

    def prots(n):
        return torch.randperm(N_PROT - 1, generator=g)[:n].tolist()              # never UNTARGETED

    targets, inter, feat = [[] for _ in range(M)], [[] for _ in range(M)], [True] * M
    feat[BARE] = False
    targets[TARGETS_ONLY] = prots(4) + [UNTARGETED]
    targets[ONE_TARGET], feat[ONE_TARGET] = prots(1), False
    inter[EDGES_ONLY] = pairs(9)
    inter[ONE_EDGE] = pairs(1)
    distinct = [(k // len(rels), rels[k % len(rels)])                            # the hub: 5 000 entries, 200 distinct pairs
                for k in torch.randperm(N * len(rels), generator=g)[:HUB_PAIRS].tolist()]
    order = torch.randperm(HUB_EDGES, generator=g).tolist()
    inter[HUB], targets[HUB] = [distinct[i % HUB_PAIRS] for i in order], prots(3)
    inter[ENDS], targets[ENDS] = [(0, 0), (N - 1, 1), (0, 0), (N - 1, R - 1)], prots(2)
    inter[LAST_REL] = [(5, R - 1), (17, R - 1), (5, R - 1)]
    for m in range(LAST_REL + 1, M):
        targets[m] = prots(int(torch.randint(0, 6, (1,), generator=g)))
        inter[m] = pairs(int(torch.randint(0, 13, (1,), generator=g)))
        feat[m] = bool(torch.randint(0, 4, (1,), generator=g))
    return targets, inter, feat


def make_case(dims, seed=0):
    """The Case of one entry of DIMS, fp32 on the host: x0 has both signs, h1 is the ReLU of a normal draw (about half zeros),
    xd is zero for the drugs without a feature."""
    ne, pd, d1, d2, n_bases, cat, p = dims
    d0 = ne + pd if cat else ne
    g = torch.Generator().manual_seed(seed + sum(dims))
    rn = lambda *s: torch.randn(*s, generator=g)
    targets, inter, feat = new_drug_lists(seed)
    layer1 = (rn(n_bases, d0, d1) / d0 ** 0.5, rn(R, n_bases) / n_bases ** 0.5, rn(d0, d1) / d0 ** 0.5)
    layer2 = (rn(n_bases, d1, d2) * (2.0 / d1), rn(R, n_bases) / n_bases ** 0.5, rn(d1, d2) * (2.0 / d1))
    xd = rn(M, ne) * torch.tensor(feat, dtype=torch.float32)[:, None]
    return Case(rn(N_PROT, p), rn(p, pd) / p ** 0.5, rn(N, d0), torch.relu(rn(N, d1)), layer1, layer2, xd,
                csr(targets, 1), csr(inter, 2), cat)


def take(case, lo, hi):
    """The same Case for the new drugs lo .. hi - 1 alone."""
    def cut(lists):
        ptr = lists[0]
        a, b = int(ptr[lo]), int(ptr[hi])
        return (ptr[lo:hi + 1] - a,) + tuple(c[a:b] for c in lists[1:])
    return case._replace(xd=case.xd[lo:hi], targets=cut(case.targets), interactions=cut(case.interactions))


def to(case, device):
    """Every tensor of the Case on `device`."""
    mv = lambda v: v.to(device) if torch.is_tensor(v) else (tuple(mv(x) for x in v) if isinstance(v, tuple) else v)
    return Case(*(mv(v) for v in case))
