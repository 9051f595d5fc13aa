"""Inputs of the protein attribution tests (include/tipk.h section 4o): seeded tri-graphs (D-D edges, P -> D edges) that hold
every kind of drug and protein the kernels treat differently, the frozen model's operands, and the queries that go with them.
`case(shape)` builds each once per process and keeps it (with its fp64 spec), unchanged, for every test that asks."""
import torch

from protein_attribution_spec import Operands, Spec, forward64

SEL_CAP = 4096                                   # entries of the kernel's selection buffer (tipk_protein_attribution.hip PA_CAP)
CHUNK = 256                                      # queries per pass over the workspace (tipk_protein_attribution_chunk())
# drug ids with a fixed role (n >= 6): HUB has an in-edge from every other non-isolated drug, some duplicated; ONE exactly one
# in-edge; ISOLATED no D-D edge at all (it has targets); LOOP a self loop and a duplicated edge; NOTARGET no protein target;
# ZEROH an all-zero h row (no in-edge, no target, a zero embedding row; it has out-edges), so its mask is empty
HUB, ONE, ISOLATED, LOOP, NOTARGET, ZEROH = 0, 1, 2, 3, 4, 5
# protein ids with a fixed role: EVERY is targeted by every drug that has a target at all, DUP twice by the hub; the last
# protein by no drug (never a candidate)
EVERY, DUP = 0, 1

# (N, P, R, B, ne, pd, p, d1, d2, k, mode)
SHAPES = [(6, 4, 2, 1, 3, 2, 2, 4, 4, 3, 'cat'),                # the smallest case
          (7, 5, 3, 3, 5, 5, 3, 7, 3, 5, 'add'),                # every width odd
          (65, 40, 5, 8, 16, 16, 16, 32, 16, 1, 'cat'),         # N one past a tile, k = 1
          (130, 9000, 5, 32, 48, 16, 16, 32, 16, 1024, 'cat'),  # > 2 x 4096 candidates: the selection cuts at least twice
          (77, 50, 3, 64, 64, 64, 64, 128, 128, 37, 'add')]     # the widest dims


def shape_id(s):
    return 'x'.join(map(str, s))


def dd_graph(n, n_rel, seed):
    """(src, dst, rel) int64 [E] in random order; relation n_rel - 1 has no edge."""
    g = torch.Generator().manual_seed(seed)
    used = max(n_rel - 1, 1)
    sources = [v for v in range(n) if v != ISOLATED]
    edges = []

    def rel():
        return int(torch.randint(0, used, (1,), generator=g))

    for s in sources:                                            # the hub: every other drug, every third one twice
        if s != HUB:
            edges.append((s, HUB, rel()))
            if s % 3 == 0:
                edges.append((s, HUB, edges[-1][2]))
    edges.append((LOOP, ONE, 0))
    edges += [(LOOP, LOOP, 0), (HUB, LOOP, used - 1), (HUB, LOOP, used - 1), (HUB, LOOP, 0)]
    for v in [NOTARGET] + list(range(ZEROH + 1, n)):
        for _ in range(int(torch.randint(1, 6, (1,), generator=g))):
            edges.append((sources[int(torch.randint(0, len(sources), (1,), generator=g))], v, rel()))
    e = torch.tensor(edges, dtype=torch.int64)
    e = e[torch.randperm(e.shape[0], generator=g)]
    return e[:, 0].contiguous(), e[:, 1].contiguous(), e[:, 2].contiguous()


def pd_graph(n, n_prot, seed):
    """(prot, drug) int64 [E] in random order: every protein but the last is targeted by some drug."""
    g = torch.Generator().manual_seed(seed + 500)
    targeted = [v for v in range(n) if v not in (NOTARGET, ZEROH)]
    edges = [(EVERY, v) for v in targeted] + [(DUP, HUB), (DUP, HUB)]
    for t in range(DUP, n_prot - 1):
        edges.append((t, targeted[int(torch.randint(0, len(targeted), (1,), generator=g))]))
    for v in targeted:
        if n_prot > 3:
            edges.append((int(torch.randint(DUP, n_prot - 1, (1,), generator=g)), v))
    e = torch.tensor(edges, dtype=torch.int64)
    e = e[torch.randperm(e.shape[0], generator=g)]
    return e[:, 0].contiguous(), e[:, 1].contiguous()


def operands(shape):
    n, n_prot, n_rel, B, ne, pd, p, d1, d2, k, mode = shape
    seed = sum(shape[:-1])
    cat = mode == 'cat'
    d0 = ne + pd if cat else ne
    g = torch.Generator().manual_seed(seed + 1000)
    hp = torch.randn(n_prot, p, generator=g)
    w_pd = torch.randn(p, pd, generator=g) / p ** 0.5
    xe = torch.randn(n, ne, generator=g)
    xe[ZEROH] = 0.0
    layer1 = (torch.randn(B, d0, d1, generator=g) * (2.0 / d0), torch.randn(n_rel, B, generator=g) / B ** 0.5,
              torch.randn(d0, d1, generator=g) * (2.0 / d0))
    layer2 = (torch.randn(B, d1, d2, generator=g) * (2.0 / d1), torch.randn(n_rel, B, generator=g) / B ** 0.5,
              torch.randn(d1, d2, generator=g) * (2.0 / d1))
    dd, pde = dd_graph(n, n_rel, seed), pd_graph(n, n_prot, seed)
    dbl = lambda ts: tuple(t.double() for t in ts)
    h = forward64(hp.double(), w_pd.double(), xe.double(), dbl(layer1), dbl(layer2), dd, pde, cat)[1].float()
    return Operands(hp, w_pd, xe, h, layer1, layer2, dd, pde, cat)


def queries(shape):
    """(q_node int64 [Q], probe fp32 [Q, d2]): every role under a random probe, the hub under a second probe and under a zero
    probe (every contribution ties at 0: the order is by protein id), the last drug, and the ids -1 and N."""
    n, d2 = shape[0], shape[8]
    g = torch.Generator().manual_seed(sum(shape[:-1]) + 2000)
    nodes = [HUB, ONE, ISOLATED, LOOP, NOTARGET, ZEROH, HUB, HUB, n - 1, -1, n]
    probe = torch.randn(len(nodes), d2, generator=g)
    probe[7] = 0.0
    return torch.tensor(nodes, dtype=torch.int64), probe


_CASES = {}


def case(shape):
    """(operands, Spec, q_node, probe) of a shape, built once."""
    if shape not in _CASES:
        op = operands(shape)
        _CASES[shape] = (op, Spec(op)) + queries(shape)
    return _CASES[shape]
