"""Inputs of the R-GCN edge attribution tests (include/tipk.h section 4j): seeded random directed graphs that hold every
kind of node the kernel treats differently, the layer's operands, and the queries that go with them."""
import torch

SEL_CAP = 4096                                   # entries of the kernel's selection buffer (tipk_attribution.hip AT_CAP)
HUB, ONE, ISOLATED, LOOP, OTHER = 0, 1, 2, 3, 4  # node ids with a fixed role (n >= 5)

# (n, R, B, d_in, d_out, k)
SHAPES = [(5, 2, 1, 4, 4, 3), (70, 5, 8, 32, 16, 1), (201, 7, 32, 32, 16, 1024), (130, 5, 32, 64, 32, 37),
          (77, 3, 64, 128, 128, 1024), (61, 4, 3, 7, 3, 5)]


def directed_graph(n, n_rel, seed, hub_edges=2 * SEL_CAP + 300):
    """(edge_index int64 [2, E], edge_type int64 [E]), edges in random order: node HUB has more than 2 x SEL_CAP in-edges (the
    selection's cut runs at least twice), node ONE exactly one, node ISOLATED no edge at all, node LOOP a self loop and a
    duplicated edge, every other node a few random ones; relation n_rel - 1 has no edge."""
    g = torch.Generator().manual_seed(seed)
    used = max(n_rel - 1, 1)
    sources = torch.tensor([v for v in range(n) if v != ISOLATED])

    def draw(m):
        return sources[torch.randint(0, sources.numel(), (m,), generator=g)], torch.randint(0, used, (m,), generator=g)

    src, rel = draw(hub_edges)
    parts = [(src, torch.full_like(src, HUB), rel)]
    parts.append((torch.tensor([OTHER]), torch.tensor([ONE]), torch.tensor([0])))
    parts.append((torch.tensor([LOOP, OTHER, OTHER, OTHER]), torch.tensor([LOOP] * 4), torch.tensor([0, used - 1, used - 1, 0])))
    for v in range(OTHER, n):
        m = int(torch.randint(1, 12, (1,), generator=g))
        src, rel = draw(m)
        parts.append((src, torch.full_like(src, v), rel))
    src, dst, rel = (torch.cat([p[i] for p in parts]) for i in range(3))
    perm = torch.randperm(src.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]]), rel[perm]


def operands(n, n_rel, n_bases, d_in, d_out, seed):
    """(h, basis, att, root) fp32 on the host: h = relu of a normal draw, as the layer's input is."""
    g = torch.Generator().manual_seed(seed + 1000)
    h = torch.relu(torch.randn(n, d_in, generator=g))
    basis = torch.randn(n_bases, d_in, d_out, generator=g) * (2.0 / d_in)
    att = torch.randn(n_rel, n_bases, generator=g) / n_bases ** 0.5
    root = torch.randn(d_in, d_out, generator=g) * (2.0 / d_in)
    return h, basis, att, root


def queries(n, d_out, seed):
    """(q_node int64 [Q], probe fp32 [Q, d_out]): every role under a random probe, the hub under a second probe and under a
    zero probe (every contribution ties at 0: the order is by position), the last node, and the ids -1 and n."""
    g = torch.Generator().manual_seed(seed + 2000)
    nodes = [HUB, ONE, ISOLATED, LOOP, OTHER, HUB, HUB, n - 1, -1, n]
    probe = torch.randn(len(nodes), d_out, generator=g)
    probe[6] = 0.0
    return torch.tensor(nodes, dtype=torch.int64), probe
