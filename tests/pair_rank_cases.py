"""The seeded inputs of the pair rank tests (include/tipk.h section 4f), built on the host so that tests/test_host_pair_rank.py
can hold every random-input case of tests/test_gpu_pair_rank.py to the degeneracy cap of tests/pair_rank_spec.py without a
device.  A case is (model, pairs [2, P], tgt_ptr [P + 1], tgt_rel [T], known or None), all CPU tensors."""
import torch

from pair_topk_spec import known_from_dict

N = 97
SMALL_R = (1, 63, 64, 65, 130)
SMALL_DIM = (4, 16, 128)
COUNTS = (0, 1, 63, 64, 65, 130)
ROUTES = ((700, 16, 3000), (700, 32, 3000), (4500, 16, 1000))      # (n_rel, dim, pairs); the last cannot take the LDS route


def model_of(kind, n, n_rel, dim, g, pad=0):
    if kind == 'distmult':
        return ('distmult', torch.randn(n, dim, generator=g) / dim ** 0.25, torch.randn(n_rel, dim, generator=g) / dim ** 0.25)
    wide = torch.randn(2, n, n_rel + pad, generator=g)                    # row stride n_rel + pad
    return ('table', wide[0, :, :n_rel], wide[1, :, :n_rel])


def csr(lists):
    ptr = [0]
    for t in lists:
        ptr.append(ptr[-1] + len(t))
    return torch.tensor(ptr, dtype=torch.int64), torch.tensor([r for t in lists for r in t], dtype=torch.int32)


def random_known(n_rel, g, n=N, pairs=300, share=0.3):
    d = {}
    for u, v in torch.randint(0, n, (pairs, 2), generator=g).tolist():
        d[(u, v)] = torch.nonzero(torch.rand(n_rel, generator=g) < share).reshape(-1).tolist()
    return d


def small_case(kind, n_rel, dim=0):
    """40 pairs -- a pair, its reverse, a self pair, the first pair again, then random ones -- with 0..6 random targets each
    (repeats allowed) and random known lists; the first pairs' key is listed too."""
    g = torch.Generator().manual_seed(1013 * n_rel + dim + (7 if kind == 'table' else 0))
    model = model_of(kind, N, n_rel, dim, g, pad=5)
    head = [(3, 7), (7, 3), (5, 5), (3, 7)]
    pairs = torch.cat([torch.tensor(head), torch.randint(0, N, (36, 2), generator=g)]).t().contiguous()
    d = random_known(n_rel, g)
    d[(7, 3)] = list(range(0, n_rel, 3))
    for u, v in pairs.t().tolist()[4:20]:                                  # half of the random pairs have a block
        d[(u, v)] = torch.nonzero(torch.rand(n_rel, generator=g) < 0.3).reshape(-1).tolist()
    lists = [torch.randint(0, n_rel, (int(c),), generator=g).tolist() for c in torch.randint(0, 7, (40,), generator=g)]
    lists[0] = lists[0] + [0, n_rel - 1]
    lists[1], lists[3] = list(lists[0]), list(lists[0])
    tgt_ptr, tgt_rel = csr(lists)
    return model, pairs, tgt_ptr, tgt_rel, known_from_dict(d, N)


def counts_case(kind):
    """One pair per target count in COUNTS (random targets, repeats allowed), then every relation once, at n_rel = 130; no
    filter on the last pair: its ranks are a permutation of 1..R."""
    n_rel = 130
    g = torch.Generator().manual_seed(4242 + (1 if kind == 'table' else 0))
    model = model_of(kind, N, n_rel, 16, g)
    pairs = torch.randint(0, N - 1, (2, len(COUNTS) + 1), generator=g)
    pairs[:, -1] = torch.tensor([N - 1, 11])
    lists = [torch.randint(0, n_rel, (c,), generator=g).tolist() for c in COUNTS] + [torch.randperm(n_rel, generator=g).tolist()]
    lists[3][5] = lists[3][40]                                            # a repeated target
    d = random_known(n_rel, g, n=N - 1)                                   # node N - 1 is in no key
    for u, v in pairs.t().tolist()[:-1]:
        d[(u, v)] = torch.nonzero(torch.rand(n_rel, generator=g) < 0.3).reshape(-1).tolist()
    tgt_ptr, tgt_rel = csr(lists)
    return model, pairs, tgt_ptr, tgt_rel, known_from_dict(d, N)


def corner_case(kind, n_rel):
    """The known filter's corners (n_rel = 4 500 spans three bitmap windows of 2 048 relations).  Pairs, in order: the first
    key (0, 0), a self pair; (4, 9), listed as (9, 4); (9, 4); (20, 30), every relation listed; (30, 20); (40, 41), no
    block; (50, 60), no block; the last key (96, 96); (0, 1); (1, 0).  -> (case, some): `some` is the list of (0, 0), (9, 4)
    and (96, 96)."""
    g = torch.Generator().manual_seed(n_rel + (1 if kind == 'table' else 0))
    model = model_of(kind, N, n_rel, 8, g)
    edge = {0, 2047, 2048, n_rel - 1} & set(range(n_rel))
    some = sorted(set(torch.randint(0, n_rel, (n_rel // 2,), generator=g).tolist()) | edge)
    d = {(0, 0): some, (9, 4): some, (20, 30): range(n_rel), (40, 41): [], (N - 1, N - 1): some}
    pairs = torch.tensor([[0, 4, 9, 20, 30, 40, 50, N - 1, 0, 1],
                          [0, 9, 4, 30, 20, 41, 60, N - 1, 1, 0]])
    listed, free = some[::max(1, len(some) // 20)], sorted(set(range(n_rel)) - set(some))
    both = sorted(edge) + listed[:20] + free[::max(1, len(free) // 20)][:20]   # on both sides of the window edge
    lists = [both] * pairs.shape[1]
    tgt_ptr, tgt_rel = csr(lists)
    return (model, pairs, tgt_ptr, tgt_rel, known_from_dict(d, N)), some


def routes_case(n_rel, dim, n_pairs=3000):
    """Random pairs with 0..9 random targets each.  Nine in ten of their keys have a known block, which lists every
    relation with probability `share`: 0.1, and 0.6 at n_rel = 4 500 -- 4 500 N(0, 1) logits at dim 16 lie so close that
    without the filter more than 1 % of the targets would have two admissible ranks, the cap of pair_rank_spec."""
    g = torch.Generator().manual_seed(31 * n_rel + dim)
    share = 0.6 if n_rel > 2048 else 0.1
    model = model_of('distmult', N, n_rel, dim, g)
    pairs = torch.randint(0, N, (2, n_pairs), generator=g)
    count = torch.randint(0, 10, (n_pairs,), generator=g)
    tgt_ptr = torch.zeros(n_pairs + 1, dtype=torch.int64)
    tgt_ptr[1:] = torch.cumsum(count, 0)
    tgt_rel = torch.randint(0, n_rel, (int(tgt_ptr[-1]),), generator=g).to(torch.int32)
    keys = torch.unique(torch.minimum(pairs[0], pairs[1]) * N + torch.maximum(pairs[0], pairs[1]))
    keys = keys[torch.rand(keys.numel(), generator=g) < 0.9]
    mask = torch.rand(keys.numel(), n_rel, generator=g) < share
    mask[:, 0] = True                                                     # no empty block
    kptr = torch.zeros(keys.numel() + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(mask.sum(1), 0)
    return model, pairs, tgt_ptr, tgt_rel, (keys, kptr, torch.nonzero(mask)[:, 1].to(torch.int32))


def biosnap_weights(n, n_rel, dim=16):
    g = torch.Generator().manual_seed(645)
    return ('distmult', torch.randn(n, dim, generator=g) / 2, torch.randn(n_rel, dim, generator=g) / 2)
