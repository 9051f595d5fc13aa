"""Inputs of the screen rank tests (include/tipk.h section 4h), as host tensors: tests/test_host_screen_rank.py asserts for each
that fp32 and fp64 logits agree exactly, tests/test_gpu_screen_rank.py runs them on the device.  A case is
(z, w, known, q_rel, tgt_ptr, tgt_u, tgt_v) with known = (keys, ptr) or None."""
import torch

from screen_spec import keys_from_pairs

SMALL = [(70, 4), (97, 16), (201, 32), (130, 64), (77, 128), (133, 256), (130, 36)]
EDGE_N = [1, 2, 63, 64, 65, 128, 129]


def exact_zw(n, dim, n_rel, g):
    """z in {-2, -1.75, ..., 2}, w in {-2, -1.5, ..., 2}: every product and partial sum is exact in fp32 for dim <= 256, and
    the few thousand distinct logits tie massively, which exercises the key order."""
    z = torch.randint(-8, 9, (n, dim), generator=g).float() / 4
    w = torch.randint(-4, 5, (n_rel, dim), generator=g).float() / 2
    return z, w


def csr(lists):
    """[[(u, v), ...], ...] -> (tgt_ptr int64, tgt_u int32, tgt_v int32)"""
    ptr, flat = [0], []
    for pairs in lists:
        flat += list(pairs)
        ptr.append(len(flat))
    u = torch.tensor([p[0] for p in flat], dtype=torch.int32)
    v = torch.tensor([p[1] for p in flat], dtype=torch.int32)
    return torch.tensor(ptr, dtype=torch.int64), u, v


def graph_known(n, g):
    """The known-pair patterns of tests/test_gpu_screen.py: r0 ~15 % of the pairs, one direction only (larger id first); r1
    ~4 %, both directions; r2 none; r3 every pair; r4 every partner of drug 7 and two more pairs -> per-relation lists."""
    iu = torch.triu_indices(n, n, 1)
    m0 = torch.rand(iu.shape[1], generator=g) < 0.15
    r0 = list(zip(iu[1][m0].tolist(), iu[0][m0].tolist()))
    m1 = torch.rand(iu.shape[1], generator=g) < 0.04
    r1 = list(zip(iu[0][m1].tolist(), iu[1][m1].tolist()))
    r1 += [(b, a) for a, b in r1]
    r3 = list(zip(iu[0].tolist(), iu[1].tolist()))
    r4 = [(7, v) for v in range(n) if v != 7] + [(1, 2), (3, 1)]
    return [r0, r1, [], r3, r4]


def _targets(n, listed, g, n_random=40):
    """listed and unlisted pairs, reversed orientations, repeats, a self pair, ids -1 and n"""
    u = torch.randint(0, n, (n_random,), generator=g).tolist()
    v = torch.randint(0, n, (n_random,), generator=g).tolist()
    t = list(zip(u, v)) + list(listed[:10])
    t += [(b, a) for a, b in t[:5]] + [(b, a) for a, b in listed[:3]] + t[:3]
    return t + [(3, 3), (-1, 2), (2, n), (n, -1), (0, 1), (1, 0)]


def small_case(n, dim):
    g = torch.Generator().manual_seed(1000 * n + dim)
    z, w = exact_zw(n, dim, 5, g)
    lists = graph_known(n, g)
    known = keys_from_pairs(lists, n)
    # every relation, a relation below and one above the range, a query without targets, a second query on relation 0
    q_rel = [0, 1, 2, 3, 4, -1, 5, 1, 0]
    tg = [_targets(n, lists[0], g), _targets(n, lists[1], g), _targets(n, [], g), _targets(n, lists[3], g),
          _targets(n, lists[4], g), _targets(n, lists[0], g), _targets(n, lists[1], g), [], _targets(n, lists[0][5:], g)]
    return (z, w, known, torch.tensor(q_rel, dtype=torch.int32)) + csr(tg)


def all_pairs_case(n, dim=16):
    """every pair of the graph as a target of relations 0 (a sparse one-direction list) and 1 (no list)"""
    g = torch.Generator().manual_seed(77 + n)
    z, w = exact_zw(n, dim, 2, g)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    listed = [(b, a) for i, (a, b) in enumerate(pairs) if i % 7 == 3]
    known = keys_from_pairs([listed, []], n)
    if not listed:
        known = None
    return (z, w, known, torch.tensor([0, 1], dtype=torch.int32)) + csr([pairs, pairs])


def nan_case(n=90, dim=16, row=11):
    """(case with row `row` of z NaN, the same case with finite z and every pair of that drug listed for every relation)"""
    g = torch.Generator().manual_seed(90)
    z, w = exact_zw(n, dim, 2, g)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    listed = [(b, a) for i, (a, b) in enumerate(pairs) if i % 5 == 1]
    tg = [pairs[::3] + [(row, 0), (n - 1, row)], [(b, a) for a, b in pairs[1::4]]]
    q = torch.tensor([0, 1], dtype=torch.int32)
    zn = z.clone()
    zn[row] = float('nan')
    drug = [(row, c) for c in range(n) if c != row]
    return ((zn, w, keys_from_pairs([listed, []], n), q) + csr(tg),
            (z, w, keys_from_pairs([listed + drug, drug], n), q) + csr(tg))


def chunk_case(n_targets, n=200, dim=16):
    """one relation, n_targets targets: the pairs in a shuffled order, repeated from the start when there are not enough"""
    g = torch.Generator().manual_seed(200)
    z, w = exact_zw(n, dim, 1, g)
    iu = torch.triu_indices(n, n, 1)[:, torch.randperm(n * (n - 1) // 2, generator=g)]
    m = iu.shape[1]
    listed = list(zip(iu[1][:m // 6].tolist(), iu[0][:m // 6].tolist()))
    at = torch.arange(n_targets) % m
    flip = torch.arange(n_targets) % 3 == 0
    u, v = torch.where(flip, iu[1][at], iu[0][at]), torch.where(flip, iu[0][at], iu[1][at])
    ptr = torch.tensor([0, n_targets], dtype=torch.int64)
    return z, w, keys_from_pairs([listed], n), torch.tensor([0], dtype=torch.int32), ptr, u.int(), v.int()


def random_targets(n, count, g):
    u = torch.randint(0, n, (count,), generator=g)
    v = (u + 1 + torch.randint(0, n - 1, (count,), generator=g)) % n
    return u.int(), v.int()


def single_query_case(n=700, dim=16, count=600):
    """n_q = 1: the query is split over 64 parts"""
    g = torch.Generator().manual_seed(700)
    z, w = exact_zw(n, dim, 1, g)
    u, v = random_targets(n, count, g)
    known = keys_from_pairs([list(zip(v[::2].tolist(), u[::2].tolist()))], n)
    return z, w, known, torch.tensor([0], dtype=torch.int32), torch.tensor([0, count], dtype=torch.int64), u, v


def many_queries_case(n_q=4200, n=70, dim=16, per=3):
    """thousands of queries of one part each, relations cycling over 5"""
    g = torch.Generator().manual_seed(4200)
    z, w = exact_zw(n, dim, 5, g)
    known = keys_from_pairs(graph_known(n, g), n)
    u, v = random_targets(n, n_q * per, g)
    q_rel = (torch.arange(n_q) % 5).int()
    return z, w, known, q_rel, torch.arange(n_q + 1, dtype=torch.int64) * per, u, v


def routes_case(n=645, dim=16, per=300):
    g = torch.Generator().manual_seed(645)
    z, w = exact_zw(n, dim, 5, g)
    known = keys_from_pairs(graph_known(n, g), n)
    u, v = random_targets(n, 5 * per, g)
    return z, w, known, torch.arange(5, dtype=torch.int32), torch.arange(6, dtype=torch.int64) * per, u, v


def search_case(n=3000, dim=128, n_rel=3, n_known=30000, per=500):
    """n^2 bits do not fit LDS: the binary-search filter; half of each relation's targets are listed pairs"""
    g = torch.Generator().manual_seed(3000)
    z, w = exact_zw(n, dim, n_rel, g)
    keys, ptr, tu, tv = [], [0], [], []
    for r in range(n_rel):
        a, b = torch.randint(0, n, (n_known,), generator=g), torch.randint(0, n, (n_known,), generator=g)
        ks = torch.unique(a[a != b] * n + b[a != b])
        keys.append(ks)
        ptr.append(ptr[-1] + ks.numel())
        u, v = random_targets(n, per - per // 2, g)
        pick = ks[torch.randperm(ks.numel(), generator=g)[:per // 2]]
        tu += [u, (pick % n).int()]                                       # listed as (key // n, key % n): asked in reverse
        tv += [v, (pick // n).int()]
    known = (torch.cat(keys), torch.tensor(ptr, dtype=torch.int64))
    return (z, w, known, torch.arange(n_rel, dtype=torch.int32), torch.arange(n_rel + 1, dtype=torch.int64) * per,
            torch.cat(tu), torch.cat(tv))
