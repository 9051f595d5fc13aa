"""Inputs of the exact screen tests (include/tipk.h section 4c), as host tensors: tests/test_host_screen_cases.py asserts for
each that the kernel's fp32 logits equal the fp64 ones and that the case reaches the edge it aims at,
tests/test_gpu_screen_edges.py runs them on the device against `screen_spec.exact_screen` with no tolerance.

A case is Case(z, w, known, queries, k, note): known = (keys, ptr) or None, queries a list of (relation, drug | -1), note the
edge it aims at.  `ids(group)` lists the cases of a group ('a' .. 'i'), `case(id)` builds one (cached; nobody writes into it).
The kernel's constants that the groups aim at are restated below; tests/test_host_screen_cases.py holds them to the library."""
import functools
from collections import namedtuple

import torch

from screen_rank_cases import EDGE_N, exact_zw, graph_known
from screen_spec import keys_from_pairs

Case = namedtuple('Case', 'z w known queries k note')

# restated from tip_amd/csrc/tipk_wg_topk.h and tipk_screen.hip
TILE, SPLIT_MAX, TARGET_WG, MERGE_G = 64, 64, 4096, 8
DBLK, CAP, ROUND = 256, 2048, 1024

KS = (1, 37, 1024)


def tiles(n):
    nb = (n + TILE - 1) // TILE
    return nb * (nb + 1) // 2


def splits(n, n_q):
    """wg_splits: parts per query"""
    return max(1, min(SPLIT_MAX, TARGET_WG // n_q if n_q > 0 else 1, tiles(n)))


def coarse_zw(n, dim, n_rel, g):
    """z and w in {-1, 0, 1}: with dim 4 the logits take nine values, so every cut runs through a run of ties"""
    z = torch.randint(-1, 2, (n, dim), generator=g).float()
    w = torch.randint(-1, 2, (n_rel, dim), generator=g).float()
    return z, w


def _inside(lists, n):
    """graph_known names drugs 1, 2, 3 and 7: below n = 8 only the pairs the graph has"""
    return [[(a, b) for a, b in pairs if a < n and b < n] for pairs in lists]


def sparse_pairs(n, g, frac, flip=True):
    """~frac of the pairs u < v, listed in one direction only (larger id first when flip)"""
    iu = torch.triu_indices(n, n, 1)
    m = torch.rand(iu.shape[1], generator=g) < frac
    a, b = iu[0][m].tolist(), iu[1][m].tolist()
    return list(zip(b, a)) if flip else list(zip(a, b))


def _graph_queries(n):
    """every relation query of the five graph_known relations; drug queries on drugs 0, n - 1 and 7 under a sparse list, a
    two-direction list and the relation that lists every partner of drug 7"""
    q = [(r, -1) for r in range(5)]
    for du in sorted({0, n - 1, 7}):
        if du < n:
            q += [(0, du), (1, du), (4, du)]
    return q


# ------------------------------------------------------------------ a. tile and size edges
def _case_a(n, k):
    g = torch.Generator().manual_seed(4000 + n)
    z, w = exact_zw(n, 16, 5, g)
    known = keys_from_pairs(_inside(graph_known(n, g), n), n)
    return Case(z, w, known, _graph_queries(n), k, 'n = %d at the edges of the 64-row tile, k = %d' % (n, k))


# ------------------------------------------------------------------ b. width edges
B_DIMS = (4, 32, 36, 64, 128, 252, 256)


def _case_b(dim):
    n = 130
    g = torch.Generator().manual_seed(4100 + dim)
    z, w = exact_zw(n, dim, 5, g)
    known = keys_from_pairs(graph_known(n, g), n)
    return Case(z, w, known, _graph_queries(n), 37, 'dim = %d: chunks of 32 columns, the last one %d wide' % (dim, (dim - 1) % 32 + 1))


# ------------------------------------------------------------------ c. drug-block edges
C_N = (255, 256, 257, 512, 513)


def _c_graph(n):
    """relation 0: a sparse one-direction list; relation 1: every partner of drug 0 (half of them reversed); relation 2: no
    list"""
    g = torch.Generator().manual_seed(4200 + n)
    z, w = exact_zw(n, 8, 3, g)
    every = [(0, v) if v % 2 else (v, 0) for v in range(1, n)]
    return z, w, keys_from_pairs([sparse_pairs(n, g, 0.1), every, []], n)


def c_drugs(n):
    return sorted({d for d in (0, 255, 256, n - 1) if d < n})


def _c_alone(n):
    """(relation, drug) sent as one query alone: drug 0 with every partner listed and under the sparse list, then the other
    drugs under the sparse list and under no list in turn"""
    return [(1, 0), (0, 0)] + [((0, 2)[i % 2], d) for i, d in enumerate(c_drugs(n)[1:])]


def _case_c(n, which):
    z, w, known = _c_graph(n)
    if which == 'eight':
        ds = c_drugs(n)
        q = [(0, d) for d in ds] + [(2, d) for d in ds] + [(1, 0), (1, ds[-1])]
        q = (q + q)[:8]
        return Case(z, w, known, q, 1024, 'n = %d: eight drug queries together, k above the %d partners' % (n, n - 1))
    q = _c_alone(n)[int(which)]
    return Case(z, w, known, [q], 37, 'n = %d: the drug query %r alone, %d blocks of 256 partners for %d parts'
                % (n, q, (n + DBLK - 1) // DBLK, splits(n, 1)))


# ------------------------------------------------------------------ d. ties that straddle the cut
D_N = (65, 200)


def _case_d(n, k, zero):
    g = torch.Generator().manual_seed(4300 + n)
    z, w = coarse_zw(n, 4, 5, g)
    if zero:
        # every logit is 0: the answer is the k smallest unfiltered keys (relation 0: a sparse one-direction list; relation 1:
        # no list) and the k smallest partners of a drug
        z = torch.zeros_like(z)
        known = keys_from_pairs([sparse_pairs(n, g, 0.15), [], [], [], []], n)
        q = [(0, -1), (1, -1), (0, 0), (1, n - 1), (0, n // 2)]
        return Case(z, w, known, q, k, 'n = %d, z = 0: every logit ties, k = %d' % (n, k))
    known = keys_from_pairs(graph_known(n, g), n)
    return Case(z, w, known, _graph_queries(n), k, 'n = %d, nine logit values, k = %d' % (n, k))


# ------------------------------------------------------------------ e. buffer pressure
E_N = 129
E_KS = (1, 1023, 1024)


def _e_graph():
    """z[i] = (i + 1, 0, 0, 0): the logit of (u, v) is +-(u + 1)(v + 1), exact, with ties such as 2 * 6 = 3 * 4.  Relations 0 and
    1: w = (+1, 0, 0, 0) and (-1, 0, 0, 0) without a list -- under + the logits rise with the key inside a row, so a row's
    later candidates keep passing the threshold; under - they fall.  Relations 2 and 3: the same with a sparse list.
    Relation 4: w = 0, no list -- every logit is 0 and passes the threshold (0 >= 0), which fills the buffer to CAP in
    every round of a full tile."""
    n = E_N
    g = torch.Generator().manual_seed(4400)
    z = torch.zeros(n, 4)
    z[:, 0] = torch.arange(1, n + 1).float()
    w = torch.zeros(5, 4)
    w[:, 0] = torch.tensor([1.0, -1.0, 1.0, -1.0, 0.0])
    sp = sparse_pairs(n, g, 0.15)
    return z, w, keys_from_pairs([[], [], sp, sp, []], n)


def _case_e(which):
    n = E_N
    if which == 'edge':
        # One part = the full tile (0, 1): rows u = 4 ty + i < 64 meet v in 64..127, round i takes the rows u % 4 == i.
        # Round 0 appends 1 024 entries (c = CAP - ROUND: no cut); in round 1 every pair is listed but (1, 100), so c becomes
        # CAP - ROUND + 1 and the buffer MUST be cut now; round 2 (logit 3 against a threshold of 1) appends 1 024 again.
        z = torch.zeros(n, 4)
        z[:, 0] = 1.0
        z[2:64:4, 0] = 3.0
        w = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
        listed = [(u, v) for u in range(1, 64, 4) for v in range(64, 128) if (u, v) != (1, 100)]
        return Case(z, w, keys_from_pairs([listed], n), [(0, -1)], 1024,
                    'c = CAP - ROUND + 1 at the end of a round, a full round next')
    z, w, known = _e_graph()
    if which == 'walk':
        # 2 049 queries: one part per query walks all six tiles with its threshold
        q = [(i % 5, -1) for i in range(2049)]
        return Case(z, w, known, q, 1024, 'one part walks every tile of n = 129 with k = 1 024')
    k = int(which)
    q = [(r, -1) for r in range(5)] + [(0, 0), (1, n - 1), (2, 64), (3, 7), (4, 100)]
    return Case(z, w, known, q, k, 'rising and falling logits and an all-zero relation, k = %d' % k)


# ------------------------------------------------------------------ f. split and merge levels
F_CASES = {        # id -> (n, n_q, k, parts per query)
    'f-200-1': (200, 1, 300, 10),           # two merge levels, groups of 8 + 2
    'f-200-455': (200, 455, 8, 9),          # 8 + 1
    'f-200-512': (200, 512, 8, 8),          # one level, a full group
    'f-200-2049': (200, 2049, 8, 1),        # one part walks all ten tiles; no merge of parts
    'f-700-1': (700, 1, 300, 64),           # eight full groups
}


def _case_f(cid):
    n, n_q, k, s = F_CASES[cid]
    g = torch.Generator().manual_seed(4500 + n)
    z, w = coarse_zw(n, 4, 5, g)
    if n == 200:
        known = keys_from_pairs(graph_known(n, g), n)
    else:
        known = keys_from_pairs([sparse_pairs(n, g, 0.1), [], [], [], []], n)
    q = [(i % 5, -1) for i in range(n_q)]
    return Case(z, w, known, q, k, 'n = %d, %d relation queries: %d parts per query' % (n, n_q, s))


# ------------------------------------------------------------------ g. filter routes
def _case_g(n):
    """relation 0: random keys, the pairs (0, 1) and (n-2, n-1) in reversed orientation ONLY, and a self key; relation 1: an
    empty block between two full ones; relation 2: random keys"""
    g = torch.Generator().manual_seed(4600 + n)
    z, w = exact_zw(n, 16, 3, g)
    skip = {(0, 1), (1, 0), (n - 2, n - 1), (n - 1, n - 2)}
    r0 = [p for p in sparse_pairs(n, g, 0.05, flip=False) if p not in skip] + [(1, 0), (n - 1, n - 2), (5, 5)]
    r2 = [p for p in sparse_pairs(n, g, 0.05) if p not in skip]
    q = [(0, -1), (1, -1), (2, -1), (0, 0), (0, 1), (0, n - 1), (0, n - 2), (0, 5), (1, 3), (2, n - 1)]
    return Case(z, w, keys_from_pairs([r0, [], r2], n), q, 100, 'n = %d: n^2 bits %s 64 KB' % (n, 'fit' if n <= 724 else 'exceed'))


# ------------------------------------------------------------------ h. top of the key range
H_N = 46340


def _case_h():
    """Drug queries only (the reference of a relation query would be an n x n matrix).  Drugs n-1 and n-2 are made the best
    pair of relation 0 and drug n-1 the best partner of drug 0 under relation 1, so keys next to n^2 - 1 are returned."""
    n = H_N
    g = torch.Generator().manual_seed(4700)
    z, w = exact_zw(n, 4, 2, g)
    w[w == 0] = 0.5
    z[n - 1] = 2.0 * torch.sign(w[0])
    z[n - 2] = 2.0
    z[0] = 2.0 * torch.sign(w[1]) * torch.sign(z[n - 1])
    known = keys_from_pairs([[(n - 1, 3), (17, n - 1), (n - 1, n - 3), (40000, n - 1)], [(0, 1), (n - 2, 0), (0, 23170)]], n)
    return Case(z, w, known, [(0, n - 1), (1, 0)], 100, 'n = 46 340: keys up to n^2 - 1 < 2^31')


# ------------------------------------------------------------------ i. NaN and infinities
I_N, I_NAN, I_INF = 70, 11, 20


def _case_i():
    """w = (1, 0, 0, 0) for both relations; z[:, 0] in {-2, 0, 2}.  Drug 11's row is NaN: every pair with it has a NaN logit.
    Drug 20's row is (3e38, 0, 0, 0): its logits are +inf, -inf or 0 by the sign of the partner's first coordinate.
    Relation 0 lists two thirds of the ordinary pairs, so that k = 1 024 reaches the -inf entries and the padding behind them;
    relation 1 has no list."""
    n = I_N
    g = torch.Generator().manual_seed(4800)
    z, _ = exact_zw(n, 4, 1, g)
    z[:, 0] = 2.0 * torch.randint(-1, 2, (n,), generator=g).float()
    z[I_NAN] = float('nan')
    z[I_INF] = torch.tensor([3e38, 0.0, 0.0, 0.0])
    w = torch.tensor([[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    listed = [(v, u) for u in range(n) for v in range(u + 1, n) if I_INF not in (u, v) and (u + v) % 3]
    q = [(0, -1), (1, -1), (0, I_INF), (1, I_INF), (0, I_NAN), (0, 0), (1, 69)]
    return Case(z, w, keys_from_pairs([listed, []], n), q, 1024, 'a NaN row and a row whose logits are +-inf')


# ------------------------------------------------------------------ the table
_TABLE = {}
for _n in EDGE_N:
    for _k in KS:
        _TABLE['a-%d-%d' % (_n, _k)] = functools.partial(_case_a, _n, _k)
for _d in B_DIMS:
    _TABLE['b-%d' % _d] = functools.partial(_case_b, _d)
for _n in C_N:
    for _w in [str(_i) for _i in range(len(_c_alone(_n)))] + ['eight']:
        _TABLE['c-%d-%s' % (_n, _w)] = functools.partial(_case_c, _n, _w)
for _n in D_N:
    for _k in KS:
        _TABLE['d-%d-%d' % (_n, _k)] = functools.partial(_case_d, _n, _k, False)
        _TABLE['d-%d-%d-zero' % (_n, _k)] = functools.partial(_case_d, _n, _k, True)
for _w in [str(_k) for _k in E_KS] + ['walk', 'edge']:
    _TABLE['e-%s' % _w] = functools.partial(_case_e, _w)
for _c in F_CASES:
    _TABLE[_c] = functools.partial(_case_f, _c)
_TABLE['g-724'] = functools.partial(_case_g, 724)
_TABLE['g-725'] = functools.partial(_case_g, 725)
_TABLE['g-724-search'] = functools.partial(_case_g, 724)             # the same input under option "screen_search"
_TABLE['h'] = _case_h
_TABLE['i'] = _case_i


def ids(group=None):
    return [c for c in _TABLE if group is None or c.split('-')[0] == group]


@functools.lru_cache(maxsize=None)
def case(cid):
    return _TABLE[cid]()
