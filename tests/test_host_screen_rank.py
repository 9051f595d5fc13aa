"""CPU tests of the screen rank (include/tipk.h section 4h): the bound symbols and the `_supported` / `_workspace_bytes` /
`_chunk` queries, argument validation of the C entry (every refusal happens before anything touches a device, so bogus
device pointers are safe here), the Python surface's refusals, `ops.targets_by_relation`, self-tests of the fp64 spec
(tests/screen_rank_spec.py) on hand-worked graphs, and the proof that the device tests' inputs leave no room for a
tolerance: for every case of tests/screen_rank_cases.py the fp32 arithmetic of the kernel equals fp64 exactly."""
import ctypes
import math
import types

import pytest
import torch

import screen_rank_cases as cases
from screen_rank_spec import dense_screen_rank, emulated_fp32_logits, on_exact_grid, spec_screen_rank
from screen_spec import keys_from_pairs
from tip_amd import _lib, ops

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _call(n=10, dim=16, n_rel=3, n_q=4, n_tgt=6, keys=None, kptr=None, z=FAKE, w=FAKE, qr=FAKE, tptr=FAKE, tu=FAKE, tv=FAKE,
          out=FAKE, logit=FAKE, ws=None):
    return _lib.lib().tipk_distmult_screen_rank(z, n, dim, w, n_rel, qr, n_q, tptr, tu, tv, n_tgt, keys, kptr, out, logit, ws,
                                                None)


def test_symbols_and_queries():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30
    for name in ('tipk_distmult_screen_rank', 'tipk_distmult_screen_rank_supported',
                 'tipk_distmult_screen_rank_workspace_bytes', 'tipk_distmult_screen_rank_chunk'):
        assert hasattr(L, name), name
    sup, wsb = L.tipk_distmult_screen_rank_supported, L.tipk_distmult_screen_rank_workspace_bytes
    assert sup(1, 4, 1) == 1 and sup(46340, 256, 65536) == 1
    assert sup(0, 16, 4) == 0 and sup(46341, 16, 4) == 0
    assert sup(645, 4, 4) == 1 and sup(645, 6, 4) == 0 and sup(645, 256, 4) == 1 and sup(645, 260, 4) == 0
    assert sup(645, 0, 4) == 0 and sup(645, 2, 4) == 0
    assert sup(645, 16, 65536) == 1 and sup(645, 16, 65537) == 0 and sup(645, 16, 0) == 0
    assert wsb(645, 16, 1097, 925000) >= 0 and wsb(645, 16, 0, 0) >= 0
    assert wsb(46341, 16, 1, 4) == -1 and wsb(645, 6, 1, 4) == -1 and wsb(645, 260, 1, 4) == -1
    assert wsb(645, 16, -1, 4) == -1 and wsb(645, 16, 1, -4) == -1
    assert L.tipk_distmult_screen_rank_chunk() >= 64


def test_bad_arguments_einval():
    assert _call(n_q=-1) == EINVAL
    assert _call(n_tgt=-1) == EINVAL
    assert _call(n=0) == EINVAL
    assert _call(n_rel=0) == EINVAL
    assert _call(dim=0) == EINVAL and _call(dim=-4) == EINVAL
    assert _call(keys=FAKE) == EINVAL                                     # keys without offsets, and the reverse
    assert _call(kptr=FAKE) == EINVAL
    for name in ('z', 'w', 'qr', 'tptr', 'tu', 'tv', 'out'):
        assert _call(**{name: None}) == EINVAL, name
    assert _call(n_tgt=-1, n=46341) == EINVAL                             # argument errors come before shape limits
    assert _call(n_q=-1, dim=6) == EINVAL
    assert _call(keys=FAKE, n_rel=65537) == EINVAL
    if _lib.lib().tipk_distmult_screen_rank_workspace_bytes(10, 16, 4, 6) > 0:
        assert _call(ws=None) == EINVAL


def test_unsupported_shapes_and_empty_lists():
    ws = FAKE
    assert _call(dim=6, ws=ws) == EUNSUPPORTED
    assert _call(dim=260, ws=ws) == EUNSUPPORTED
    assert _call(n=46341, ws=ws) == EUNSUPPORTED
    assert _call(n_rel=65537, ws=ws) == EUNSUPPORTED
    assert _call(z=ctypes.c_void_p((1 << 20) + 4), ws=ws) == EUNSUPPORTED    # z must be 16-byte aligned
    assert _call(n_q=0, ws=ws) == 0 and _call(n_tgt=0, ws=ws) == 0           # nothing to rank: nothing launched
    assert _call(n_tgt=0, z=None, qr=None, tu=None, out=None) == 0
    assert _call(n_q=0, w=None, tptr=None, tv=None, out=None) == 0
    assert _call(n_q=0, keys=FAKE, kptr=FAKE, ws=ws) == 0
    assert _call(logit=None, n_tgt=0, ws=ws) == 0                           # out_logit is optional


def test_ops_refuse_cpu_tensors():
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_screen_rank(torch.ones(5, 4), torch.ones(2, 4), torch.tensor([0, 1]), torch.tensor([0, 1, 2]),
                                 torch.tensor([0, 1]), torch.tensor([2, 3]))


def test_tip_rank_pairs_refusals():
    from tip_amd.layers import TIP
    triples = (torch.tensor([[0], [1]]), torch.tensor([2]))
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.rank_pairs(types.SimpleNamespace(decoder_kind='nn', shard=None), triples)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.rank_pairs(types.SimpleNamespace(decoder_kind='distmult', shard=object()), triples)
    for bad in ('test', 'none', 0):
        with pytest.raises(ValueError, match='filter'):
            TIP.rank_pairs(types.SimpleNamespace(decoder_kind='distmult', shard=None), triples, filter=bad)
    me = types.SimpleNamespace(decoder_kind='distmult', shard=None, embeddings=torch.zeros(5, 4),
                               data=types.SimpleNamespace(n_drug=5, n_dd_et=3))
    for idx in ([[0], [5]], [[-1], [1]]):
        with pytest.raises(ValueError, match='drug id out of range'):
            TIP.rank_pairs(me, (torch.tensor(idx), torch.tensor([2])), filter=None)
    for et in (3, -1):
        with pytest.raises(ValueError, match='side-effect id out of range'):
            TIP.rank_pairs(me, (torch.tensor([[0], [1]]), torch.tensor([et])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_pairs(me, (torch.tensor([[0.0], [1.0]]), torch.tensor([2])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_pairs(me, (torch.tensor([[0], [1]]), torch.tensor([2.0])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_pairs(me, (torch.tensor([0, 1]), torch.tensor([2])), filter=None)


# ------------------------------------------------------------------ targets_by_relation
def test_targets_by_relation_vs_dict():
    ei = torch.tensor([[0, 1, 0, 6, 0, 3, 1, 0],
                       [1, 0, 2, 6, 1, 2, 0, 1]])
    et = torch.tensor([4, 4, 2, 0, 4, 1, 7, 4])
    q_rel, ptr, tu, tv, order = ops.targets_by_relation(ei, et, 9)
    want = {}
    for i, (u, v, r) in enumerate(zip(ei[0].tolist(), ei[1].tolist(), et.tolist())):
        want.setdefault(r, []).append((u, v, i))
    rels = sorted(want)
    assert q_rel.tolist() == rels == [0, 1, 2, 4, 7]                      # only relations that have triples, ascending
    assert ptr.tolist() == [0, 1, 2, 3, 7, 8]
    assert list(zip(tu.tolist(), tv.tolist())) == [(u, v) for r in rels for u, v, _ in want[r]]   # the given orientation
    assert order.tolist() == [i for r in rels for _, _, i in want[r]]
    assert q_rel.dtype == torch.int32 and ptr.dtype == torch.int64 and tu.dtype == torch.int32 and tv.dtype == torch.int32
    back = torch.empty((2, 8), dtype=torch.int64)                         # the round trip: grouped results to the given order
    back[0, order], back[1, order] = tu.long(), tv.long()
    assert torch.equal(back, ei)
    rel = torch.empty(8, dtype=torch.int64)
    rel[order] = torch.repeat_interleave(q_rel.long(), ptr[1:] - ptr[:-1])
    assert torch.equal(rel, et)
    e = ops.targets_by_relation(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 9)
    assert e[0].numel() == 0 and e[1].tolist() == [0] and e[2].numel() == 0 and e[3].numel() == 0 and e[4].numel() == 0
    with pytest.raises(_lib.TipkError):
        ops.targets_by_relation(ei.float(), et, 9)
    with pytest.raises(_lib.TipkError):
        ops.targets_by_relation(ei, et[:-1], 9)


def test_targets_by_relation_random():
    g = torch.Generator().manual_seed(5)
    T = 400
    ei, et = torch.randint(0, 11, (2, T), generator=g), torch.randint(0, 9, (T,), generator=g)
    q_rel, ptr, tu, tv, order = ops.targets_by_relation(ei, et, 9)
    assert bool((q_rel[1:] > q_rel[:-1]).all()) and int(ptr[-1]) == T and sorted(order.tolist()) == list(range(T))
    owner = torch.repeat_interleave(torch.arange(q_rel.numel()), ptr[1:] - ptr[:-1])
    assert torch.equal(et[order].int(), q_rel[owner])
    assert torch.equal(ei[0][order].int(), tu) and torch.equal(ei[1][order].int(), tv)
    same = owner[1:] == owner[:-1]
    assert bool((order[1:] > order[:-1])[same].all())                     # stable inside a query


# ------------------------------------------------------------------ the spec on hand-worked graphs
def _line_graph():
    """n = 3, dim = 1, z = (1, 2, 3), w = 1: logits (0,1) = 2, (0,2) = 3, (1,2) = 6 (tests/test_host_screen.py)."""
    return torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[1.0]])


def _both(z, w, q_rel, ptr, tu, tv, known=None):
    """the loop spec and the dense one must agree wherever both run"""
    r, s = spec_screen_rank(z, w, q_rel, ptr, tu, tv, known)
    r2, s2 = dense_screen_rank(z, w, q_rel, ptr, tu, tv, known, row_chunk=2)
    assert torch.equal(r, r2) and torch.equal(s.isnan(), s2.isnan()) and torch.equal(s.nan_to_num(), s2.nan_to_num())
    return r, s


def test_spec_ranks_on_the_line_graph():
    z, w = _line_graph()
    r, s = _both(z, w, [0], [0, 3], [1, 0, 1], [2, 2, 0])
    assert r.tolist() == [1, 2, 3] and s.tolist() == [6.0, 3.0, 2.0]
    r, s = _both(z, w, [0], [0, 4], [2, 2, 0, 2], [1, 0, 1, 1])           # reversed orientation and a repeat: the same pair
    assert r.tolist() == [1, 2, 3, 1] and s.tolist() == [6.0, 3.0, 2.0, 6.0]


def test_spec_known_pairs():
    z, w = _line_graph()
    known = keys_from_pairs([[(2, 1)]], 3)                               # listed as (2, 1): (1, 2) leaves the candidate set
    r, s = _both(z, w, [0], [0, 3], [1, 0, 0], [2, 2, 1], known)
    # the listed target is still ranked (nothing is better than 6), and it no longer stands above the other two
    assert r.tolist() == [1, 1, 2] and s.tolist() == [6.0, 3.0, 2.0]
    r, _ = _both(z, w, [0], [0, 1], [0], [1], keys_from_pairs([[(0, 2), (2, 0), (1, 2)]], 3))
    assert r.tolist() == [1]
    # keys outside [0, n^2) are ignored; a list of another relation filters nothing
    r, _ = _both(z, w, [0], [0, 1], [0], [1], (torch.tensor([-5, 9, 40]), torch.tensor([0, 3])))
    assert r.tolist() == [3]
    w2 = torch.tensor([[1.0], [1.0]])
    r, _ = _both(z, w2, [0, 1], [0, 1, 2], [0, 0], [1, 1], keys_from_pairs([[], [(1, 2), (0, 2)]], 3))
    assert r.tolist() == [3, 1]


def test_spec_ties_by_key_and_unranked():
    ones, w = torch.ones(4, 2), torch.ones(1, 2)                          # every logit 2: ranks follow the key a*n+b
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    r, s = _both(ones, w, [0], [0, 6], [p[1] for p in pairs], [p[0] for p in pairs])
    assert r.tolist() == [1, 2, 3, 4, 5, 6] and s.tolist() == [2.0] * 6
    r, _ = _both(ones, w, [0], [0, 2], [2, 1], [3, 3], keys_from_pairs([[(2, 0)]], 4))    # (0, 2) is no candidate
    assert r.tolist() == [5, 4]
    # a self pair, ids outside [0, n), a relation outside [0, n_rel): (0, NaN); tgt_ptr is clamped to the list
    z, w1 = _line_graph()
    r, s = _both(z, w1, [0, 1, -1, 0], [0, 4, 5, 6, 99], [1, -1, 0, 3, 0, 0, 1], [1, 0, 3, 0, 1, 1, 2])
    assert r.tolist() == [0, 0, 0, 0, 0, 0, 1] and bool(s[:6].isnan().all()) and s[6] == 6.0


def test_spec_nan_row():
    z = torch.tensor([[1.0], [float('nan')], [3.0], [2.0]])              # pairs of drug 1 are NaN; (0,2) = 3, (0,3) = 2, (2,3) = 6
    w = torch.tensor([[1.0]])
    r, s = _both(z, w, [0], [0, 4], [0, 1, 3, 0], [2, 2, 2, 3])
    assert r.tolist() == [2, 0, 1, 3] and math.isnan(s[1]) and s[[0, 2, 3]].tolist() == [3.0, 6.0, 2.0]


def test_dense_spec_matches_loop_spec_on_a_case():
    z, w, known, q_rel, ptr, tu, tv = cases.small_case(24, 4)
    r, s = _both(z, w, q_rel, ptr, tu, tv, known)
    assert int((r > 0).sum()) > 100 and int((r == 0).sum()) >= 120         # two whole queries are outside the relations
    assert r[int(ptr[3]):int(ptr[4])].max() == 1                           # relation 3: every pair known, nothing competes


# ------------------------------------------------------------------ the inputs leave no room for a tolerance
def _assert_exact(z, w, rows=None):
    assert on_exact_grid(z, w)
    zf = torch.nan_to_num(z)
    pick = None if rows is None or rows >= z.shape[0] else torch.linspace(0, z.shape[0] - 1, rows).long()
    for r in range(w.shape[0]):
        a64 = zf.double() * w[r].double()
        if pick is not None:
            a64 = a64[pick]
        assert torch.equal(emulated_fp32_logits(zf, w, r, pick).double(), a64 @ zf.double().t())


def test_case_inputs_are_exact_in_fp32():
    for n, dim in cases.SMALL:
        _assert_exact(*cases.small_case(n, dim)[:2])
    for n in cases.EDGE_N:
        _assert_exact(*cases.all_pairs_case(n)[:2])
    _assert_exact(*cases.nan_case()[0][:2])
    _assert_exact(*cases.chunk_case(10)[:2])
    _assert_exact(*cases.single_query_case()[:2], rows=48)
    _assert_exact(*cases.many_queries_case()[:2])
    _assert_exact(*cases.routes_case()[:2], rows=48)
    _assert_exact(*cases.search_case()[:2], rows=16)


def test_exact_grid_is_rich_in_ties():
    """n = 300, dim = 128: a few thousand distinct logits over 44 850 pairs, fp32 == fp64 everywhere."""
    g = torch.Generator().manual_seed(300)
    z, w = cases.exact_zw(300, 128, 1, g)
    _assert_exact(z, w)
    L = (z.double() * w[0].double()) @ z.double().t()
    distinct = torch.unique(L[torch.triu(torch.ones(300, 300, dtype=torch.bool), 1)]).numel()
    assert 1000 < distinct < 10000, distinct
