"""-m gpu: `tipk_distmult_screen_rank` (include/tipk.h section 4h) and `TIP.rank_pairs`.  The inputs of the main cases
(tests/screen_rank_cases.py) are exactly representable -- tests/test_host_screen_rank.py shows fp32 == fp64 for each -- so
ranks and logits are held to the fp64 spec `dense_screen_rank` with NO tolerance.  The cases with real rounding are held
bitwise to the existing screen (`ops.distmult_screen`, `TIP.screen`): an unlisted target sits at index rank - 1 of the
relation's list with identical logit bits, and for a listed one rank - 1 is the number of list entries better than it."""
import os

import pytest
import torch

import screen_rank_cases as cases
from screen_rank_spec import dense_screen_rank, known_mask
from screen_spec import keys_from_pairs
from tip_amd import _lib, ops, utils

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(case):
    z, w, known, q_rel, ptr, tu, tv = case
    known = None if known is None else (known[0].to(DEV), known[1].to(DEV))
    return z.to(DEV), w.to(DEV), known, q_rel.to(DEV), ptr.to(DEV), tu.to(DEV), tv.to(DEV)


def _run(case):
    z, w, known, q_rel, ptr, tu, tv = case
    return ops.distmult_screen_rank(z, w, q_rel, ptr, tu, tv, known)


def _check_exact(case, got=None):
    """ranks and logits equal the fp64 spec exactly; -> (rank, logit) of the kernel"""
    z, w, known, q_rel, ptr, tu, tv = case
    rank, logit = _run(case) if got is None else got
    want_r, want_s = dense_screen_rank(z, w, q_rel, ptr, tu, tv, known)
    assert rank.dtype == torch.int32 and logit.dtype == torch.float32 and rank.shape == tu.shape == logit.shape
    assert torch.equal(rank.long(), want_r), 'ranks: %d of %d differ' % (int((rank.long() != want_r).sum()), rank.numel())
    assert torch.equal(logit.isnan(), want_s.isnan()) and torch.equal(logit.isnan(), rank == 0)
    assert torch.equal(logit.double().nan_to_num(), want_s.nan_to_num()), 'logits'
    return rank, logit


@pytest.mark.parametrize('n,dim', cases.SMALL)
def test_small_exact_graphs(n, dim):
    case = _dev(cases.small_case(n, dim))
    z, w, known, q_rel, ptr, tu, tv = case
    rank, logit = _check_exact(case)
    p = ptr.tolist()
    assert int(rank[p[5]:p[7]].abs().sum()) == 0                          # the queries of relations -1 and n_rel
    assert p[7] == p[8] and int((rank[p[8]:] > 0).sum()) > 40             # the empty query; the second query on relation 0
    assert int(rank[p[3]:p[4]].max()) == 1                                # relation 3: every pair known, nothing competes
    # (u, v) and (v, u): the same rank and the same logit bits
    r2, s2 = ops.distmult_screen_rank(z, w, q_rel, ptr, tv, tu, known)
    assert torch.equal(r2, rank) and torch.equal(s2.view(torch.int32), logit.view(torch.int32))
    # out_logit = NULL is accepted
    out = torch.full_like(rank, -7)
    st = _lib.lib().tipk_distmult_screen_rank(_lib.ptr(z), n, dim, _lib.ptr(w), w.shape[0], _lib.ptr(q_rel), q_rel.numel(),
                                              _lib.ptr(ptr), _lib.ptr(tu), _lib.ptr(tv), tu.numel(), _lib.ptr(known[0]),
                                              _lib.ptr(known[1]), _lib.ptr(out), None, None, _lib.stream_ptr(z.device))
    assert st == 0 and torch.equal(out, rank)


@pytest.mark.parametrize('n', cases.EDGE_N)
def test_tile_and_size_edges_all_pairs(n):
    case = _dev(cases.all_pairs_case(n))
    rank, _ = _check_exact(case)
    m = n * (n - 1) // 2
    assert rank.numel() == 2 * m
    if m:
        assert sorted(rank[m:].tolist()) == list(range(1, m + 1))         # no list: the ranks are a permutation


def test_nan_row():
    with_nan, without = cases.nan_case()
    row = 11
    case = _dev(with_nan)
    rank, logit = _check_exact(case)
    touch = (case[5] == row) | (case[6] == row)
    assert int(touch.sum()) > 20 and int(rank[touch].abs().sum()) == 0 and bool(logit[touch].isnan().all())
    # every other rank is that of the graph without the drug's pairs as candidates
    ref_r, ref_s = _check_exact(_dev(without))
    assert torch.equal(rank[~touch], ref_r[~touch]) and torch.equal(logit[~touch], ref_s[~touch])
    assert int((rank[~touch] > 0).sum()) == int((~touch).sum())


def test_chunk_passes():
    c = _lib.lib().tipk_distmult_screen_rank_chunk()
    assert c >= 64
    for count in (c - 1, c, c + 1, 2 * c + 3):
        _check_exact(_dev(cases.chunk_case(count)))


def test_single_query_64_parts():
    _check_exact(_dev(cases.single_query_case()))


def test_many_queries_one_part_each():
    _check_exact(_dev(cases.many_queries_case()))


def test_routes_identical_and_repeatable():
    case = _dev(cases.routes_case())
    assert _lib.lib().tipk_distmult_screen_bitmap_route(645) == 1
    a = _run(case)
    b = _run(case)
    _lib.set_option('screen_search', 1)
    try:
        assert _lib.lib().tipk_distmult_screen_bitmap_route(645) == 0
        c = _run(case)
    finally:
        _lib.set_option('screen_search', 0)
    for x, y, name in zip(a, b, ('rank', 'logit')):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), 'run to run: ' + name
    for x, y, name in zip(a, c, ('rank', 'logit')):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), 'bitmap vs search route: ' + name
    _check_exact(case, a)


def test_search_route_at_scale():
    case = _dev(cases.search_case())
    assert _lib.lib().tipk_distmult_screen_bitmap_route(3000) == 0
    rank, _ = _check_exact(case)
    assert int((rank > 0).sum()) == rank.numel()


def _check_against_screen(rank, logit, rel, tu, tv, n, lists, known, what):
    """lists = (score [R, k], u [R, k], v [R, k]) of the relation queries under `known`; rank, logit, rel, tu, tv [T].
    Every target with rank <= k: unlisted -> it sits at index rank - 1 with identical logit bits; listed -> rank - 1 is the
    number of list entries better than (its logit, key)."""
    score, lu, lv = lists
    k = score.shape[1]
    a, b = torch.minimum(tu, tv).long(), torch.maximum(tu, tv).long()
    key = a * n + b
    lkey = lu.long() * n + lv.long()
    seen = 0
    for r in torch.unique(rel).tolist():
        km = known_mask(known, r, n, DEV)
        sel = (rel == r) & (rank > 0) & (rank <= k)
        listed = km[a, b] & sel
        free = sel & ~listed
        at = (rank[free] - 1).long()
        assert torch.equal(lkey[r][at], key[free]), (what, r, 'an unlisted target is not at index rank - 1')
        assert torch.equal(score[r][at].view(torch.int32), logit[free].view(torch.int32)), (what, r, 'logit bits')
        valid = lu[r] >= 0
        s, kk = logit[listed], key[listed]
        beats = valid[None, :] & ((score[r][None, :] > s[:, None]) | ((score[r][None, :] == s[:, None]) & (lkey[r][None, :] < kk[:, None])))
        cnt = beats.sum(1)
        inside = cnt < k                                                  # k better entries: the list cannot tell the rank
        assert torch.equal(cnt[inside], (rank[listed] - 1).long()[inside]), (what, r, 'a listed target')
        seen += int(free.sum()) + int(inside.sum())
    return seen


def test_real_rounding_bitwise_against_the_screen():
    n, dim, k = 40, 16, 1024
    g = torch.Generator().manual_seed(40)
    z = (torch.randn(n, dim, generator=g) / dim ** 0.25).to(DEV)
    w = (torch.randn(5, dim, generator=g) / dim ** 0.25).to(DEV)
    keys, kptr = keys_from_pairs(cases.graph_known(n, g), n)
    known = (keys.to(DEV), kptr.to(DEV))
    pairs = [(a, b) if (a + b) % 3 else (b, a) for a in range(n) for b in range(a + 1, n)]
    ptr, tu, tv = (t.to(DEV) for t in cases.csr([pairs] * 5))
    q_rel = torch.arange(5, dtype=torch.int32, device=DEV)
    rank, logit = ops.distmult_screen_rank(z, w, q_rel, ptr, tu, tv, known)
    lists = ops.distmult_screen(z, w, torch.tensor([[r, -1] for r in range(5)]), k, known=known)
    rel = torch.repeat_interleave(torch.arange(5, device=DEV), len(pairs))
    assert bool((rank > 0).all())
    seen = _check_against_screen(rank, logit, rel, tu, tv, n, lists, known, 'n = 40')
    assert seen == rank.numel()                                           # k >= 780 pairs: every target is decided
    raw, _ = ops.distmult_screen_rank(z, w, q_rel, ptr, tu, tv, None)
    assert bool((raw >= rank).all())
    for r in range(5):
        assert sorted(raw[rel == r].tolist()) == list(range(1, len(pairs) + 1))


def test_tip_rank_pairs_small_pickle():
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    tu, tv, et = d.dd_test_idx[0], d.dd_test_idx[1], d.dd_test_et.long()
    ks = (1, 10, 50)
    from tip_amd.layers import _screen_known
    # make one held-out pair of relation 0 that is no training pair the best pair of that relation by far (as
    # tests/test_gpu_screen.py does): its rank is 1 under every filter
    tm0 = known_mask(_screen_known(d, 'train'), 0, n, DEV)
    first = int(torch.nonzero((et == 0) & (tu != tv) & ~tm0[tu, tv])[0])
    pa, pb = int(tu[first]), int(tv[first])
    z = model.embeddings.detach().clone()
    w0 = model.decoder.weight.detach()[0]
    c = 10.0 * float(z.abs().max())
    z[pa] = c * torch.sign(w0)
    z[pb] = c
    model.embeddings = z
    reports = {}
    for flt in ('train', 'all', None):
        rep = model.rank_pairs(filter=flt, ks=ks)
        reports[flt] = rep
        assert rep.rank.shape == et.shape and rep.rank.dtype == torch.int64 and str(rep.rank.device) == DEV
        assert bool((rep.rank > 0).all()) and not bool(rep.logit.isnan().any())
        res = model.screen(k=1024, exclude=flt, sigmoid=False)
        seen = _check_against_screen(rep.rank, rep.logit, et, tu, tv, n, (res.score, res.u, res.v), _screen_known(d, flt),
                                     'filter = %r' % (flt,))
        print('filter %r: %d of %d triples decided by the 1024-entry lists' % (flt, seen, et.numel()))
        assert seen >= 1 and int(rep.rank[first]) == 1, (flt, seen)
        # the report is utils.rank_report of the returned ranks
        # (to 1e-12: the report's fp64 scatter_add sums at most 4 432 terms <= 1 with device atomics, in an order that
        # changes from call to call -- two orders differ by at most 4 432 * 2^-53 = 5e-13; the counts are exact)
        want = utils.rank_report(rep.rank, et, R, ks)
        assert abs(rep.mrr - want['mrr']) <= 1e-12 and abs(rep.macro_mrr - want['macro_mrr']) <= 1e-12
        assert tuple(rep.hits) == ks and all(abs(rep.hits[k] - want['hits'][k]) <= 1e-12 for k in ks)
        assert rep.unranked == want['unranked'] == 0
        assert torch.equal(rep.per_relation['count'], want['per_relation']['count'])
        assert int(rep.per_relation['count'].sum()) == et.numel()
        for name in ('mrr', 'hits'):
            got_t, want_t = rep.per_relation[name], want['per_relation'][name]
            assert torch.equal(got_t.isnan(), want_t.isnan()), name
            assert bool(((got_t - want_t).nan_to_num().abs() <= 1e-12).all()), name
        # (u, v) and (v, u): equal ranks
        swapped = model.rank_pairs(triples=(d.dd_test_idx.flip(0), d.dd_test_et), filter=flt, ks=ks)
        assert torch.equal(swapped.rank, rep.rank) and torch.equal(swapped.logit.view(torch.int32), rep.logit.view(torch.int32))
    explicit = model.rank_pairs(triples=(d.dd_test_idx.cpu(), d.dd_test_et.cpu()), filter='all', ks=ks)
    assert torch.equal(explicit.rank, reports['all'].rank) and abs(explicit.mrr - reports['all'].mrr) <= 1e-12
    assert bool((reports['all'].rank <= reports['train'].rank).all())
    assert bool((reports['train'].rank <= reports[None].rank).all())
