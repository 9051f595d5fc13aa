"""-m gpu: `tipk_distmult_screen` (include/tipk.h section 4c) and `TIP.screen` against the fp64 acceptance rule of
tests/screen_spec.py -- small random graphs at every supported width, both filter routes, repeat runs, the exclude modes
of `TIP.screen`, the full BioSNAP relation screen and a config-5-sized graph.  Each case launches the screen once (the
route and repeat case: three times) and checks on the device."""
import os

import pytest
import torch

from screen_spec import check_screen, keys_from_pairs, known_mask
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _graph(n, dim, seed):
    """z, w (5 relations) and known pairs: r0 ~15 % of the pairs, listed in one direction only (larger id first); r1 ~4 %,
    both directions; r2 none; r3 every pair; r4 every partner of drug 7 and two more pairs."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, dim, generator=g) / dim ** 0.25
    w = torch.randn(5, dim, generator=g) / dim ** 0.25
    iu = torch.triu_indices(n, n, 1)
    m0 = torch.rand(iu.shape[1], generator=g) < 0.15
    r0 = list(zip(iu[1][m0].tolist(), iu[0][m0].tolist()))
    m1 = torch.rand(iu.shape[1], generator=g) < 0.04
    r1 = list(zip(iu[0][m1].tolist(), iu[1][m1].tolist()))
    r1 += [(b, a) for a, b in r1]
    r3 = list(zip(iu[0].tolist(), iu[1].tolist()))
    r4 = [(7, v) for v in range(n) if v != 7] + [(1, 2), (3, 1)]
    keys, ptr = keys_from_pairs([r0, r1, [], r3, r4], n)
    return z.to(DEV), w.to(DEV), (keys.to(DEV), ptr.to(DEV))


def _queries(n):
    """every relation query, then drug queries: a plain one, the last node, a drug whose every partner is known (twice),
    a relation without known pairs, a relation whose every pair is known."""
    return [[r, -1] for r in range(5)] + [[0, 0], [1, n - 1], [4, 7], [4, 7], [2, 3], [3, 5]]


@pytest.mark.parametrize('n,dim,k', [(70, 4, 1), (133, 8, 1024), (97, 16, 37), (201, 32, 1024), (130, 64, 5),
                                     (77, 128, 1024), (301, 16, 1), (130, 36, 37)])
def test_screen_small_graphs(n, dim, k):
    z, w, known = _graph(n, dim, seed=1000 * n + dim)
    q = _queries(n)
    got = ops.distmult_screen(z, w, torch.tensor(q), k, known=known)
    check_screen(z, w, q, k, got, known)
    s, u, _ = got
    assert bool((u[3] == -1).all()) and bool(s[3].isneginf().all())                  # relation 3: every pair known
    assert bool((u[7] == -1).all()) and bool((u[8] == -1).all())                      # drug 7 under relation 4


def test_screen_single_query_split_merge():
    """n_q = 1: the relation query is split over 64 workgroups and merged in two levels; then one drug query alone."""
    n, dim, k = 700, 16, 300
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, dim, generator=g).to(DEV)
    w = torch.randn(1, dim, generator=g).to(DEV)
    got = ops.distmult_screen(z, w, torch.tensor([[0, -1]]), k)
    check_screen(z, w, [[0, -1]], k, got)
    got = ops.distmult_screen(z, w, torch.tensor([[0, 123]]), k)
    check_screen(z, w, [[0, 123]], k, got)


def test_screen_routes_identical_and_repeatable():
    n, dim, k = 645, 16, 100
    z, w, known = _graph(n, dim, seed=645)
    q = _queries(n) + [[r % 5, (37 * r) % n] for r in range(40)]
    assert _lib.lib().tipk_distmult_screen_bitmap_route(n) == 1
    a = ops.distmult_screen(z, w, torch.tensor(q), k, known=known)
    b = ops.distmult_screen(z, w, torch.tensor(q), k, known=known)
    _lib.set_option('screen_search', 1)
    try:
        assert _lib.lib().tipk_distmult_screen_bitmap_route(n) == 0
        c = ops.distmult_screen(z, w, torch.tensor(q), k, known=known)
    finally:
        _lib.set_option('screen_search', 0)
    for x, y, name in zip(a, b, ('score', 'u', 'v')):
        assert torch.equal(x, y), 'run to run: ' + name
    for x, y, name in zip(a, c, ('score', 'u', 'v')):
        assert torch.equal(x, y), 'bitmap vs search route: ' + name
    check_screen(z, w, q, k, a, known)


def test_screen_empty_known_lists_drop_nothing():
    """A known list without any key is `known=None`, bit for bit (an empty tensor has no address to hand over); a list that
    is empty for relation 0 only leaves the relation-0 rows as they are.  The smallest shape with both query kinds."""
    n, dim, n_rel, k = 5, 4, 2, 3
    g = torch.Generator().manual_seed(5)
    z, w = torch.randn(n, dim, generator=g).to(DEV), torch.randn(n_rel, dim, generator=g).to(DEV)
    q = torch.tensor([[0, -1], [1, 2]])
    plain = ops.distmult_screen(z, w, q, k, known=None)
    empty = (torch.empty(0, dtype=torch.int64, device=DEV), torch.zeros(n_rel + 1, dtype=torch.int64, device=DEV))
    for x, y, name in zip(ops.distmult_screen(z, w, q, k, known=empty), plain, ('score', 'u', 'v')):
        assert torch.equal(x, y), 'empty list vs None: ' + name
    partner = int(plain[2][1, 0])                                         # drug 2's best partner under relation 1
    half = (torch.tensor([2 * n + partner], device=DEV), torch.tensor([0, 0, 1], device=DEV))
    got = ops.distmult_screen(z, w, q, k, known=half)
    for x, y, name in zip(got, plain, ('score', 'u', 'v')):
        assert torch.equal(x[0], y[0]), 'relation 0 has no keys: ' + name
    assert partner not in got[2][1].tolist()                              # ... and relation 1's one key was read


# ------------------------------------------------------------------ TIP.screen
def _known_of(idx, rng, n, extra=None):
    """(keys, ptr) on the device from edge lists grouped by relation (optionally merged with a second one)."""
    lists = []
    for r, (a, b) in enumerate(torch.as_tensor(rng).long().tolist()):
        pairs = list(zip(idx[0, a:b].tolist(), idx[1, a:b].tolist()))
        if extra is not None:
            ea, eb = torch.as_tensor(extra[1]).long().tolist()[r]
            pairs += list(zip(extra[0][0, ea:eb].tolist(), extra[0][1, ea:eb].tolist()))
        lists.append(pairs)
    keys, ptr = keys_from_pairs(lists, n)
    return keys.to(DEV), ptr.to(DEV)


def test_tip_screen_exclude_modes():
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    tr_idx, te_idx = d.dd_train_idx.cpu(), d.dd_test_idx.cpu()
    train = _known_of(tr_idx, d.dd_train_range, n)
    both = _known_of(tr_idx, d.dd_train_range, n, extra=(te_idx, d.dd_test_range))
    # make one held-out pair of relation 0 the best pair of that relation by far
    a0, b0 = torch.as_tensor(d.dd_test_range).long().tolist()[0]
    tm0 = known_mask(train[0], train[1], 0, n, 'cpu')
    pa, pb = next((u, v) for u, v in zip(te_idx[0, a0:b0].tolist(), te_idx[1, a0:b0].tolist()) if u != v and not tm0[u, v])
    pa, pb = min(pa, pb), max(pa, pb)
    z = model.embeddings.detach().clone()
    w = model.decoder.weight.detach()
    c = 10.0 * float(z.abs().max())                      # logit(pa, pb) = c^2 sum|w0| >= 10 x logit(pa or pb, any other)
    z[pa] = c * torch.sign(w[0])
    z[pb] = c
    model.embeddings = z
    q = [[r, -1] for r in range(R)]
    k = 64

    res = model.screen(k=k, exclude='train', sigmoid=False)
    check_screen(z, w, q, k, (res.score, res.u, res.v), train)
    assert (int(res.u[0, 0]), int(res.v[0, 0])) == (pa, pb), 'a held-out pair that ranks first is returned first'
    assert torch.equal(res.relation, torch.arange(R, device=DEV)[:, None].expand(R, k))
    sig = model.screen(k=k, exclude='train')
    assert torch.equal(sig.score, torch.sigmoid(res.score)) and torch.equal(sig.u, res.u) and torch.equal(sig.v, res.v)

    # the returned logits are the decoder kernel's logits of the same triples
    ok = res.u >= 0
    idx = torch.stack([res.u[ok], res.v[ok]]).long()
    ref = model.decoder(model.embeddings, idx, res.relation[ok], sigmoid=False)
    torch.testing.assert_close(res.score[ok], ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()))

    res_all = model.screen(k=k, exclude='all', sigmoid=False)
    check_screen(z, w, q, k, (res_all.score, res_all.u, res_all.v), both)
    assert not bool(((res_all.u[0] == pa) & (res_all.v[0] == pb)).any())

    res_none = model.screen(k=k, exclude=None, sigmoid=False)
    check_screen(z, w, q, k, (res_none.score, res_none.u, res_none.v), None)
    iu = torch.triu_indices(n, n, 1, device=DEV)
    for r in range(R):                                   # the unfiltered dense top-k of the decoder kernel's logits
        dense = model.decoder(model.embeddings, iu, torch.full((iu.shape[1],), r, device=DEV), sigmoid=False)
        top = torch.sort(dense, descending=True, stable=True)
        torch.testing.assert_close(res_none.score[r], top.values[:k], rtol=1e-6, atol=1e-6 * float(top.values.abs().max()))
        same = (res_none.u[r].long() == iu[0, top.indices[:k]]) & (res_none.v[r].long() == iu[1, top.indices[:k]])
        gap = (top.values[:k] - top.values[1:k + 1]).abs() > 1e-5 * float(top.values.abs().max())
        assert bool((same | ~gap).all()), r                  # pairs differ only where two logits are within rounding

    dq = model.screen(k=5, relations=[0, 2], drugs=[pa, 3], exclude='train', sigmoid=False)
    qd = [[0, pa], [2, pa], [0, 3], [2, 3]]
    check_screen(z, w, qd, 5, (dq.score, dq.u, dq.v), train)
    assert dq.relation[:, 0].tolist() == [0, 2, 0, 2]
    assert (int(dq.u[0, 0]), int(dq.v[0, 0])) == (pa, pb)


def test_biosnap_relation_screen():
    """The bundled BioSNAP graph (645 drugs, 1 097 relations), three training steps, then the full relation screen with
    k = 100 excluding the training positives: 32 relations against fp64 in full, the top pair of every relation too."""
    from tip_amd.layers import TIP, Setting
    from tip_amd.neg_sampling import _cached_keys
    torch.manual_seed(2)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for _ in range(3):
        opt.zero_grad()
        model().backward()
        opt.step()
    d = model.data
    n, R, k = d.n_drug, d.n_dd_et, 100
    res = model.screen(k=k, exclude='train', sigmoid=False)
    torch.cuda.synchronize()
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    known = _cached_keys(d.dd_train_idx, n, d.dd_train_range)[:2]
    g = torch.Generator().manual_seed(11)
    rels = sorted(torch.randperm(R, generator=g)[:32].tolist())
    check_screen(z, w, [[r, -1] for r in rels], k, (res.score[rels], res.u[rels], res.v[rels]), known)

    # top-1 of every relation, 64 relations at a time
    z64, w64 = z.double(), w.double()
    ptr = known[1].tolist()
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), 1)
    for r0 in range(0, R, 64):
        rs = list(range(r0, min(R, r0 + 64)))
        A = z64[None] * w64[rs][:, None, :]
        L = A @ z64.t()
        T = 1e-5 * (1.0 + A.abs() @ z64.abs().t())
        km = torch.zeros((len(rs), n, n), dtype=torch.bool, device=DEV)
        for j, r in enumerate(rs):
            ks = known[0][ptr[r]:ptr[r + 1]]
            km[j, ks // n, ks % n] = True
            km[j, ks % n, ks // n] = True
        cand = upper[None] & ~km
        b = torch.arange(len(rs), device=DEV)
        u1, v1, s1 = res.u[rs, 0].long(), res.v[rs, 0].long(), res.score[rs, 0].double()
        assert bool((u1 >= 0).all()) and bool(cand[b, u1, v1].all())
        assert bool(((s1 - L[b, u1, v1]).abs() <= T[b, u1, v1]).all())
        worst = (L - T).masked_fill(~cand, float('-inf')).amax((1, 2))
        assert bool((worst <= L[b, u1, v1] + T[b, u1, v1]).all()), r0


def test_large_graph_search_route():
    """N = 10 000, dim = 128, 4 relations with ~1e5 known pairs each (n^2 bits do not fit in LDS: search route)."""
    n, dim, k = 10000, 128, 100
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(n, dim, generator=g) / dim ** 0.25).to(DEV)
    w = (torch.randn(4, dim, generator=g) / dim ** 0.25).to(DEV)
    keys, ptr = [], [0]
    for r in range(4):
        a = torch.randint(0, n, (100000,), generator=g)
        b = torch.randint(0, n, (100000,), generator=g)
        ks = torch.unique(a[a != b] * n + b[a != b])
        keys.append(ks)
        ptr.append(ptr[-1] + ks.numel())
    known = (torch.cat(keys).to(DEV), torch.tensor(ptr, dtype=torch.int64, device=DEV))
    assert _lib.lib().tipk_distmult_screen_bitmap_route(n) == 0
    q = [[0, -1], [1, -1], [2, -1], [3, -1], [1, 17], [3, n - 1]]
    got = ops.distmult_screen(z, w, torch.tensor(q), k, known=known)
    check_screen(z, w, q, k, got, known)
