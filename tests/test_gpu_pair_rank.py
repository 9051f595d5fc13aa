"""-m gpu: `tipk_distmult_pair_rank` / `tipk_pair_table_pair_rank` (include/tipk.h section 4f) and `TIP.rank_side_effects`
against the fp64 acceptance rule of tests/pair_rank_spec.py -- small shapes around the 64-relation lane groups for both
decoders, exact inputs with many ties, bitwise agreement with the pair top-k, the target-chunk edge, the known filter's
corners across the 2 048-relation bitmap window, what is not ranked, both DistMult routes and repeat runs, the three filters
of `TIP.rank_side_effects` for both decoder kinds, and the held-out triples of the bundled graph.  The inputs come from
tests/pair_rank_cases.py, whose seeds tests/test_host_pair_rank.py holds to the rule's degeneracy cap."""
import os

import numpy as np
import pytest
import torch

import pair_rank_cases as cases
from pair_rank_spec import check_pair_rank, spec_pair_rank
from pair_topk_spec import known_from_dict
from tip_amd import _lib, ops, utils

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = cases.N
K = 128


def _dev(case):
    model, pairs, ptr, rel, known = case
    return ((model[0], model[1].to(DEV), model[2].to(DEV)), pairs.to(DEV), ptr.to(DEV), rel.to(DEV),
            None if known is None else tuple(t.to(DEV) for t in known))


def _run(model, pairs, ptr, rel, known=None):
    fn = ops.distmult_pair_rank if model[0] == 'distmult' else ops.pair_table_pair_rank
    return fn(model[1], model[2], pairs, ptr, rel, known)


def _topk(model, pairs, k, known=None):
    fn = ops.distmult_pair_topk if model[0] == 'distmult' else ops.pair_table_pair_topk
    return fn(model[1], model[2], pairs, k, known)


def _owner(ptr):
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=ptr.device), ptr[1:] - ptr[:-1])


def _small(kind, n_rel, dim):
    model, pairs, ptr, rel, known = _dev(cases.small_case(kind, n_rel, dim))
    for kn in (None, known):
        r, s = _run(model, pairs, ptr, rel, kn)
        assert r.dtype == torch.int32 and s.dtype == torch.float32 and r.shape == rel.shape == s.shape
        check_pair_rank(model, pairs, ptr, rel, (r, s), kn)
        a, b = int(ptr[0]), int(ptr[1])
        lo, hi = int(ptr[3]), int(ptr[4])
        assert torch.equal(r[a:b], r[lo:hi]) and torch.equal(s[a:b], s[lo:hi])            # the repeated pair
        if kind == 'distmult':                                                            # the reversed pair: same bits
            assert torch.equal(r[a:b], r[int(ptr[1]):int(ptr[2])]) and torch.equal(s[a:b], s[int(ptr[1]):int(ptr[2])])


@pytest.mark.parametrize('dim', cases.SMALL_DIM)
@pytest.mark.parametrize('n_rel', cases.SMALL_R)
def test_distmult_small_shapes(n_rel, dim):
    _small('distmult', n_rel, dim)


@pytest.mark.parametrize('n_rel', cases.SMALL_R)
def test_table_small_shapes(n_rel):
    _small('table', n_rel, 0)


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_exact_inputs_match_the_spec(kind):
    """z in {-2..2}, w in {-1, -0.5, 0, 0.5, 1} (the tables likewise): every product and sum is exact in fp32, logits tie in
    droves, and the rank is the spec's rank exactly, tie rule included."""
    g = torch.Generator().manual_seed(77)
    n_rel, dim = 130, 16
    if kind == 'distmult':
        model = ('distmult', torch.randint(-2, 3, (N, dim), generator=g).float(),
                 (torch.randint(-2, 3, (n_rel, dim), generator=g) / 2).float())
    else:
        model = ('table', torch.randint(-2, 3, (N, n_rel), generator=g).float(),
                 (torch.randint(-2, 3, (N, n_rel), generator=g) / 2).float())
    _, pairs, ptr, rel, known = cases.small_case(kind, n_rel, dim)
    want_r, want_s = spec_pair_rank(model, pairs, ptr, rel, known)
    r, s = _run(*_dev((model, pairs, ptr, rel, known)))
    assert torch.equal(r.cpu().long(), want_r) and torch.equal(s.cpu().double(), want_s)
    ties = sum(int((want_s == x).sum()) > 1 for x in want_s.tolist())
    assert ties >= 10, ties


@pytest.mark.parametrize('kind', ['distmult', 'table'])
@pytest.mark.parametrize('n_rel', [130, 700])
def test_agrees_with_pair_topk_bitwise(kind, n_rel):
    """Same inputs, same known lists with each target taken off its pair's block on the host (one top-k row per target): a
    target of rank <= 128 sits at position rank - 1 of the row with the same logit bits, one of rank > 128 is absent."""
    model, pairs, ptr, rel, known = cases.small_case(kind, 130, 16) if n_rel == 130 else cases.routes_case(700, 16, 60)
    if kind == 'table' and n_rel == 700:
        model = cases.model_of('table', N, n_rel, 0, torch.Generator().manual_seed(3))
    keys, kptr, krel = (t.tolist() for t in known)
    blocks = {k: krel[kptr[i]:kptr[i + 1]] for i, k in enumerate(keys)}
    owner = _owner(ptr).tolist()
    one_u, one_v, d = [], [], {}
    # a pair of its own per target: node ids are shifted by a copy index so every (pair, target) has a key of its own
    copies = len(owner)
    assert copies * N <= 46340
    za = model[1].repeat(copies, 1) if kind == 'distmult' else model[1].repeat(copies, 1)
    zb = model[2] if kind == 'distmult' else model[2].repeat(copies, 1)
    big = (kind, za, zb)
    n_big = copies * N
    for i, (p, t) in enumerate(zip(owner, rel.tolist())):
        u, v = int(pairs[0, p]) + i * N, int(pairs[1, p]) + i * N
        one_u.append(u)
        one_v.append(v)
        lo, hi = min(int(pairs[0, p]), int(pairs[1, p])), max(int(pairs[0, p]), int(pairs[1, p]))
        d[(u, v)] = [x for x in blocks.get(lo * N + hi, []) if x != t]
    rows = torch.tensor([one_u, one_v])
    big_known = tuple(t.to(DEV) for t in known_from_dict(d, n_big))
    big_d = _dev((big, rows, torch.arange(copies + 1), rel, None))
    r, s = _run(big_d[0], big_d[1], big_d[2], big_d[3], big_known)
    # the shifted copies rank as the original pairs do under the original lists
    r0, s0 = _run(*_dev((model, pairs, ptr, rel, known)))
    assert torch.equal(r, r0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    ts, tr = _topk(big_d[0], big_d[1], K, big_known)
    r, t = r.long(), big_d[3].long()
    inside = r <= K
    assert bool(inside.any()) and (n_rel == 130 or bool((~inside).any()))
    at = (r - 1).clamp(max=K - 1)[:, None]
    assert bool((tr.long().gather(1, at)[:, 0] == t)[inside].all())
    assert torch.equal(ts.gather(1, at)[:, 0][inside].view(torch.int32), s[inside].view(torch.int32))
    assert not bool((tr.long() == t[:, None]).any(1)[~inside].any())


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_targets_per_pair(kind):
    model, pairs, ptr, rel, known = _dev(cases.counts_case(kind))
    assert (ptr[1:] - ptr[:-1]).tolist() == list(cases.COUNTS) + [130]
    for kn in (None, known):
        r, s = _run(model, pairs, ptr, rel, kn)
        check_pair_rank(model, pairs, ptr, rel, (r, s), kn)
        a = int(ptr[3])
        assert int(rel[a + 5]) == int(rel[a + 40]) and int(r[a + 5]) == int(r[a + 40])   # a repeated target: equal ranks
        last = r[int(ptr[-2]):].long()                                    # every relation, no block: a permutation
        assert sorted(last.tolist()) == list(range(1, 131))
    # the same targets one per pair give the same ranks: chunks of 64 do not interact
    owner = _owner(ptr)
    one = _run(model, pairs[:, owner], torch.arange(rel.numel() + 1, device=DEV), rel, known)
    assert torch.equal(one[0], r) and torch.equal(one[1].view(torch.int32), s.view(torch.int32))


@pytest.mark.parametrize('kind', ['distmult', 'table'])
@pytest.mark.parametrize('n_rel', [70, 4500])
def test_known_filter_corners(kind, n_rel):
    case, some = cases.corner_case(kind, n_rel)
    model, pairs, ptr, rel, known = _dev(case)
    assert known[0].tolist() == [0, 4 * N + 9, 20 * N + 30, (N - 1) * N + N - 1]
    r, s = _run(model, pairs, ptr, rel, known)
    check_pair_rank(model, pairs, ptr, rel, (r, s), known)
    raw = _run(model, pairs, ptr, rel)
    check_pair_rank(model, pairs, ptr, rel, raw)
    m = int(ptr[1])
    rows, raw_rows = r.view(-1, m).long(), raw[0].view(-1, m).long()
    assert bool((rows[3] == 1).all()) and bool((rows[4] == 1).all())      # every relation listed, either direction
    for row in (5, 6, 8, 9):                                              # no block: the raw rank
        assert torch.equal(rows[row], raw_rows[row])
    for row in (0, 1, 2, 7):                                              # `some` listed: it no longer competes
        assert bool((rows[row] <= raw_rows[row]).all()) and bool((rows[row] < raw_rows[row]).any())
        assert int(rows[row].max()) <= n_rel - len(some) + 1
    if kind == 'distmult':
        assert torch.equal(rows[1], rows[2]) and torch.equal(rows[8], rows[9])   # the pair given in reverse
    # an empty list (no key at all) filters nothing
    none = tuple(t.to(DEV) for t in known_from_dict({}, N))
    e = _run(model, pairs, ptr, rel, none)
    assert torch.equal(e[0], raw[0]) and torch.equal(e[1].view(torch.int32), raw[1].view(torch.int32))


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_not_ranked(kind):
    """Through the ops (the Python face of `TIP` refuses such ids): rank 0 and logit NaN, the neighbours unaffected."""
    g = torch.Generator().manual_seed(9)
    n_rel, dim = 70, 16
    model = cases.model_of(kind, N, n_rel, dim, g)
    model[1][50, 3] = float('nan')                                        # z[50] (s1[50]): every logit of a pair with 50 (of
    if kind == 'table':                                                   # relation 3 for the tables) is NaN
        model[1][50, :] = float('nan')
    model = (kind, model[1].to(DEV), model[2].to(DEV))
    pu = torch.tensor([1, N, 2, -1, 3, 2 ** 31 - 1, 4, 50, 5], dtype=torch.int32, device=DEV)
    pv = torch.tensor([2, 0, 500, 0, 3, 5, -7, 6, 6], dtype=torch.int32, device=DEV)
    tg = [3, 69, 0]
    lists = [tg, tg, tg, tg, [-1, 3, n_rel, 69, 2 ** 31 - 1, 0], tg, tg, tg, tg]
    ptr, rel = (t.to(DEV) for t in cases.csr(lists))
    r, s = _run(model, torch.stack([pu, pv]), ptr, rel)
    rows = {i: slice(int(ptr[i]), int(ptr[i + 1])) for i in range(9)}
    for i in (1, 2, 3, 5, 6, 7):
        assert bool((r[rows[i]] == 0).all()) and bool(torch.isnan(s[rows[i]]).all()), i
    good = torch.tensor([[1, 3, 5], [2, 3, 6]], device=DEV)
    gp, gr = (t.to(DEV) for t in cases.csr([tg, tg, tg]))
    want = _run(model, good, gp, gr)
    assert bool((want[0] > 0).all())
    for j, i in enumerate((0, 4, 8)):
        got_r, got_s = r[rows[i]], s[rows[i]]
        if i == 4:
            assert got_r[[0, 2, 4]].tolist() == [0, 0, 0] and bool(torch.isnan(got_s[[0, 2, 4]]).all())
            got_r, got_s = got_r[[1, 3, 5]], got_s[[1, 3, 5]]
        assert torch.equal(got_r, want[0][3 * j:3 * j + 3]) and torch.equal(got_s, want[1][3 * j:3 * j + 3]), i
    check_pair_rank(model, torch.stack([pu, pv]), ptr, rel, (r, s))


def test_routes_identical_and_repeatable():
    L = _lib.lib()
    assert _lib.get_option('pair_rank_stream') == 0
    for n_rel, dim, n_pairs in cases.ROUTES:
        model, pairs, ptr, rel, known = _dev(cases.routes_case(n_rel, dim, n_pairs))
        fits = n_rel < 4500
        assert L.tipk_distmult_pair_rank_lds_route(dim, n_rel) == int(fits)
        a = _run(model, pairs, ptr, rel, known)
        b = _run(model, pairs, ptr, rel, known)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), 'run to run'
        check_pair_rank(model, pairs, ptr, rel, a, known)
        if not fits:
            continue
        _lib.set_option('pair_rank_stream', 1)
        try:
            assert L.tipk_distmult_pair_rank_lds_route(dim, n_rel) == 0
            c = _run(model, pairs, ptr, rel, known)
            d = _run(model, pairs, ptr, rel, known)
        finally:
            _lib.set_option('pair_rank_stream', 0)
        for x, y, what in ((c, d, 'global route, run to run'), (a, c, 'LDS vs global route')):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)), (what, dim)
    # no logits asked for: the C entry takes NULL
    out = torch.zeros(rel.numel(), dtype=torch.int32, device=DEV)
    p = _lib.ptr
    pu, pv = pairs[0].int().contiguous(), pairs[1].int().contiguous()
    st = L.tipk_distmult_pair_rank(p(model[1]), N, dim, p(model[2]), n_rel, p(pu), p(pv), pairs.shape[1], p(ptr), p(rel),
                                   rel.numel(), p(known[0]),
                                   p(known[1]), p(known[2]), known[0].numel(), p(out), None,
                                   _lib.stream_ptr(torch.device(DEV)))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(out, a[0])


# ------------------------------------------------------------------ TIP.rank_side_effects
def _model_of(model):
    z = model.embeddings.detach()
    if model.decoder_kind == 'distmult':
        return ('distmult', z, model.decoder.weight.detach())
    dec = model.decoder
    with torch.no_grad():                                                 # the tables as NNDecoder.forward forms them
        s1 = ops.matmul(torch.relu(ops.matmul(z, dec.w1_l1)), dec.w1_l2.t())
        s2 = ops.matmul(torch.relu(ops.matmul(z, dec.w2_l1)), dec.w2_l2.t())
    return ('table', s1, s2)


def _report_numpy(rank, rel, n_rel, ks):
    rank, rel = rank.cpu().numpy().astype(np.int64), rel.cpu().numpy().astype(np.int64)
    ok = rank > 0
    rr = 1.0 / rank[ok].astype(np.float64)
    out = {'mrr': rr.mean(), 'hits': {k: (rank[ok] <= k).mean() for k in ks}, 'unranked': int((~ok).sum())}
    per = np.full(n_rel, np.nan)
    for r in np.unique(rel[ok]):
        per[r] = rr[rel[ok] == r].mean()
    out['per'] = per
    out['macro'] = np.nanmean(per)
    return out


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_rank_side_effects(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    m = _model_of(model)
    pairs, ptr, rel, order = ops.targets_by_pair(d.dd_test_idx, d.dd_test_et, n)
    train = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n)
    both = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n, extra=(d.dd_test_idx, d.dd_test_range))
    reports = {}
    for flt, known in (('all', both), ('train', train), (None, None)):
        rep = model.rank_side_effects(filter=flt, ks=(1, 3, 10))
        reports[flt] = rep
        assert rep.rank.dtype == torch.int64 and rep.rank.shape == d.dd_test_et.shape == rep.logit.shape
        check_pair_rank(m, pairs, ptr, rel, (rep.rank[order], rep.logit[order]), known)
        want = _report_numpy(rep.rank, d.dd_test_et, R, (1, 3, 10))
        assert abs(rep.mrr - want['mrr']) <= 1e-12 and abs(rep.macro_mrr - want['macro']) <= 1e-12
        assert all(abs(rep.hits[k] - want['hits'][k]) <= 1e-12 for k in (1, 3, 10)) and rep.unranked == want['unranked'] == 0
        again = utils.rank_report(rep.rank.cpu(), d.dd_test_et.cpu(), R, (1, 3, 10))
        assert abs(again['mrr'] - rep.mrr) <= 1e-12 and all(abs(again['hits'][k] - rep.hits[k]) <= 1e-12 for k in (1, 3, 10))
        np.testing.assert_allclose(rep.per_relation['mrr'].cpu().numpy(), want['per'], rtol=0, atol=1e-12, equal_nan=True)
    assert bool((reports['all'].rank <= reports['train'].rank).all()) and bool((reports['train'].rank <= reports[None].rank).all())
    assert reports['all'].mrr >= reports['train'].mrr >= reports[None].mrr
    given = model.rank_side_effects((d.dd_test_idx, d.dd_test_et), filter='train')
    assert torch.equal(given.rank, reports['train'].rank)

    # side_effects(exclude='train') holds a held-out relation of rank <= k at position rank - 1, unless it is a training
    # relation of the pair as well (then side_effects drops it, while its rank stands)
    k = min(R, 128)
    rep = reports['train']
    tpairs = d.dd_test_idx
    se = model.side_effects(tpairs, k=k, exclude='train', sigmoid=False)
    key = (torch.minimum(tpairs[0], tpairs[1]) * n + torch.maximum(tpairs[0], tpairs[1])) * R + d.dd_test_et
    owner = torch.repeat_interleave(torch.arange(train[0].numel(), device=DEV), train[1][1:] - train[1][:-1])
    in_train = torch.isin(key, train[0][owner] * R + train[2].long())
    use = (rep.rank <= k) & ~in_train
    assert int(use.sum()) >= 10
    at = (rep.rank - 1).clamp(max=k - 1)[:, None]
    assert bool((se.relation.gather(1, at)[:, 0] == d.dd_test_et)[use].all())
    assert torch.equal(se.score.gather(1, at)[:, 0][use].view(torch.int32), rep.logit[use].view(torch.int32))

    # relations=[...]: ranks among the subset; a triple outside it is not ranked
    sub = [4, 1, 5, 0]
    rs = model.rank_side_effects(filter='train', relations=sub)
    inside = torch.isin(d.dd_test_et, torch.tensor(sub, device=DEV))
    assert bool((rs.rank[~inside] == 0).all()) and bool((rs.rank[inside] >= 1).all()) and int(rs.rank.max()) <= len(sub)
    assert rs.unranked == int((~inside).sum())
    with pytest.raises(ValueError, match='out of range'):
        model.rank_side_effects((torch.tensor([[0], [n]]), torch.tensor([0])))


def test_biosnap_size_held_out_triples():
    """The held-out triples of the bundled graph (924 708 on 117 836 ordered pairs, 1 097 relations), seeded random
    embeddings of dim 16, filter 'all' (train and test lists: about 73 known relations per known pair): one launch, every
    rank against fp64, chunked on the device."""
    from tip_amd.data import build_data_dict
    d = build_data_dict()
    n, R = d['n_drug'], d['n_dd_et']
    test_idx, test_et = d['dd_test_idx'].to(DEV), d['dd_test_et'].to(DEV)
    pairs, ptr, rel, order = ops.targets_by_pair(test_idx, test_et, n)
    known = ops.known_relations_by_pair(d['dd_train_idx'].to(DEV), d['dd_train_range'], n,
                                        extra=(test_idx, d['dd_test_range']))
    model = cases.biosnap_weights(n, R)
    model = ('distmult', model[1].to(DEV), model[2].to(DEV))
    assert _lib.lib().tipk_distmult_pair_rank_lds_route(16, R) == 1
    r, s = ops.distmult_pair_rank(model[1], model[2], pairs, ptr, rel, known)
    share = check_pair_rank(model, pairs, ptr, rel, (r, s), known, chunk=16384)
    print('biosnap: %d triples, %d pairs, share of targets with two admissible ranks %.2e' % (rel.numel(), pairs.shape[1], share))
    assert bool((r > 0).all())
    rep = utils.rank_report(r, rel, R)
    assert rep['unranked'] == 0 and 0 < rep['mrr'] < 1
