"""-m gpu: `tipk_distmult_partner_rank` / `tipk_pair_table_partner_rank` (include/tipk.h section 4g) and `TIP.rank_partners`
against the fp64 acceptance rule of tests/partner_rank_spec.py -- small shapes around the 64-drug lane groups for both
decoders, exact inputs with many ties, bitwise agreement with the screen's drug queries, the target-chunk edge, the known
filter's corners across the 2 048-drug bitmap window, what is not ranked, both DistMult routes, repeat runs and a captured
run, the three filters of `TIP.rank_partners` for both decoder kinds, and held-out triples of the bundled graph.  The inputs
come from tests/partner_rank_cases.py, whose seeds tests/test_host_partner_rank.py holds to the rule's degeneracy cap."""
import os

import numpy as np
import pytest
import torch

import partner_rank_cases as cases
from partner_rank_spec import check_partner_rank, spec_partner_rank
from tip_amd import _lib, ops, utils

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _table_to_dev(t):
    """A matrix on the device with the row stride it has on the host (`.to` would pack a padded view); the pad is NaN."""
    if t.stride(0) == t.shape[1]:
        return t.to(DEV)
    wide = torch.full((t.shape[0], t.stride(0)), float('nan'), dtype=t.dtype, device=DEV)
    wide[:, :t.shape[1]] = t.to(DEV)
    return wide[:, :t.shape[1]]


def _dev(case):
    model, q_rel, q_drug, ptr, node, known = case
    return ((model[0], _table_to_dev(model[1]), _table_to_dev(model[2])), q_rel.to(DEV), q_drug.to(DEV), ptr.to(DEV),
            node.to(DEV), None if known is None else tuple(t.to(DEV) for t in known))


def _run(model, q_rel, q_drug, ptr, node, known=None):
    fn = ops.distmult_partner_rank if model[0] == 'distmult' else ops.pair_table_partner_rank
    return fn(model[1], model[2], q_rel, q_drug, ptr, node, known)


def _same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))


def _owner(ptr):
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=ptr.device), ptr[1:] - ptr[:-1])


def _small(kind, n, dim):
    model, q_rel, q_drug, ptr, node, known = _dev(cases.small_case(kind, n, dim))
    assert q_rel.numel() == 40 and (q_rel[0], q_drug[0]) == (q_rel[2], q_drug[2])
    if n > 2:                                                             # the drug of query 3 is in no key
        assert not bool(((known[0] // n == n - 1) | (known[0] % n == n - 1)).any())
    for kn in (None, known):
        r, s = _run(model, q_rel, q_drug, ptr, node, kn)
        assert r.dtype == torch.int32 and s.dtype == torch.float32 and r.shape == node.shape == s.shape
        check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s), kn)
        a, b = int(ptr[0]), int(ptr[1])
        lo, hi = int(ptr[2]), int(ptr[3])
        assert torch.equal(r[a:b], r[lo:hi]) and torch.equal(s[a:b].view(torch.int32), s[lo:hi].view(torch.int32))   # the repeated query


@pytest.mark.parametrize('dim', cases.SMALL_DIM)
@pytest.mark.parametrize('n', cases.SMALL_N)
def test_distmult_small_shapes(n, dim):
    _small('distmult', n, dim)


@pytest.mark.parametrize('n', cases.SMALL_N)
def test_table_small_shapes(n):
    model = _dev(cases.small_case('table', n))[0]
    assert model[1].stride(0) == model[2].stride(0) == n + 5 and model[1].shape == (cases.R, n)      # ld = n_nodes + 5
    _small('table', n, 0)


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_exact_inputs_match_the_spec(kind):
    """z in {-2..2}, w in {-1, -0.5, 0, 0.5, 1} (the tables likewise): every product and sum is exact in fp32, logits tie in
    droves, and the rank is the spec's rank exactly, tie rule included."""
    g = torch.Generator().manual_seed(77)
    n, dim = 130, 16
    if kind == 'distmult':
        model = ('distmult', torch.randint(-2, 3, (n, dim), generator=g).float(),
                 (torch.randint(-2, 3, (cases.R, dim), generator=g) / 2).float())
    else:
        model = ('table', torch.randint(-2, 3, (cases.R, n), generator=g).float(),
                 (torch.randint(-2, 3, (cases.R, n), generator=g) / 2).float())
    _, q_rel, q_drug, ptr, node, known = cases.small_case(kind, n, dim)
    want_r, want_s = spec_partner_rank(model, q_rel, q_drug, ptr, node, known)
    r, s = _run(*_dev((model, q_rel, q_drug, ptr, node, known)))
    assert torch.equal(r.cpu().long(), want_r)
    ranked = want_r > 0                                                   # (a target that is its query's drug is not ranked)
    assert torch.equal(s.cpu().double()[ranked], want_s[ranked]) and bool(torch.isnan(s.cpu()[~ranked]).all())
    ties = sum(int((want_s == x).sum()) > 1 for x in want_s.tolist())
    assert ties >= 10, ties


@pytest.mark.parametrize('n,one_direction', [(130, False), (700, False), (130, True)])
def test_agrees_with_the_screen_bitwise(n, one_direction):
    """Queries whose targets are not on the known list: the screen's drug query (r, u) at k = n_nodes under the same lists
    holds (u, t) at position rank - 1, with the same logit bits."""
    case = cases.screen_case(n, one_direction)
    model, q_rel, q_drug, ptr, node, known = _dev(case)
    if one_direction:                                                     # no pair is listed both ways
        rev = (known[0] % n) * n + known[0] // n
        rel = torch.repeat_interleave(torch.arange(4, device=DEV), known[1][1:] - known[1][:-1])
        assert not bool(torch.isin(rel * n * n + rev, rel * n * n + known[0]).any())
    r, s = _run(model, q_rel, q_drug, ptr, node, known)
    check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s), known)
    assert bool((r > 0).all())
    queries = torch.stack([q_rel, q_drug], 1).cpu()
    ss, su, sv = ops.distmult_screen(model[1], model[2], queries, n, known)
    owner = _owner(ptr)
    at = (r.long() - 1)[:, None]
    assert bool((su[owner].long().gather(1, at)[:, 0] == q_drug[owner]).all())
    assert bool((sv[owner].long().gather(1, at)[:, 0] == node.long()).all())
    assert torch.equal(ss[owner].gather(1, at)[:, 0].view(torch.int32), s.view(torch.int32))
    # the raw ranks agree with the unfiltered screen as well
    r0, s0 = _run(model, q_rel, q_drug, ptr, node)
    ss, su, sv = ops.distmult_screen(model[1], model[2], queries, n)
    at = (r0.long() - 1)[:, None]
    assert bool((sv[owner].long().gather(1, at)[:, 0] == node.long()).all())
    assert torch.equal(ss[owner].gather(1, at)[:, 0].view(torch.int32), s0.view(torch.int32))
    assert bool((r <= r0).all()) and bool((r < r0).any())


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_targets_per_query(kind):
    model, q_rel, q_drug, ptr, node, known = _dev(cases.counts_case(kind))
    n = cases.COUNTS_N
    assert (ptr[1:] - ptr[:-1]).tolist() == list(cases.COUNTS) + [n - 1]
    assert int(known[1][-1]) == int(known[1][-2])                         # the last relation's block is empty
    for kn in (None, known):
        r, s = _run(model, q_rel, q_drug, ptr, node, kn)
        check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s), kn)
        a = int(ptr[3])
        assert int(node[a + 5]) == int(node[a + 40]) and int(r[a + 5]) == int(r[a + 40])   # a repeated target: equal ranks
        last = r[int(ptr[-2]):].long()                                    # every other drug, no key: a permutation
        assert sorted(last.tolist()) == list(range(1, n))
    # the same targets one per query give the same ranks: chunks of 64 do not interact
    owner = _owner(ptr)
    one = _run(model, q_rel[owner], q_drug[owner], torch.arange(node.numel() + 1, device=DEV), node, known)
    assert _same(one, (r, s))


@pytest.mark.parametrize('kind', ['distmult', 'table'])
@pytest.mark.parametrize('n', [70, 4500])
def test_known_filter_corners(kind, n):
    case, some = cases.corner_case(kind, n)
    model, q_rel, q_drug, ptr, node, known = _dev(case)
    keys, kptr = known
    assert int(keys[0]) == 1 and int(keys[-1]) == (n - 1) * n + n - 2     # the first key of relation 0, the last of relation 3
    assert int(kptr[2]) == int(kptr[3]) and int(kptr[0]) == 0             # relation 2: an empty block
    r, s = _run(model, q_rel, q_drug, ptr, node, known)
    check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s), known)
    raw = _run(model, q_rel, q_drug, ptr, node)
    check_partner_rank(model, q_rel, q_drug, ptr, node, raw)
    m = int(ptr[1])
    rows, raw_rows = r.view(-1, m).long(), raw[0].view(-1, m).long()
    assert bool((rows > 0).all())                                         # listed targets are ranked all the same
    assert bool((rows[2] == 1).all()) and bool((rows[3] == 1).all())      # every partner listed, forward or in reverse
    for row in (4, 6):                                                    # nothing listed for the query: the raw rank
        assert torch.equal(rows[row], raw_rows[row])
    for row in (0, 1, 5, 7):                                              # `some` listed: it no longer competes
        assert bool((rows[row] <= raw_rows[row]).all()) and bool((rows[row] < raw_rows[row]).any())
        assert int(rows[row].max()) <= n - 1 - len(some) + 1
    # an empty list (no key at all) filters nothing
    none = tuple(t.to(DEV) for t in cases.known_from_dict({}, n, 4))
    assert _same(_run(model, q_rel, q_drug, ptr, node, none), raw)


def _canary_call(model, q_rel, q_drug, ptr, node, known=None, logits=True):
    """The C entry on output arrays that sit inside larger buffers of canary values -> (rank, logit or None)."""
    L, p = _lib.lib(), _lib.ptr
    T, pad = node.numel(), 64
    rank_buf = torch.full((T + 2 * pad,), -77, dtype=torch.int32, device=DEV)
    logit_buf = torch.full((T + 2 * pad,), -77.0, dtype=torch.float32, device=DEV)
    out_r, out_s = rank_buf[pad:pad + T], logit_buf[pad:pad + T]
    qr, qd, node = q_rel.int().contiguous(), q_drug.int().contiguous(), node.int().contiguous()
    keys, kptr = (None, None) if known is None else known
    st = _lib.stream_ptr(torch.device(DEV))
    if model[0] == 'distmult':
        z, w = model[1].contiguous(), model[2].contiguous()
        rc = L.tipk_distmult_partner_rank(p(z), z.shape[0], z.shape[1], p(w), w.shape[0], p(qr), p(qd), qr.numel(), p(ptr), p(node),
                                          T, p(keys), p(kptr), p(out_r), p(out_s) if logits else None, st)
    else:
        s1t, s2t = model[1], model[2]
        rc = L.tipk_pair_table_partner_rank(p(s1t), p(s2t), s1t.stride(0), s1t.shape[1], s1t.shape[0], p(qr), p(qd), qr.numel(),
                                            p(ptr), p(node), T, p(keys), p(kptr), p(out_r), p(out_s) if logits else None, st)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, val in ((rank_buf, -77), (logit_buf, -77.0)):
        assert bool((buf[:pad] == val).all()) and bool((buf[pad + T:] == val).all()), 'a canary was overwritten'
    if not logits:
        assert bool((out_s == -77.0).all())
    return out_r.clone(), (out_s.clone() if logits else None)


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_not_ranked(kind):
    """Through the ops and the C entries (the Python face of `TIP` refuses such ids): each cause alone gives rank 0 and
    logit NaN, the neighbours are unaffected, and nothing is written around the output arrays."""
    g = torch.Generator().manual_seed(9)
    n, n_rel, dim = 70, 5, 16
    model = cases.model_of(kind, n, n_rel, dim, g, pad=3)
    if kind == 'distmult':
        model[1][50, 3] = float('nan')                                    # z[50]: every logit with drug 50 is NaN
    else:
        model[2][:, 50] = float('nan')                                    # s2t[:, 50]: drug 50 as a partner is NaN
    model = (kind, _table_to_dev(model[1]), _table_to_dev(model[2]))
    tg = [3, 69, 0]
    #        good   r high  r low  u high  u low  u huge      targets            NaN candidate only   good
    qr = [1, n_rel, -1, 2, 2, 2, 3, 4, 0]
    qd = [2, 2, 2, n, -1, 2 ** 31 - 1, 5, 6, 7]
    lists = [tg, tg, tg, tg, tg, tg, [-1, 3, n, 69, 2 ** 31 - 1, 0, 5, 50], tg, tg]
    q_rel, q_drug = torch.tensor(qr, device=DEV), torch.tensor(qd, device=DEV)
    ptr, node = (t.to(DEV) for t in cases.csr(lists))
    r, s = _run(model, q_rel, q_drug, ptr, node)
    rows = {i: slice(int(ptr[i]), int(ptr[i + 1])) for i in range(9)}
    for i in (1, 2, 3, 4, 5):
        assert bool((r[rows[i]] == 0).all()) and bool(torch.isnan(s[rows[i]]).all()), i
    good = _run(model, torch.tensor([1, 3, 4, 0], device=DEV), torch.tensor([2, 5, 6, 7], device=DEV),
                *(t.to(DEV) for t in cases.csr([tg] * 4)))
    assert bool((good[0] > 0).all())                                      # drug 50 is a NaN candidate of them all: it beats nothing
    for j, i in enumerate((0, 6, 7, 8)):
        got_r, got_s = r[rows[i]], s[rows[i]]
        if i == 6:                                                        # t low, t high, t huge, t == u, the NaN row as target
            assert got_r[[0, 2, 4, 6, 7]].tolist() == [0] * 5 and bool(torch.isnan(got_s[[0, 2, 4, 6, 7]]).all())
            got_r, got_s = got_r[[1, 3, 5]], got_s[[1, 3, 5]]
        assert torch.equal(got_r, good[0][3 * j:3 * j + 3]), i
        assert torch.equal(got_s.view(torch.int32), good[1][3 * j:3 * j + 3].view(torch.int32)), i
    check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s))
    if kind == 'distmult':                                                # the NaN row as the queried drug: no logit at all
        rn, sn = _run(model, torch.tensor([0], device=DEV), torch.tensor([50], device=DEV), *(t.to(DEV) for t in cases.csr([tg])))
        assert rn.tolist() == [0, 0, 0] and bool(torch.isnan(sn).all())
    # canaries around the outputs; a tgt_ptr that runs past both ends is clamped to [0, n_tgt)
    assert _same(_canary_call(model, q_rel, q_drug, ptr, node), (r, s))
    assert torch.equal(_canary_call(model, q_rel, q_drug, ptr, node, logits=False)[0], r)
    wild = ptr.clone()
    wild[0], wild[-1] = -5, int(ptr[-1]) + 1000
    assert _same(_canary_call(model, q_rel, q_drug, wild, node), (r, s))
    # the ops refuse what is not a list of queries
    with pytest.raises(_lib.TipkError, match='expected'):
        _run(model, q_rel, q_drug[:-1], ptr, node)
    with pytest.raises(_lib.TipkError, match='expected'):
        _run(model, q_rel.float(), q_drug, ptr, node)


def test_routes_identical_and_repeatable():
    L = _lib.lib()
    assert _lib.get_option('partner_rank_global') == 0
    for n, dim, n_q in cases.ROUTES:
        model, q_rel, q_drug, ptr, node, known = _dev(cases.routes_case(n, dim, n_q))
        fits = n < 2600
        assert L.tipk_distmult_partner_rank_lds_route(n, dim) == int(fits)
        a = _run(model, q_rel, q_drug, ptr, node, known)
        b = _run(model, q_rel, q_drug, ptr, node, known)
        assert _same(a, b), 'run to run'
        check_partner_rank(model, q_rel, q_drug, ptr, node, a, known)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                     # the single entry alone: no parallel branches
            c = _run(model, q_rel, q_drug, ptr, node, known)
        for x in c:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a, c), 'captured and replayed'
        if not fits:
            continue
        _lib.set_option('partner_rank_global', 1)
        try:
            assert L.tipk_distmult_partner_rank_lds_route(n, dim) == 0
            c = _run(model, q_rel, q_drug, ptr, node, known)
            d = _run(model, q_rel, q_drug, ptr, node, known)
        finally:
            _lib.set_option('partner_rank_global', 0)
        assert _same(c, d), ('global route, run to run', dim)
        assert _same(a, c), ('LDS vs global route', dim)


# ------------------------------------------------------------------ TIP.rank_partners
def _model_of(model):
    z = model.embeddings.detach()
    if model.decoder_kind == 'distmult':
        return ('distmult', z, model.decoder.weight.detach())
    dec = model.decoder
    with torch.no_grad():                                                 # the tables as NNDecoder.objective forms them
        s1t = ops.matmul(dec.w1_l2, torch.relu(ops.matmul(z, dec.w1_l1)).t())
        s2t = ops.matmul(dec.w2_l2, torch.relu(ops.matmul(z, dec.w2_l1)).t())
    return ('table', s1t, s2t)


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


def _keys_of(lists, n, n_rel):
    """(keys, ptr), relation-major, of the edge lists [(edge_index, range_list), ...] merged, with torch ops: what the
    screen's known lists hold for them."""
    comb = []
    for idx, rng in lists:
        ends = torch.as_tensor(rng).reshape(-1, 2)[:, 1].contiguous().long().to(idx.device)
        rel = torch.bucketize(torch.arange(idx.shape[1], device=idx.device), ends, right=True)
        comb.append(rel * (n * n) + idx[0].long() * n + idx[1].long())
    comb = torch.unique(torch.cat(comb))
    ptr = torch.zeros(n_rel + 1, dtype=torch.int64, device=comb.device)
    ptr[1:] = torch.cumsum(torch.bincount(torch.div(comb, n * n, rounding_mode='floor'), minlength=n_rel), 0)
    return comb % (n * n), ptr


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_rank_partners(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    m = _model_of(model)
    q_rel, q_drug, ptr, node, order = ops.targets_by_query(d.dd_test_idx, d.dd_test_et, n)
    train = _keys_of([(d.dd_train_idx, d.dd_train_range)], n, R)
    both = _keys_of([(d.dd_train_idx, d.dd_train_range), (d.dd_test_idx, d.dd_test_range)], n, R)
    reports = {}
    for flt, known in (('all', both), ('train', train), (None, None)):
        rep = model.rank_partners(filter=flt, ks=(1, 3, 10))
        reports[flt] = rep
        assert rep.rank.dtype == torch.int64 and rep.rank.shape == d.dd_test_et.shape == rep.logit.shape
        check_partner_rank(m, q_rel, q_drug, ptr, node, (rep.rank[order], rep.logit[order]), known)
        want = _report_numpy(rep.rank, d.dd_test_et, R, (1, 3, 10))
        assert abs(rep.mrr - want['mrr']) <= 1e-12 and abs(rep.macro_mrr - want['macro']) <= 1e-12
        assert all(abs(rep.hits[k] - want['hits'][k]) <= 1e-12 for k in (1, 3, 10)) and rep.unranked == want['unranked'] == 0
        again = utils.rank_report(rep.rank.cpu(), d.dd_test_et.cpu(), R, (1, 3, 10))
        assert abs(again['mrr'] - rep.mrr) <= 1e-12 and all(abs(again['hits'][k] - rep.hits[k]) <= 1e-12 for k in (1, 3, 10))
        np.testing.assert_allclose(rep.per_relation['mrr'].cpu().numpy(), want['per'], rtol=0, atol=1e-12, equal_nan=True)
    assert bool((reports['all'].rank <= reports['train'].rank).all()) and bool((reports['train'].rank <= reports[None].rank).all())
    assert reports['all'].mrr >= reports['train'].mrr >= reports[None].mrr
    given = model.rank_partners((d.dd_test_idx, d.dd_test_et), filter='train')
    assert torch.equal(given.rank, reports['train'].rank) and torch.equal(given.logit.view(torch.int32),
                                                                         reports['train'].logit.view(torch.int32))
    with pytest.raises(ValueError, match='out of range'):
        model.rank_partners((torch.tensor([[0], [n]]), torch.tensor([0])))
    if decoder != 'distmult':
        return

    # screen(drugs=..., exclude='train') holds a held-out partner of rank <= k at position rank - 1, unless the pair is a
    # training pair of the relation as well (then the screen drops it, while its rank stands)
    k = min(n - 1, 64)
    rep = reports['train']
    u, v, et = d.dd_test_idx[0], d.dd_test_idx[1], d.dd_test_et.long()
    sc = model.screen(k=k, drugs=torch.arange(n), exclude='train', sigmoid=False)       # row u * R + r
    fwd, rev = et * (n * n) + u * n + v, et * (n * n) + v * n + u
    tcomb = torch.repeat_interleave(torch.arange(R, device=DEV), train[1][1:] - train[1][:-1]) * (n * n) + train[0]
    in_train = torch.isin(fwd, tcomb) | torch.isin(rev, tcomb)
    use = (rep.rank <= k) & ~in_train
    assert int(use.sum()) >= 10
    row = u * R + et
    at = (rep.rank - 1).clamp(max=k - 1)[:, None]
    assert bool((sc.relation[row, 0] == et).all()) and bool((sc.u[row].long().gather(1, at)[:, 0] == u)[use].all())
    assert bool((sc.v[row].long().gather(1, at)[:, 0] == v)[use].all())
    assert torch.equal(sc.score[row].gather(1, at)[:, 0][use].view(torch.int32), rep.logit[use].view(torch.int32))


def test_biosnap_size_held_out_triples():
    """The held-out triples of relations 0..199 of the bundled graph (645 drugs), seeded random embeddings of dim 16, filter
    'all' (train and test keys): one launch on the LDS route, every rank against fp64, chunked on the device."""
    from tip_amd.data import build_data_dict
    d = build_data_dict()
    n, R = d['n_drug'], d['n_dd_et']
    keep = d['dd_test_et'] < 200
    q_rel, q_drug, ptr, node, order = ops.targets_by_query(d['dd_test_idx'][:, keep].to(DEV), d['dd_test_et'][keep].to(DEV), n)
    known = _keys_of([(d['dd_train_idx'].to(DEV), d['dd_train_range']), (d['dd_test_idx'].to(DEV), d['dd_test_range'])], n, R)
    model = cases.biosnap_weights(n, R)
    model = ('distmult', model[1].to(DEV), model[2].to(DEV))
    assert _lib.lib().tipk_distmult_partner_rank_lds_route(n, 16) == 1
    r, s = ops.distmult_partner_rank(model[1], model[2], q_rel, q_drug, ptr, node, known)
    share = check_partner_rank(model, q_rel, q_drug, ptr, node, (r, s), known, chunk=16384)
    print('biosnap: %d triples, %d queries, share of targets with two admissible ranks %.2e' % (node.numel(), q_rel.numel(), share))
    assert bool((r > 0).all())
    rep = utils.rank_report(r, q_rel[_owner(ptr)], R)
    assert rep['unranked'] == 0 and 0 < rep['mrr'] < 1
