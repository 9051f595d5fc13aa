"""GPU tests of the confidence path (include/tipk.h section 4p) against tests/conf_spec.py: `tipk_spd_factor`,
`tipk_distmult_pair_conf_topk`, the chain statistics -> factor -> query on the named cases, and the two `TIP` methods on the
small pickle."""
import math
import os

import pytest
import torch

import conf_cases as cases
import fit_cases
from conf_spec import check_end_to_end, check_factor, check_pair_conf, logical
from conftest import GOLDEN
from pair_topk_spec import check_pair_topk, known_from_dict
from tip_amd import _lib, ops
from tip_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0
SCALES = (1.0, 3.0 ** -0.5, 7600.0 ** -0.5)


def _bits(ts):
    return [None if t is None else t.contiguous().view(torch.int32).clone() for t in ts]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ------------------------------------------------------------------ factor
def _raw_factor(h, r):
    """tipk_spd_factor on device tensors; the outputs are pre-filled with a sentinel."""
    b, dim = h.shape[0], h.shape[1]
    out_l, out_w = torch.full_like(h, SENTINEL), torch.full_like(h, SENTINEL)
    status = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().tipk_spd_factor(ptr(h), ptr(r), b, dim, ptr(out_l), ptr(out_w), ptr(status), stream_ptr(DEV)), 'spd_factor')
    torch.cuda.synchronize()
    return out_l, out_w, status


def _factor_inputs(b, dim, seed):
    h = cases.spd_matrices(b, dim, seed).to(DEV)
    r = torch.tensor(SCALES, dtype=torch.float32)[torch.arange(b) % 3].to(DEV)
    return h, r


@pytest.mark.parametrize('dim', [1, 4, 12, 16, 20, 32])
def test_factor_widths_and_batches(dim):
    for b in (1, 3, 64, 65):
        h, r = _factor_inputs(b, dim, 10 * dim + b)
        got = _raw_factor(h, r)
        assert got[2].tolist() == [1] * b
        check_factor(h, r, got, what='dim%d b%d' % (dim, b))
        if b == 65:
            assert _same(got, _raw_factor(h, r))                             # two calls, equal bits
            alone = _raw_factor(h[7:8].contiguous(), r[7:8].contiguous())    # a row's bits do not depend on its neighbours
            assert _same([x[7:8] for x in got], alone)
            junk = h.clone()                                                 # only the lower triangle is read
            junk[:, torch.triu(torch.ones((dim, dim), dtype=torch.bool, device=DEV), 1)] = float('nan')
            assert _same(got, _raw_factor(junk, r))
            assert _same(got[:2], ops.spd_factor(h, r)[:2])


def test_factor_empty_batch_launches_nothing():
    assert _lib.lib().tipk_spd_factor(None, None, 0, 16, None, None, None, stream_ptr(DEV)) == 0
    out_l, out_w, status = ops.spd_factor(torch.zeros((0, 16, 16), device=DEV), torch.zeros(0, device=DEV))
    assert out_l.shape == (0, 16, 16) and out_w.shape == (0, 16, 16) and status.shape == (0,)


@pytest.mark.parametrize('dim', [1, 16, 20])
def test_factor_bad_rows_are_zero_and_touch_no_neighbour(dim):
    b = 9
    h, r = _factor_inputs(b, dim, 77 + dim)
    clean = _raw_factor(h, r)
    bad = h.clone()
    bad[1] = 0.0                                                             # a zero matrix
    bad[3, dim - 1, dim - 1] = -1.0                                          # a negative diagonal entry
    bad[5, dim - 1, 0] = float('nan')                                        # a NaN entry (lower triangle)
    bad[7, dim // 2, dim // 2] = float('inf')
    got = _raw_factor(bad, r)
    assert got[2].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    check_factor(bad, r, got, what='bad rows dim%d' % dim)
    for i in (0, 2, 4, 6, 8):
        assert _same([x[i] for x in got], [x[i] for x in clean]), i
        assert _same([x[i:i + 1] for x in got], _raw_factor(h[i:i + 1].contiguous(), r[i:i + 1].contiguous())), i
    rr = r.clone()
    rr[2] = float('inf')                                                     # a row scale that is not finite
    assert _raw_factor(h, rr)[2].tolist() == [1, 1, 0] + [1] * 6


# ------------------------------------------------------------------ query
def _raw_query(z, rel_w, w_fac, pairs, k, mode, c, known=None, dense=False):
    """tipk_distmult_pair_conf_topk on device tensors; the outputs are pre-filled with a sentinel."""
    n, dim = z.shape
    n_rel, n_p = rel_w.shape[0], pairs.shape[1]
    pu, pv = pairs[0].to(DEV, torch.int32).contiguous(), pairs[1].to(DEV, torch.int32).contiguous()
    keys = kptr = krel = None
    n_keys = 0
    if known is not None and known[0].numel() > 0:                           # (empty tensors have no address)
        keys, kptr, krel = known[0].to(DEV, torch.int64), known[1].to(DEV, torch.int64), known[2].to(DEV, torch.int32)
        n_keys = keys.numel()
    out = [torch.full((n_p, k), SENTINEL, device=DEV), torch.full((n_p, k), -7, dtype=torch.int32, device=DEV),
           torch.full((n_p, k), SENTINEL, device=DEV), torch.full((n_p, k), SENTINEL, device=DEV)]
    dl = torch.full((n_p, n_rel), SENTINEL, device=DEV) if dense else None
    dv = torch.full((n_p, n_rel), SENTINEL, device=DEV) if dense else None
    st = _lib.lib().tipk_distmult_pair_conf_topk(ptr(z), n, dim, ptr(rel_w), ptr(w_fac), n_rel, ptr(pu), ptr(pv), n_p, ptr(keys),
                                                 ptr(kptr), ptr(krel), n_keys, k, mode, c, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                                 ptr(out[3]), ptr(dl), ptr(dv), stream_ptr(DEV))
    _lib.check(st, 'pair_conf_topk')
    torch.cuda.synchronize()
    return tuple(out) + (dl, dv)


_QUERY = {}


def _query_case(n, dim, n_rel):
    if (n, dim, n_rel) not in _QUERY:
        _QUERY[(n, dim, n_rel)] = tuple(t.to(DEV) for t in cases.query_case(n, dim, n_rel, 1000 + n + 7 * dim + n_rel, 2.0))
    return _QUERY[(n, dim, n_rel)]


def _pairs(n, count, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, n, (2, count), generator=g)
    if count > 3:
        p[1, 2] = p[0, 2]                                                    # a self pair
        p[:, 3] = p[:, 1].flip(0)                                            # a pair and its mirror
    return p


def _known(n, n_rel, pairs):
    """Known lists: pair 0 with EVERY relation, pair 1 listed only in the other direction, a few random blocks."""
    d = {}
    p = pairs.tolist()
    if pairs.shape[1] > 0:
        d[(p[0][0], p[1][0])] = list(range(n_rel))
    if pairs.shape[1] > 1:
        d[(p[1][1], p[0][1])] = list(range(0, n_rel, 2))
    for i in range(4, pairs.shape[1], 5):
        d.setdefault((p[0][i], p[1][i]), [(i * 7 + j * 3) % n_rel for j in range(1 + i % 6)])
    return known_from_dict(d, n)


MODES = ((0, 0.0), (1, -1.645), (1, 0.0), (1, 2.0))


@pytest.mark.parametrize('n_rel', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('n_p', [0, 1, 15, 16, 17, 257])
def test_query_pair_and_relation_edges(n_p, n_rel):
    n, dim = 40, 16
    z, rel_w, w_fac = _query_case(n, dim, n_rel)
    pairs = _pairs(n, n_p, n_p + n_rel)
    known = _known(n, n_rel, pairs)
    mode, c = MODES[(n_p + n_rel) % 4]
    for k in (10, n_rel + 3) if n_rel < 126 else (10, 128):
        got = _raw_query(z, rel_w, w_fac, pairs, k, mode, c, known, dense=True)
        check_pair_conf(z, rel_w, w_fac, pairs, k, mode, c, got, known, what='P%d R%d k%d' % (n_p, n_rel, k))


@pytest.mark.parametrize('dim', [4, 12, 16, 20, 32])
def test_query_widths_modes_and_k(dim):
    n, n_rel, n_p = 33, 130, 37
    z, rel_w, w_fac = _query_case(n, dim, n_rel)
    z = z.clone()
    z[5] = 0.0                                                               # an all-zero row: s = var = 0 for its pairs
    pairs = _pairs(n, n_p, dim)
    pairs[0, 6] = 5
    pairs[:, 7] = 5
    known = _known(n, n_rel, pairs)
    for mode, c in MODES:
        for k in (0, 1, 10, 128):
            dense = _raw_query(z, rel_w, w_fac, pairs, k, mode, c, known, dense=True)
            check_pair_conf(z, rel_w, w_fac, pairs, k, mode, c, dense, known, what='dim%d mode%d c%g k%d' % (dim, mode, c, k))
            if k:
                plain = _raw_query(z, rel_w, w_fac, pairs, k, mode, c, known, dense=False)
                assert _same(plain[:4], dense[:4])                           # the same top-k bits with and without dense
                assert _same(dense, _raw_query(z, rel_w, w_fac, pairs, k, mode, c, known, dense=True))      # two calls
                free = _raw_query(z, rel_w, w_fac, pairs, k, mode, c, None)
                check_pair_conf(z, rel_w, w_fac, pairs, k, mode, c, free, None, what='no known lists')
        assert float(dense[4][6].abs().max()) == 0 and float(dense[5][7].max()) == 0
    # mode 1 with c = 0: the keys are the logits, and the rows are a pair top-k
    got = _raw_query(z, rel_w, w_fac, pairs, 10, 1, 0.0, known)
    assert torch.equal(got[0], got[2])
    check_pair_topk(('distmult', z, rel_w), pairs, 10, (got[0], got[1]), known)
    # one pair's bits do not depend on the rest of the call
    alone = _raw_query(z, rel_w, w_fac, pairs[:, 9:10], 10, 0, 0.0, known, dense=True)
    whole = _raw_query(z, rel_w, w_fac, pairs, 10, 0, 0.0, known, dense=True)
    assert _same([x[9:10] for x in whole], alone)
    # the wrapper is the entry
    via = ops.distmult_pair_conf_topk(z, rel_w, w_fac, pairs.to(DEV), 10, 'moderated', 0.0, tuple(t.to(DEV) for t in known), dense=True)
    assert _same(via, whole)


def test_query_out_of_range_pair_is_padding():
    n, dim, n_rel = 40, 16, 65
    z, rel_w, w_fac = _query_case(n, dim, n_rel)
    pairs = _pairs(n, 20, 5)
    pairs[0, 4], pairs[1, 11], pairs[0, 17] = n, -1, 2 ** 31 - 1
    got = _raw_query(z, rel_w, w_fac, pairs, 10, 0, 0.0, None, dense=True)
    check_pair_conf(z, rel_w, w_fac, pairs, 10, 0, 0.0, got, None, what='bad ids')
    for i in (4, 11, 17):
        assert got[1][i].tolist() == [-1] * 10 and bool(torch.isneginf(got[0][i]).all()) and bool(torch.isposinf(got[3][i]).all())


def test_query_refusals_write_nothing():
    L = _lib.lib()
    z, rel_w, w_fac = _query_case(40, 16, 65)
    pu = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.full((4, 10), SENTINEL, device=DEV)
    oi = torch.full((4, 10), -7, dtype=torch.int32, device=DEV)

    def call(k=10, mode=0, c=0.0, dl=None, dv=None, n_rel=65, dim=16):
        return L.tipk_distmult_pair_conf_topk(ptr(z), 40, dim, ptr(rel_w), ptr(w_fac), n_rel, ptr(pu), ptr(pu), 4, None, None, None,
                                              0, k, mode, c, ptr(out), ptr(oi), ptr(out), ptr(out), dl, dv, stream_ptr(DEV))
    assert call(k=-1) != 0 and call(mode=2) != 0 and call(c=float('nan')) != 0 and call(dl=ptr(out)) != 0
    assert call(k=129) != 0 and call(n_rel=0) != 0 and call(dim=6) != 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((oi == -7).all())


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize('name,n,dim,kind,l2', cases.END_TO_END)
def test_end_to_end(name, n, dim, kind, l2):
    z, lists, w = cases.end_to_end_case(n, dim, kind)
    z, w = z.to(DEV), w.to(DEV)
    fp = ops.fit_pairs_csr(lists, n)
    w_fac, out_l, status, hess = ops.distmult_posterior(z, w, fp, l2)
    assert status.tolist() == [1] * len(lists)
    scale = fp.n_pairs.double().rsqrt().float().to(DEV)
    check_factor(hess, scale, (out_l, w_fac, status), what=name)
    iu, iv = torch.triu_indices(n, n)
    pick = torch.arange(0, iu.numel(), max(1, iu.numel() // 600))
    pairs = torch.stack([iu[pick], iv[pick]]).to(DEV)
    got = ops.distmult_pair_conf_topk(z, w, w_fac, pairs, 2, 'moderated', 0.0, None, dense=True)
    check_pair_conf(z, w, w_fac, pairs, 2, 0, 0.0, got, None, what=name)
    check_end_to_end(z, w, hess, fp.n_pairs, pairs[0], pairs[1], got[5], what=name)


# ------------------------------------------------------------------ TIP on the small pickle
_MODELS = {}


def _model():
    from tip_amd.layers import TIP, Setting
    if 'cat' not in _MODELS:
        torch.manual_seed(0)
        st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
        _MODELS['cat'] = TIP(st, torch.device(DEV), mod='cat', data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
    return _MODELS['cat']


def _check_result(res, k, n_p):
    have = res.relation >= 0
    assert res.probability.shape == (n_p, k) and res.relation.dtype == torch.int64
    assert bool((res.std[have] >= 0).all())
    lo = torch.minimum(res.mean_probability, torch.full_like(res.mean_probability, 0.5))
    hi = torch.maximum(res.mean_probability, torch.full_like(res.mean_probability, 0.5))
    assert bool(((res.probability >= lo) & (res.probability <= hi))[have].all())       # between 1/2 and sigma(s)
    assert bool((res.probability[~have] == 0).all()) and bool((res.mean_probability[~have] == 0).all())


def test_tip_model_posterior():
    from tip_amd.layers import ConfidentSideEffects, DecoderPosterior
    model = _model()
    d = model.data
    z = model.embeddings.detach()
    rel = torch.arange(0, d.n_dd_et, 2)
    for relations in (None, rel):
        post = model.decoder_posterior(relations=relations)
        ids = torch.arange(d.n_dd_et) if relations is None else relations
        assert isinstance(post, DecoderPosterior) and post.known is None and post.relation.tolist() == ids.tolist()
        assert torch.equal(post.weight, model.decoder.weight.detach()[ids.to(DEV)])
        lists = []
        for r in ids.tolist():
            a, b = d.dd_train_range[r].tolist()
            blk = d.dd_train_idx[:, a:b].cpu()
            lists.append(sorted({(min(u, v), max(u, v)) for u, v in zip(blk[0].tolist(), blk[1].tolist())}))
        assert post.n_pairs.tolist() == [len(l) for l in lists]
        fp = ops.fit_pairs_csr(lists, d.n_drug)
        want = ops.distmult_posterior(z, post.weight, fp, 1e-4)
        assert torch.equal(post.factor.view(torch.int32), want[0].view(torch.int32))
        cov = post.covariance()
        assert torch.equal(cov, cov.transpose(1, 2)) and bool((cov.diagonal(dim1=1, dim2=2) > 0).all())
        pairs = torch.stack([d.dd_train_idx[0, ::97], d.dd_train_idx[1, ::97]]).to(DEV)
        for rank_by, mode, c in (('moderated', 0, 0.0), ('lower', 1, -1.645), ('upper', 1, 1.645)):
            for exclude in (None, 'train', 'all'):
                res = model.side_effects_confidence(pairs, post, k=5, rank_by=rank_by, exclude=exclude, dense=True)
                assert isinstance(res, ConfidentSideEffects)
                known = None
                if exclude is not None:
                    extra = (d.dd_test_idx, d.dd_test_range) if exclude == 'all' else None
                    known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, d.n_drug, extra=extra)
                    if relations is not None:
                        known = ops.restrict_known_relations(known, relations.to(DEV), d.n_dd_et)
                key, idx, logit, var, dl, dv = ops.distmult_pair_conf_topk(z, post.weight, post.factor, pairs, 5, mode, c, known, True)
                assert torch.equal(res.logit.view(torch.int32), logit.view(torch.int32))
                assert torch.equal(res.std.view(torch.int32), var.sqrt().view(torch.int32))
                assert torch.equal(res.dense_logit.view(torch.int32), dl.view(torch.int32))
                assert torch.equal(res.dense_std.view(torch.int32), dv.sqrt().view(torch.int32))
                assert torch.equal(res.relation, torch.where(idx >= 0, ids.to(DEV)[idx.long().clamp(min=0)], torch.full_like(idx, -1).long()))
                if rank_by == 'moderated':
                    have = idx >= 0
                    assert torch.equal(res.probability[have], torch.sigmoid(logit / torch.sqrt(1.0 + (math.pi / 8) * var))[have])
                _check_result(res, 5, pairs.shape[1])
                if exclude == 'train':                                       # a training side effect of the pair never comes back
                    seen = {(int(u), int(v), int(r)) for (u, v), r in zip(d.dd_train_idx.t().tolist(), d.dd_train_et.tolist())}
                    for i, (u, v) in enumerate(pairs.t().tolist()):
                        assert not any((u, v, r) in seen or (v, u, r) in seen for r in res.relation[i].tolist() if r >= 0)


def test_tip_posterior_of_fitted_rows():
    model = _model()
    d = model.data
    z = model.embeddings.detach()
    lists = [fit_cases.random_pairs(d.n_drug, 5, 1), fit_cases.random_pairs(d.n_drug, 60, 2), [(0, 1), (1, 0), (2, 2)]]
    fit = model.fit_side_effects(lists)
    post = model.decoder_posterior(lists, fit.weight)
    assert post.relation.tolist() == [0, 1, 2] and post.n_pairs.tolist() == [5, 60, 3]
    fp = ops.fit_pairs_csr(lists, d.n_drug)
    want = ops.distmult_posterior(z, fit.weight, fp, 1e-4)
    assert torch.equal(post.factor.view(torch.int32), want[0].view(torch.int32))
    keys, kptr, krel = (t.cpu() for t in post.known)
    assert keys.tolist() == sorted(keys.tolist()) and int(kptr[-1]) == krel.numel() == sum(len({(min(a, b), max(a, b)) for a, b in l}) for l in lists)
    cov = post.covariance()
    assert torch.equal(cov, cov.transpose(1, 2))
    # fewer recorded pairs: a wider posterior on the same scale of embeddings
    assert float(cov[0].diagonal().sum()) > float(cov[1].diagonal().sum())
    pairs = torch.tensor([[l[0][0] for l in lists] + [7], [l[0][1] for l in lists] + [9]], device=DEV)
    for exclude in (None, True):
        res = model.side_effects_confidence(pairs, post, k=3, rank_by='lower', z_score=2.0, exclude=exclude)
        key, idx, logit, var, _, _ = ops.distmult_pair_conf_topk(z, fit.weight, post.factor, pairs, 3, 'bound', -2.0,
                                                                  post.known if exclude else None)
        assert torch.equal(res.logit.view(torch.int32), logit.view(torch.int32)) and torch.equal(res.relation, idx.long())
        assert res.dense_logit is None and res.dense_std is None
        _check_result(res, 3, 4)
        for i in range(3):                                                   # the pair side effect i was given with
            assert (i in res.relation[i].tolist()) == (exclude is None)
    with pytest.raises(ValueError, match='positive definite'):
        model.decoder_posterior(lists, torch.full_like(fit.weight, float('nan')))


def test_tip_confidence_with_new_drugs():
    model = _model()
    d = model.data
    new = model.embed_new_drugs([[0, 1], [2]], [[(3, 0)], [(4, 1), (5, 1)]])
    n_all = d.n_drug + 2
    z_ext = torch.cat([model.embeddings.detach(), new.z])
    post = model.decoder_posterior(relations=[1, 4], new=new)            # the wider node set: more unrecorded pairs
    narrow = model.decoder_posterior(relations=[1, 4])
    assert post.n_pairs.tolist() == narrow.n_pairs.tolist() and not torch.equal(post.factor, narrow.factor)
    u, v = d.dd_train_idx[0, 5].item(), d.dd_train_idx[1, 5].item()      # a recorded pair, and pairs with the new drugs
    pairs = torch.tensor([[u, d.n_drug, d.n_drug + 1], [v, 3, d.n_drug]], device=DEV)
    res = model.side_effects_confidence(pairs, post, k=2, exclude='train', dense=True, new=new)
    known = ops.restrict_known_relations(ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, d.n_drug),
                                         post.relation, d.n_dd_et)
    keys = torch.div(known[0], d.n_drug, rounding_mode='floor') * n_all + known[0] % d.n_drug
    want = ops.distmult_pair_conf_topk(z_ext, post.weight, post.factor, pairs, 2, 0, 0.0, (keys, known[1], known[2]), True)
    assert torch.equal(res.logit.view(torch.int32), want[2].view(torch.int32))
    assert torch.equal(res.relation, torch.where(want[1] >= 0, post.relation[want[1].long().clamp(min=0)], -torch.ones_like(want[1]).long()))
    check_pair_conf(z_ext, post.weight, post.factor, pairs, 2, 0, 0.0, want, (keys, known[1], known[2]), what='new drugs')
    recorded = {int(r) for (a, b), r in zip(d.dd_train_idx.t().tolist(), d.dd_train_et.tolist()) if {a, b} == {u, v}}
    assert not (set(res.relation[0].tolist()) & recorded)
    assert sorted(res.relation[1].tolist()) == [1, 4]                    # nothing is recorded for a new drug
    with pytest.raises(ValueError, match='out of range'):
        model.side_effects_confidence(pairs, post, k=2)                  # without `new` the ids are out of range
