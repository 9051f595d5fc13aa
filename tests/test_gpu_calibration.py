"""-m gpu: the per-relation calibration (include/tipk.h section 4r, tip_amd/csrc/tipk_calibrate.hip) against the fp64 spec and the
acceptance rules of tests/calibration_spec.py.  The statistics and the fit are tested through the C entries themselves, with
outputs pre-filled with a sentinel; then `TIP.calibrate` and the `calibration=` keyword of the queries on the small pickle."""
import inspect
import os

import pytest
import torch

import calibration_cases as cases
from calibration_spec import C_CAL, U, cell_sets, check_fit, check_stats, spec_stats
from conftest import GOLDEN
from pair_topk_spec import check_pair_topk, logits64
from partner_sum_spec import C_PROFILE, check_partner_sum
from tip_amd import _lib, ops
from tip_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0
STATS = {c['name']: c for c in cases.stats_cases()}
FITS = {c['name']: c for c in cases.fit_cases()}
_SHARED = {}                                   # per case: the lists, the sets and the spec's tables, computed once


def _chain(n, dim, n_q):
    return _lib.lib().tipk_distmult_calibrate_max_chain(n, dim, max(n_q, 1))


def _shared(case):
    """(cl, sets) of a case: the device lists of `ops.calibration_lists` and the brute-force sets of the spec."""
    if case['name'] not in _SHARED:
        n = case['z'].shape[0]
        cl = ops.calibration_lists(case['train'], case['given'], n, case['w'].shape[0], case['relations'])
        _SHARED[case['name']] = (cl, cell_sets(case['train'], case['given'], n, case['relations']))
    return _SHARED[case['name']]


def _lists_on_device(cl):
    return [t.to(DEV).contiguous() for t in (cl.q_rel, cl.dense_w, cl.ptr, cl.u, cl.v, cl.wpos, cl.wneg)]


def _workspace(n, dim, n_q):
    nbytes = _lib.lib().tipk_distmult_calibrate_workspace_bytes(n, dim, n_q)
    assert nbytes >= 0
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)


def _raw_stats(z, w, ab, cl, l2=cases.L2, active=None, out=None, spare=0):
    """tipk_distmult_calibrate_stats on device tensors; the outputs are pre-filled with a sentinel (`spare` more rows than
    queries, to see that nothing is written behind the last query)."""
    n, dim = z.shape
    q = cl.q_rel.numel()
    qrel, dense, pptr, pu, pv, wpos, wneg = _lists_on_device(cl)
    if out is None:
        out = (torch.full((q + spare,), SENTINEL, device=DEV), torch.full((q + spare, 2), SENTINEL, device=DEV),
               torch.full((q + spare, 2, 2), SENTINEL, device=DEV))
    ws = _workspace(n, dim, q)
    act = None if active is None else active.to(DEV, torch.int32).contiguous()
    st = _lib.lib().tipk_distmult_calibrate_stats(ptr(z), n, dim, ptr(w), w.shape[0], ptr(qrel), ptr(ab), q, ptr(dense),
                                                  ptr(pptr), ptr(pu), ptr(pv), ptr(wpos), ptr(wneg), pu.numel(), l2, ptr(act),
                                                  ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), stream_ptr(DEV))
    _lib.check(st, 'calibrate stats')
    torch.cuda.synchronize()
    return out


def _raw_fit(z, w, cl, l2, init, max_iter, gtol, spare=0):
    """tipk_distmult_calibrate on device tensors -> (ab, loss, grad, info), pre-filled with a sentinel."""
    n, dim = z.shape
    q = cl.q_rel.numel()
    qrel, dense, pptr, pu, pv, wpos, wneg = _lists_on_device(cl)
    ab, loss, grad = (torch.full(s, SENTINEL, device=DEV) for s in ((q + spare, 2), (q + spare,), (q + spare, 2)))
    info = torch.full((q + spare, 4), -7, dtype=torch.int32, device=DEV)
    ws = _workspace(n, dim, q)
    st = _lib.lib().tipk_distmult_calibrate(ptr(z), n, dim, ptr(w), w.shape[0], ptr(qrel), q, ptr(dense), ptr(pptr), ptr(pu),
                                            ptr(pv), ptr(wpos), ptr(wneg), pu.numel(), l2, ptr(init), max_iter, gtol, ptr(ab),
                                            ptr(loss), ptr(grad), ptr(info), ptr(ws), stream_ptr(DEV))
    _lib.check(st, 'calibrate')
    torch.cuda.synchronize()
    return ab, loss, grad, info


def _bits(ts):
    return [t.contiguous().view(torch.int32).clone() for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('name', list(STATS))
def test_stats_against_the_spec(name):
    """Every shape and list kind at three trial points; nothing behind the last query is written; two calls give equal bits."""
    case = STATS[name]
    cl, sets = _shared(case)
    z, w = case['z'].to(DEV), case['w'].to(DEV)
    n, dim = z.shape
    q = cl.q_rel.numel()
    assert _lib.lib().tipk_distmult_calibrate_splits(n, dim, q) == min(max(4096 // q, 1), 64, ((n + 63) // 64) * ((n + 63) // 64 + 1) // 2)
    for point, ab in cases.trial_points(cl.n_pos, cl.n_neg).items():
        ab = ab.to(DEV)
        got = _raw_stats(z, w, ab, cl, spare=3)
        for v in got:
            assert bool((v[q:] == SENTINEL).all())
        got = tuple(v[:q] for v in got)
        spec = spec_stats(z, w, ab, case['train'], case['given'], case['relations'], cases.L2, sets=sets)
        check_stats(got, spec, _chain(n, dim, q), what='%s %s' % (name, point))
        assert bool(torch.isfinite(got[0]).all())
        assert torch.equal(got[2][:, 0, 1], got[2][:, 1, 0])
        assert _same_bits(got, _raw_stats(z, w, ab, cl)), 'call to call'
        if point == 'identity':                                          # a query with M = 0 has the l2 term alone: nothing
            empty = (cl.n_pos + cl.n_neg) == 0
            assert bool((got[0].cpu()[empty] == 0).all()) and bool((got[1].cpu()[empty] == 0).all())


def test_stats_nan_row_and_infinite_entry():
    case = STATS['n65_d36_q5']
    cl, sets = _shared(case)
    w = case['w'].to(DEV)
    ab = cases.trial_points(cl.n_pos, cl.n_neg)['prevalence'].to(DEV)
    chain = _chain(65, 36, 5)
    # a NaN row of z reaches every query that has terms (every query streams every cell); M = 0 keeps the l2 term alone
    z = cases.with_nan_row(case['z'], 64).to(DEV)
    got = _raw_stats(z, w, ab, cl)
    spec = spec_stats(z, w, ab, case['train'], case['given'], case['relations'], cases.L2, sets=sets)
    sees = torch.tensor([k != 'full' for k in case['kinds']], device=DEV)                    # M > 0: the query has terms
    assert torch.equal(torch.isnan(spec['loss']), sees) and int(sees.sum()) == 4
    check_stats(got, spec, chain, what='nan row')
    assert all(bool(torch.isnan(v[sees]).all()) and bool(torch.isfinite(v[~sees]).all()) for v in got)
    # an infinite entry: t = +-inf on a row of cells.  dL/db and H_bb stay finite and within the rule; dL/da and the other
    # Hessian entries are non-finite; nothing finite is invented
    z = cases.with_inf_entry(case['z'], 3, 5).to(DEV)
    got = _raw_stats(z, w, ab, cl)
    spec = spec_stats(z, w, ab, case['train'], case['given'], case['relations'], cases.L2, sets=sets)
    check_stats(got, spec, chain, what='inf entry')
    assert bool(torch.isfinite(got[1][sees, 1]).all()) and bool(torch.isfinite(got[2][sees, 1, 1]).all())
    assert not bool(torch.isfinite(got[1][sees, 0]).any()) and not bool(torch.isfinite(got[2][sees, 0, 0]).any())
    assert not bool(torch.isfinite(got[2][sees, 0, 1]).any()) and not bool(torch.isfinite(got[0][sees]).any())


def test_nan_isolation():
    """A NaN in one relation's decoder row, and one in another query's (a, b), make exactly those two queries NaN."""
    case = STATS['n130_d16_q5']
    cl, sets = _shared(case)
    z, w = case['z'].to(DEV), case['w'].clone()
    w[int(case['relations'][1]), 7] = float('nan')
    w[0, 2] = float('nan')                                               # the side effect nobody queries
    w = w.to(DEV)
    ab = cases.trial_points(cl.n_pos, cl.n_neg)['prevalence']
    ab[3, 0] = float('nan')
    ab = ab.to(DEV)
    got = _raw_stats(z, w, ab, cl)
    spec = spec_stats(z, w, ab, case['train'], case['given'], case['relations'], cases.L2, sets=sets)
    assert torch.isnan(spec['loss']).tolist() == [False, True, False, True, False]
    check_stats(got, spec, _chain(130, 16, 5), what='nan isolation')
    clean = _raw_stats(z, case['w'].to(DEV), cases.trial_points(cl.n_pos, cl.n_neg)['prevalence'].to(DEV), cl)
    for a, b in zip(_bits(got), _bits(clean)):                           # the others keep their bits
        assert torch.equal(a[[0, 2, 4]], b[[0, 2, 4]])


def test_active_mask():
    case = STATS['n65_d4_q70']
    cl, _ = _shared(case)
    z, w = case['z'].to(DEV), case['w'].to(DEV)
    ab = cases.trial_points(cl.n_pos, cl.n_neg)['prevalence'].to(DEV)
    full = _raw_stats(z, w, ab, cl)
    active = (torch.arange(70) % 3 != 1).to(torch.int32)
    got = _raw_stats(z, w, ab, cl, active=active)
    on = active.bool().to(DEV)
    for a, b, v in zip(_bits(got), _bits(full), got):
        assert torch.equal(a[on], b[on])                                 # an active query does not depend on the mask
        assert bool((v[~on] == SENTINEL).all())                          # an inactive query's rows are not touched
    none = _raw_stats(z, w, ab, cl, active=torch.zeros(70, dtype=torch.int32))
    assert all(bool((v == SENTINEL).all()) for v in none)


def test_empty_call():
    L = _lib.lib()
    assert L.tipk_distmult_calibrate_stats(None, 5, 16, None, 3, None, None, 0, None, None, None, None, None, None, 0, 1e-6, None,
                                           None, None, None, None, stream_ptr(DEV)) == 0
    assert L.tipk_distmult_calibrate(None, 5, 16, None, 3, None, 0, None, None, None, None, None, None, 0, 1e-6, None, 4, 1e-6,
                                     None, None, None, None, None, stream_ptr(DEV)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize('name', list(FITS))
def test_fit_against_the_spec(name):
    """From the prevalence start every fit case ends with status 1 within 16 evaluations (tests/test_host_calibration.py holds
    the fp64 rule to that), and the result obeys (a)-(e) of the spec; equal bits call to call; sentinels stay."""
    case = FITS[name]
    cl, sets = _shared(case)
    z, w = case['z'].to(DEV), case['w'].to(DEV)
    n, dim = z.shape
    q = cl.q_rel.numel()
    start = cases.prevalence_start(cl.n_pos, cl.n_neg).to(DEV)
    max_iter = cases.MAX_EVALUATIONS - 1
    got = _raw_fit(z, w, cl, cases.L2, start, max_iter, cases.GTOL, spare=2)
    for v in got[:3]:
        assert bool((v[q:] == SENTINEL).all())
    assert bool((got[3][q:] == -7).all())
    ab, loss, grad, info = (v[:q] for v in got)
    print(name, 'status', info[:, 0].tolist(), 'evaluations', info[:, 1].tolist())
    assert info[:, 0].tolist() == [1] * q, info.tolist()
    assert bool((grad.abs().amax(1) <= cases.GTOL).all())
    check_fit(z, w, case['train'], case['given'], case['relations'], cases.L2, start, max_iter, cases.GTOL, (ab, info),
              _chain(n, dim, q), what=name, sets=sets)
    # the reported loss and gradient are the statistics at the accepted map, bit for bit
    at = _raw_stats(z, w, ab.contiguous(), cl)
    assert _same_bits((loss, grad), at[:2])
    assert _same_bits(got, _raw_fit(z, w, cl, cases.L2, start, max_iter, cases.GTOL, spare=2)), 'call to call'


def test_fit_defaults_and_capture():
    """init NULL starts at the identity; max_iter 0 is one evaluation; the entry alone captures and replays to equal bits."""
    case = FITS['n65_d16_q5']
    cl, sets = _shared(case)
    z, w = case['z'].to(DEV), case['w'].to(DEV)
    ab, loss, grad, info = _raw_fit(z, w, cl, cases.L2, None, 0, cases.GTOL)
    assert ab.tolist() == [[1.0, 0.0]] * 5 and info.tolist() == [[0, 1, 0, 0]] * 5
    ident = torch.tensor([[1.0, 0.0]], device=DEV).repeat(5, 1)
    assert _same_bits((loss, grad), _raw_stats(z, w, ident, cl)[:2])
    dev_cl = cl._replace(**{k: getattr(cl, k).to(DEV) for k in ('ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w', 'q_rel')})
    start = cases.prevalence_start(cl.n_pos, cl.n_neg).to(DEV)
    a = ops.distmult_calibrate(z, w, dev_cl, cases.L2, start, 15, cases.GTOL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # the single entry alone: sequential launches
        c = ops.distmult_calibrate(z, w, dev_cl, cases.L2, start, 15, cases.GTOL)
    for v in c:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(a, c), 'captured and replayed'
    assert a[3][:, 0].tolist() == [1] * 5
    s = ops.distmult_calibrate_stats(z, w, a[0], dev_cl, cases.L2)
    torch.cuda.synchronize()
    assert _same_bits(s[:2], a[1:3])


# ------------------------------------------------------------------ TIP.calibrate and the calibration= keyword on the small pickle
_MODELS = {}


def _model():
    from tip_amd.layers import TIP, Setting
    if 'cat' not in _MODELS:
        torch.manual_seed(0)
        st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
        model = TIP(st, torch.device(DEV), mod='cat', data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
        _MODELS['cat'] = (model, model.calibrate())
    return _MODELS['cat']


def test_tip_calibrate():
    from tip_amd.layers import Calibration
    model, cal = _model()
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    assert isinstance(cal, Calibration) and cal.z.shape == (n, 20) and cal.decoder.in_dim == 20 and cal.decoder.num_et == R
    assert all(getattr(cal, f).shape == (R,) for f in ('scale', 'offset', 'loss', 'loss_raw', 'expected_raw', 'n_pos', 'n_neg',
                                                       'n_dropped', 'evaluations', 'status'))
    assert all(getattr(cal, f).dtype == torch.int64 for f in ('n_pos', 'n_neg', 'n_dropped', 'evaluations', 'status'))
    assert not cal.z.requires_grad and not cal.decoder.weight.requires_grad and model.decoder.weight.requires_grad
    assert 'decoder' in dict(model.named_modules()) and all(m is not cal.decoder for m in model.modules())
    train, given, rel = (d.dd_train_idx, d.dd_train_et), (d.dd_test_idx, d.dd_test_et), torch.arange(R)
    sets = cell_sets(train, given, n, rel)
    ident = torch.tensor([[1.0, 0.0]], device=DEV).repeat(R, 1)
    raw = spec_stats(z, w, ident, train, given, rel, 0.0, sets=sets)
    assert cal.n_pos.tolist() == raw['n_pos'].tolist() and cal.n_neg.tolist() == raw['n_neg'].tolist()
    assert cal.n_dropped.tolist() == raw['n_dropped'].tolist()
    chain = _chain(n, 16, R)
    # loss_raw and expected_raw: ONE statistics call at (1, 0).  expected = M dL/db + n_pos, so M times the bound of dL/db
    bound_l = raw['T_loss'] + (chain + C_CAL) * U * raw['A_loss']
    assert bool(((cal.loss_raw.double() - raw['loss']).abs() <= bound_l).all())
    m = (raw['n_pos'] + raw['n_neg']).double().to(DEV)
    bound_e = m * (raw['T_g'][:, 1] + (chain + C_CAL) * U * raw['A_g'][:, 1]) + 2 * U * raw['expected']   # + the fp32 result
    print('expected_raw', cal.expected_raw.tolist(), 'held out', cal.n_pos.tolist())
    assert bool(((cal.expected_raw.double() - raw['expected']).abs() <= bound_e).all())
    # the fit: both classes present -> fitted from the prevalence start, status 1 (every side effect of this pickle; the empty
    # classes are test_tip_calibrate_empty_classes_on_the_small_pickle and test_tip_calibrate_every_list_kind)
    fitted = ((raw['n_pos'] > 0) & (raw['n_neg'] > 0)).to(DEV)
    assert bool(fitted.any())
    assert bool((cal.status[fitted] == 1).all()), cal.status.tolist()
    assert bool((cal.status[~fitted] == 4).all()) and bool((cal.scale[~fitted] == 1).all()) and bool((cal.offset[~fitted] == 0).all())
    idx = torch.nonzero(fitted).reshape(-1).cpu()
    start = cases.prevalence_start(raw['n_pos'][idx], raw['n_neg'][idx])
    ab = torch.stack([cal.scale, cal.offset], 1)[idx.to(DEV)]
    info = torch.stack([cal.status, cal.evaluations, cal.evaluations - 1, torch.zeros_like(cal.status)], 1)[idx.to(DEV)]
    sub = (sets[0], sets[1], sets[2][idx], sets[3][idx], sets[4][idx])
    defaults = {k: p.default for k, p in inspect.signature(model.calibrate).parameters.items()}
    assert defaults['l2'] == 1e-6 and defaults['max_iter'] == 32
    res = check_fit(z, w, train, given, idx, defaults['l2'], start, defaults['max_iter'], defaults['gtol'], (ab, info), chain,
                    what='tip', sets=sub)
    # the calibrated model expects fewer positives than the raw one: the inflation the calibration removes
    assert bool((res['at_w']['expected'] < raw['expected'][idx.to(DEV)]).all())
    # the widened decoder holds the map
    assert torch.equal(cal.decoder.weight[:, :16], cal.scale[:, None] * w) and torch.equal(cal.decoder.weight[:, 16], cal.offset)
    # relations: the others keep the identity and status 4; an init is taken
    some = idx[:2].tolist()
    part = model.calibrate(relations=some, init=torch.stack([cal.scale, cal.offset], 1))
    keep = torch.zeros(R, dtype=torch.bool, device=DEV)
    keep[some] = True
    assert bool((part.status[keep] == 1).all()) and bool((part.status[~keep] == 4).all())
    assert bool((part.scale[~keep] == 1).all()) and bool((part.offset[~keep] == 0).all())
    assert bool((part.evaluations[keep] <= 2).all())                     # it starts where the first fit ended
    # given pairs: both directions are one pair
    e = d.dd_test_idx
    twice = model.calibrate(pairs=(torch.cat([e, e.flip(0)], 1), torch.cat([d.dd_test_et, d.dd_test_et])))
    assert _same_bits((twice.scale, twice.offset, twice.loss), (cal.scale, cal.offset, cal.loss))


def test_tip_calibrate_empty_classes_on_the_small_pickle():
    """A side effect without a given pair, and one whose given pairs are all training pairs, are not sent to the fit: status 4,
    the identity, no evaluation; the others are fitted."""
    model, full = _model()
    d = model.data
    R = d.n_dd_et
    none, trained = 0, 2
    keep = (d.dd_test_et != none) & (d.dd_test_et != trained)
    tr = d.dd_train_idx[:, d.dd_train_et == trained][:, :40]
    assert tr.shape[1] == 40
    given = (torch.cat([d.dd_test_idx[:, keep], tr.flip(0)], 1),                       # the training pairs the other way round
             torch.cat([d.dd_test_et[keep], torch.full((40,), trained, dtype=d.dd_test_et.dtype, device=tr.device)]))
    cal = model.calibrate(pairs=given)
    empty = torch.zeros(R, dtype=torch.bool, device=DEV)
    empty[[none, trained]] = True
    assert int(empty.sum()) == 2 and int((~empty).sum()) == R - 2
    assert cal.status[empty].tolist() == [4, 4] and cal.evaluations[empty].tolist() == [0, 0]
    assert cal.scale[empty].tolist() == [1.0, 1.0] and cal.offset[empty].tolist() == [0.0, 0.0]
    assert cal.n_pos[empty].tolist() == [0, 0] and int(cal.n_dropped[none]) == 0
    distinct = torch.unique(torch.minimum(tr[0], tr[1]) * d.n_drug + torch.maximum(tr[0], tr[1])).numel()
    assert int(cal.n_dropped[trained]) == distinct > 0
    assert bool((cal.n_neg[empty] > 0).all()) and _same_bits((cal.loss[empty],), (cal.loss_raw[empty],))
    assert torch.equal(cal.decoder.weight[empty][:, :16], model.decoder.weight.detach()[empty])
    assert bool((cal.decoder.weight[empty][:, 16:] == 0).all())
    # the rest: the lists of the other side effects are those of the plain call, so are the maps, bit for bit
    assert bool((cal.status[~empty] == 1).all()) and bool((cal.evaluations[~empty] > 0).all())
    assert _same_bits((cal.scale[~empty], cal.offset[~empty], cal.loss[~empty]),
                      (full.scale[~empty], full.offset[~empty], full.loss[~empty]))
    assert torch.equal(cal.n_pos[~empty], full.n_pos[~empty]) and bool((cal.n_pos[~empty] > 0).all())


def test_tip_calibrate_every_list_kind():
    """`TIP.calibrate` on a case that holds every list kind, among them a side effect whose every cell is trained (no negative,
    M = 0) and one with nothing given (no positive): those two keep the identity with status 4 and are never evaluated, the
    others are fitted from the prevalence start and obey the spec."""
    import types
    from tip_amd.layers import TIP
    case = STATS['n65_d36_q5']
    z, w = case['z'].to(DEV), case['w'].to(DEV)
    n, R = z.shape[0], w.shape[0]
    data = types.SimpleNamespace(n_drug=n, n_dd_et=R, dd_train_idx=case['train'][0], dd_train_et=case['train'][1],
                                 dd_test_idx=case['given'][0], dd_test_et=case['given'][1])
    model = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, embeddings=z,
                                  decoder=types.SimpleNamespace(in_dim=36, num_et=R, weight=w))
    cal = TIP.calibrate(model)
    kind_of = {int(r): k for r, k in zip(case['relations'].tolist(), case['kinds'])}
    kind_of[0] = 'mixed'                                                 # the side effect the case never queries
    kinds = [kind_of[r] for r in range(R)]
    assert sorted(kinds) == ['full', 'mixed', 'mixed', 'nopos', 'separable', 'untrained']
    empty = torch.tensor([k in ('full', 'nopos') for k in kinds], device=DEV)
    rel = torch.arange(R)
    sets = cell_sets(case['train'], case['given'], n, rel)
    raw = spec_stats(z, w, torch.tensor([[1.0, 0.0]], device=DEV).repeat(R, 1), case['train'], case['given'], rel, 0.0, sets=sets)
    assert cal.n_pos.tolist() == raw['n_pos'].tolist() and cal.n_neg.tolist() == raw['n_neg'].tolist()
    assert cal.n_dropped.tolist() == raw['n_dropped'].tolist()
    full_r, nopos_r = kinds.index('full'), kinds.index('nopos')
    assert int(cal.n_neg[full_r]) == 0 and int(cal.n_pos[full_r]) == 0 and int(cal.n_dropped[full_r]) == 2
    assert int(cal.n_pos[nopos_r]) == 0 and int(cal.n_neg[nopos_r]) > 0
    assert cal.status[empty].tolist() == [4, 4] and cal.evaluations[empty].tolist() == [0, 0]
    assert cal.scale[empty].tolist() == [1.0, 1.0] and cal.offset[empty].tolist() == [0.0, 0.0]
    assert float(cal.loss_raw[full_r]) == 0.0 and float(cal.expected_raw[full_r]) == 0.0
    assert bool((cal.status[~empty] == 1).all()), cal.status.tolist()
    idx = torch.nonzero(~empty).reshape(-1).cpu()
    start = cases.prevalence_start(raw['n_pos'][idx], raw['n_neg'][idx])
    ab = torch.stack([cal.scale, cal.offset], 1)[idx.to(DEV)]
    info = torch.stack([cal.status, cal.evaluations, cal.evaluations - 1, torch.zeros_like(cal.status)], 1)[idx.to(DEV)]
    sub = (sets[0], sets[1], sets[2][idx], sets[3][idx], sets[4][idx])
    check_fit(z, w, case['train'], case['given'], idx, 1e-6, start, 32, 1e-6, (ab, info), _chain(n, 36, R), what='every kind',
              sets=sub)
    assert cal.z.shape == (n, 40) and cal.decoder.in_dim == 40


def test_calibrated_side_effects_and_profile():
    model, cal = _model()
    d = model.data
    n, R, dim = d.n_drug, d.n_dd_et, 16
    z64, w64 = model.embeddings.detach().double(), model.decoder.weight.detach().double()
    a64, b64 = cal.scale.double(), cal.offset.double()
    g = torch.Generator().manual_seed(8)
    pairs = torch.randint(0, n, (2, 150), generator=g).to(DEV)
    wide = ('distmult', cal.z, cal.decoder.weight.detach())
    # side_effects: every side effect of every pair, against sigma(a s + b) from fp64 within the pair top-k's tau for the
    # widened operands ((dim' + 2) U sum_k |z'_u z'_v w'_r|, dim' = dim + 4: the rounding of a w is one of its roundings)
    res = model.side_effects(pairs, k=R, exclude=None, sigmoid=False, calibration=cal)
    check_pair_topk(wide, pairs, R, res, None)
    s = (z64[pairs[0]] * z64[pairs[1]]) @ w64.t()                        # [P, R]
    want = a64[None, :] * s + b64[None, :]
    _, tau = logits64(wide, pairs[0], pairs[1])
    got = torch.empty_like(want).scatter_(1, res.relation, res.score.double())
    assert bool(((got - want).abs() <= tau).all()), float(((got - want).abs() - tau).max())
    prob = model.side_effects(pairs, k=R, exclude=None, calibration=cal)
    assert torch.equal(prob.relation, res.relation) and torch.equal(prob.score, torch.sigmoid(res.score))
    gotp = torch.empty_like(want).scatter_(1, prob.relation, prob.score.double())
    assert bool(((gotp - torch.sigmoid(want)).abs() <= tau / 4 + 2 * U).all())
    # drug_profile: the partner sum's rule on the widened operands, then the same bound against sum_c sigma(a s + b)
    drugs = torch.arange(n, device=DEV)
    prof = model.drug_profile(k=4, exclude=None, calibration=cal)
    t = check_partner_sum(wide, drugs, 4, (prof.expected, prof.candidates, prof.top_expected, prof.top_relation),
                          what='calibrated profile')
    sig = torch.sigmoid(a64[None, None, :] * torch.einsum('uk,ck,rk->ucr', z64, z64, w64) + b64[None, None, :])
    sig[drugs, drugs] = 0.0                                              # a drug is no partner of itself
    e64 = sig.sum(1)                                                     # [n, R]
    bound = t['T_tau'] + (t['count'].double() + C_PROFILE) * U * e64
    off = (prof.expected.double() - e64).abs()
    assert bool((off <= bound).all()), float((off - bound).max())
    plain = model.drug_profile(k=4, exclude='all')
    with_cal = model.drug_profile(k=4, exclude='all', calibration=cal)
    assert torch.equal(plain.candidates, with_cal.candidates)            # who is summed over does not depend on the map
    fitted = cal.status == 1
    assert float(with_cal.expected[:, fitted].sum()) < float(plain.expected[:, fitted].sum())   # the inflation is gone
    # new drugs are widened by embed
    from tip_amd.layers import NewDrugs
    new = NewDrugs(None, None, model.embeddings.detach()[:3].clone(), None, None)
    ext = model.drug_profile([n, n + 2, 1], k=2, exclude=None, new=new, calibration=cal)
    # new drug i has the row of drug i, which is itself a partner of it here: its sum is drug i's plus sigma of (i, i)
    self_term = torch.sigmoid(a64[None, :] * ((z64[:3] * z64[:3]) @ w64.t()) + b64[None, :])
    want_new = e64[[0, 2]] + self_term[[0, 2]]
    assert torch.allclose(ext.expected[:2].double(), want_new, rtol=1e-4, atol=0)
    assert torch.allclose(ext.expected[2].double(), e64[1], rtol=1e-4, atol=0)


def test_calibrated_screen_keeps_the_pairs():
    """Rankings within one side effect do not change for scale > 0: the calibrated screen returns the pairs of the plain one.
    Both rank by their own fp32 logit, each within its bound of the exact one, so two pairs may swap only where their exact
    raw logits differ by at most tau_p (the plain screen's bound) + tau' / scale (the bound of the widened operands, (dim' +
    2) U sum_k |z'_u z'_v w'_r|, brought back to the raw scale)."""
    from tip_amd.layers import calibrated_operands
    model, fitted = _model()
    d = model.data
    n, R, dim = d.n_drug, d.n_dd_et, 16
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    # the fitted maps where their scale is positive; a map with a positive scale of that size elsewhere (an untrained model
    # need not give one)
    scale = torch.where(fitted.scale > 0, fitted.scale, fitted.scale.abs().clamp(min=0.05))
    wide, dec = calibrated_operands(z, w, torch.stack([scale, fitted.offset], 1))
    cal = fitted._replace(scale=scale, z=wide, decoder=dec)
    k = 12
    plain = model.screen(k=k, exclude='train', sigmoid=False)
    calib = model.screen(k=k, exclude='train', sigmoid=False, calibration=cal)
    assert torch.equal(plain.relation, calib.relation) and plain.u.shape == calib.u.shape == (R, k)
    z64, w64, a64, b64 = z.double(), w.double(), scale.double(), fitted.offset.double()
    agree = 0
    for r in range(R):
        pu, pv, cu, cv = (t[r].long() for t in (plain.u, plain.v, calib.u, calib.v))
        assert bool((pu >= 0).all()) and bool((cu >= 0).all()) and bool((cu < cv).all())
        fp, fc = z64[pu] * z64[pv] * w64[r], z64[cu] * z64[cv] * w64[r]
        s_p, s_c = fp.sum(1), fc.sum(1)
        tau_p = (dim + 2) * U * fp.abs().sum(1)
        tau_c = (dim + 4 + 2) * U * (a64[r] * fc.abs().sum(1) + b64[r].abs())
        # the calibrated scores are a s + b of their own pairs
        assert bool(((calib.score[r].double() - (a64[r] * s_c + b64[r])).abs() <= tau_c).all())
        differs = (pu != cu) | (pv != cv)
        agree += int((~differs).sum())
        assert bool(((s_p - s_c).abs() <= tau_p + tau_c / a64[r])[differs].all()), (r, 'a clearly ranked pair moved')
    assert agree > 0


def test_calibration_none_is_the_plain_call():
    """calibration=None runs the code the call without the keyword runs: equal bits for all six queries."""
    model, cal = _model()
    n = model.data.n_drug
    g = torch.Generator().manual_seed(9)
    pairs = torch.randint(0, n, (2, 40), generator=g)
    regs = [[0, 3, 5], [2, 7], [1, 4, 6, 8]]
    calls = {
        'side_effects': lambda **kw: model.side_effects(pairs, k=5, exclude='train', **kw),
        'regimen_side_effects': lambda **kw: model.regimen_side_effects(regs, k=4, **kw),
        'add_on_risk': lambda **kw: model.add_on_risk(regs, [9, 10, 11], k=2, **kw),
        'combination_risk': lambda **kw: model.combination_risk([[1, 2], [3, -1]], fixed=[0], k=2, **kw),
        'drug_profile': lambda **kw: model.drug_profile([0, 5], k=3, **kw),
        'screen': lambda **kw: model.screen(k=4, relations=[0, 1], **kw),
    }
    for name, call in calls.items():
        a, b = call(), call(calibration=None)
        assert type(a) is type(b), name
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), name
        c = call(calibration=cal)                                        # and every query takes a calibration
        assert type(c) is type(a) and all(x.shape == y.shape for x, y in zip(a, c)), name
    with pytest.raises(ValueError, match='calibration'):
        model.side_effects(pairs, calibration=(cal.z, cal.decoder))
