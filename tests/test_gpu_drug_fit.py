"""-m gpu: the new-drug fit (include/tipk.h section 4q, tip_amd/csrc/tipk_drug_fit.hip) against the fp64 spec and the acceptance
rules of tests/drug_fit_spec.py.  The statistics and the fit are tested through the C entries themselves, with outputs
pre-filled with a sentinel; then `ops.distmult_drug_fit` and `TIP.fit_new_drugs` on the small pickle."""
import os

import pytest
import torch

import drug_fit_cases as cases
from conftest import GOLDEN
from drug_fit_spec import C_DFIT, U, bound_of, check_fit, check_stats, spec_stats
from tip_amd import _lib, ops
from tip_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0
LOG2 = 0.6931472


def _chain(n, dim, n_rel, m):
    return _lib.lib().tipk_distmult_drug_fit_max_chain(n, dim, n_rel, max(m, 1))


def _lists_on_device(fl):
    return [t.to(DEV).contiguous() for t in (fl.dense_w, fl.ptr, fl.v, fl.r, fl.wpos, fl.wneg)]


def _workspace(n, dim, n_rel, m):
    nbytes = _lib.lib().tipk_distmult_drug_fit_workspace_bytes(n, dim, n_rel, m)
    assert nbytes >= 0
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)


def _raw_stats(z, rel_w, x, fl, prior=None, l2=1e-4, active=None, out=None, spare=0):
    """tipk_distmult_drug_fit_stats on device tensors; the outputs are pre-filled with a sentinel (`spare` more rows than
    drugs, to see that nothing is written behind the last drug)."""
    n, dim = z.shape
    n_rel, m = rel_w.shape[0], fl.dense_w.numel()
    lists = _lists_on_device(fl)
    if out is None:
        out = (torch.full((m + spare,), SENTINEL, device=DEV), torch.full((m + spare, dim), SENTINEL, device=DEV),
               torch.full((m + spare, dim, dim), SENTINEL, device=DEV))
    ws = _workspace(n, dim, n_rel, m)
    act = None if active is None else active.to(DEV, torch.int32).contiguous()
    st = _lib.lib().tipk_distmult_drug_fit_stats(ptr(z), n, dim, ptr(rel_w), n_rel, ptr(x), m, ptr(lists[0]), ptr(lists[1]),
                                                 ptr(lists[2]), ptr(lists[3]), ptr(lists[4]), ptr(lists[5]), fl.v.numel(),
                                                 ptr(prior), l2, ptr(act), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws),
                                                 stream_ptr(DEV))
    _lib.check(st, 'drug fit stats')
    torch.cuda.synchronize()
    return out


def _raw_fit(z, rel_w, fl, prior=None, l2=1e-4, init=None, max_iter=16, gtol=1e-5, hess=True):
    """tipk_distmult_drug_fit on device tensors -> (x, loss, grad, info, hess), pre-filled with a sentinel."""
    n, dim = z.shape
    n_rel, m = rel_w.shape[0], fl.dense_w.numel()
    lists = _lists_on_device(fl)
    x, loss, grad = (torch.full(s, SENTINEL, device=DEV) for s in ((m, dim), (m,), (m, dim)))
    info = torch.full((m, 4), -7, dtype=torch.int32, device=DEV)
    h = torch.full((m, dim, dim), SENTINEL, device=DEV) if hess else None
    ws = _workspace(n, dim, n_rel, m)
    st = _lib.lib().tipk_distmult_drug_fit(ptr(z), n, dim, ptr(rel_w), n_rel, m, ptr(lists[0]), ptr(lists[1]), ptr(lists[2]),
                                           ptr(lists[3]), ptr(lists[4]), ptr(lists[5]), fl.v.numel(), ptr(prior), l2, ptr(init),
                                           max_iter, gtol, ptr(x), ptr(loss), ptr(grad), ptr(info), ptr(h), ptr(ws),
                                           stream_ptr(DEV))
    _lib.check(st, 'drug fit')
    torch.cuda.synchronize()
    return x, loss, grad, info, h


def _bits(ts):
    return [t.contiguous().view(torch.int32).clone() for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _operands(n, n_rel, dim, m, kind, seed, with_prior=False):
    z = cases.embeddings(n, dim, 300 + seed, 2.0).to(DEV)
    rel_w = cases.relations(n_rel, dim, 350 + seed).to(DEV)
    x = cases.trial_rows(m, dim, kind, 400 + seed).to(DEV)
    prior = cases.trial_rows(m, dim, 'random', 450 + seed).to(DEV) if with_prior else None
    return z, rel_w, x, prior


def _stats_case(n, n_rel, dim, lists, kind, l2=1e-4, rho=1.0, seed=0, with_prior=False, what=''):
    z, rel_w, x, prior = _operands(n, n_rel, dim, len(lists), kind, seed, with_prior)
    fl = ops.drug_fit_csr(lists, n, n_rel, rho)
    got = _raw_stats(z, rel_w, x, fl, prior, l2)
    t = check_stats(z, rel_w, x, lists, prior, l2, rho, got, _chain(n, dim, n_rel, len(lists)), what=what)
    return z, rel_w, x, prior, fl, got, t


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('shape', [(1, 1), (1, 65), (65, 1), (63, 64), (64, 63), (65, 65), (129, 130)], ids=lambda s: '%dx%d' % s)
def test_stats_tile_edges(shape):
    """Tile edges in both directions of the rectangular tiling; every list kind as its own drug, three kinds of rows."""
    n, n_rel = shape
    kinds = cases.list_kinds(n, n_rel, n + n_rel)
    lists = [kinds[k] for k in ('empty', 'one', 'every', 'long')]
    for kind in ('zero', 'random', 'large'):
        z, rel_w, x, prior, fl, got, t = _stats_case(n, n_rel, 16, lists, kind, seed=n + n_rel, what='%dx%d %s' % (n, n_rel, kind))
        assert bool(torch.isfinite(got[0]).all())
        if kind == 'zero':                                               # softplus(0) = log 2 on both classes
            want = torch.tensor([(len(l) > 0) + (float(fl.dense_w[i]) > 0) for i, l in enumerate(lists)], device=DEV) * LOG2
            torch.testing.assert_close(got[0], want.float(), rtol=1e-5, atol=0)


@pytest.mark.parametrize('dim', [4, 12, 16, 20, 32])
def test_stats_widths(dim):
    n = n_rel = 65
    kinds = cases.list_kinds(n, n_rel, dim)
    for kind in ('random', 'large'):
        _stats_case(n, n_rel, dim, [kinds['long'], kinds['one'], kinds['empty']], kind, l2=1e-2, rho=2.0, seed=dim,
                    with_prior=True, what='dim%d %s' % (dim, kind))


@pytest.mark.parametrize('m', [1, 4, 5, 9])
def test_stats_drug_blocks(m):
    """A block of 4 drugs that straddles M writes nothing behind row M - 1; two calls give equal bits; a drug's bits do not
    depend on its neighbours or its slot in the block."""
    n = n_rel = 65
    lists = [cases.random_cells(n, n_rel, 1 + 7 * i, 50 + i) for i in range(m)]
    z, rel_w, x, prior = _operands(n, n_rel, 16, m, 'random', m, with_prior=True)
    fl = ops.drug_fit_csr(lists, n, n_rel)
    got = _raw_stats(z, rel_w, x, fl, prior, spare=5)
    for v in got:
        assert bool((v[m:] == SENTINEL).all())
    got = tuple(v[:m] for v in got)
    check_stats(z, rel_w, x, lists, prior, 1e-4, 1.0, got, _chain(n, 16, n_rel, m), what='m%d' % m)
    assert _same_bits(got, _raw_stats(z, rel_w, x, fl, prior))
    slabs = _lib.lib().tipk_distmult_drug_fit_slabs
    assert slabs(n, 16, n_rel, 1) == slabs(n, 16, n_rel, m) == 4         # 4 tiles: one slab per tile whatever M
    alone = _raw_stats(z, rel_w, x[m - 1:].contiguous(), ops.drug_fit_csr(lists[m - 1:], n, n_rel), prior[m - 1:].contiguous())
    for name, a, b in zip(('loss', 'grad', 'hess'), _bits(alone), _bits(got)):
        assert torch.equal(a, b[m - 1:]), name


def test_stats_slabs():
    """More tiles than slabs (1 024 drugs: 256 blocks, 3 slabs of 3 of the 9 tiles) and fewer tiles than the slab target (one
    drug: a slab per tile); _max_chain bounds what the partial layout implies."""
    L = _lib.lib()
    n, n_rel, dim, m = 129, 130, 16, 1024
    assert L.tipk_distmult_drug_fit_slabs(n, dim, n_rel, m) == 3 and L.tipk_distmult_drug_fit_slabs(n, dim, n_rel, 1) == 9
    for mm in (1, m):
        slabs = L.tipk_distmult_drug_fit_slabs(n, dim, n_rel, mm)
        tps = -(-9 // slabs)
        assert _chain(n, dim, n_rel, mm) >= 16 * 64 * tps + 6 + 4 * slabs + 2
    z, rel_w, x, prior = _operands(n, n_rel, dim, m, 'random', 5)
    pick = [0, 1, 514, m - 1]
    lists = [[] for _ in range(m)]
    for i in pick:
        lists[i] = cases.random_cells(n, n_rel, 40 + i % 7, 60 + i)
    got = _raw_stats(z, rel_w, x, ops.drug_fit_csr(lists, n, n_rel))
    sub = tuple(v[pick] for v in got)
    check_stats(z, rel_w, x[pick], [lists[i] for i in pick], None, 1e-4, 1.0, sub, _chain(n, dim, n_rel, m), what='3 slabs')
    assert bool(torch.isfinite(got[2]).all())
    one = _raw_stats(z, rel_w, x[:1].contiguous(), ops.drug_fit_csr(lists[:1], n, n_rel))
    check_stats(z, rel_w, x[:1], lists[:1], None, 1e-4, 1.0, one, _chain(n, dim, n_rel, 1), what='9 slabs')


def test_stats_active_mask_leaves_rows_untouched():
    n, n_rel, m = 65, 65, 9
    lists = [cases.random_cells(n, n_rel, 5 + i, 70 + i) for i in range(m)]
    z, rel_w, x, prior, fl, full, t = _stats_case(n, n_rel, 16, lists, 'random', seed=3, what='mask')
    active = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0, 0])                   # drugs 4..7 and drug 8: two whole blocks are inactive
    got = _raw_stats(z, rel_w, x, fl, active=active)
    on = active.bool().to(DEV)
    for v, ref in zip(got, full):
        assert bool((v[~on] == SENTINEL).all())                          # bit-untouched
        assert torch.equal(v[on].view(torch.int32), ref[on].view(torch.int32))
    mixed = torch.tensor([0, 1, 0, 0, 0, 0, 1, 0, 1])                    # blocks with active and inactive drugs side by side
    got = _raw_stats(z, rel_w, x, fl, active=mixed)
    on = mixed.bool().to(DEV)
    for v, ref in zip(got, full):
        assert bool((v[~on] == SENTINEL).all())
        assert torch.equal(v[on].view(torch.int32), ref[on].view(torch.int32))


def test_stats_nan_and_inf():
    n, n_rel, m = 65, 65, 5
    lists = [cases.random_cells(n, n_rel, 5 + i, 80 + i) for i in range(m - 1)] + [cases.list_kinds(n, n_rel, 1)['every']]
    z, rel_w, x, prior = _operands(n, n_rel, 16, m, 'random', 9)
    fl = ops.drug_fit_csr(lists, n, n_rel)
    assert float(fl.dense_w[4]) == 0.0                                   # the last drug recorded every cell
    chain = _chain(n, 16, n_rel, m)
    xn = x.clone()
    xn[2, 5] = float('nan')                                              # a NaN in one trial row: that drug alone
    got = _raw_stats(z, rel_w, xn, fl)
    check_stats(z, rel_w, xn, lists, None, 1e-4, 1.0, got, chain, what='nan row of x')
    for v in got:
        assert bool(torch.isnan(v[2]).all()) and bool(torch.isfinite(v[[0, 1, 3, 4]]).all())
    for what, zz, ww in (('z', z.clone(), rel_w), ('rel_w', z, rel_w.clone())):
        (zz if what == 'z' else ww)[64, 3] = float('nan')                # a NaN row of z or rel_w: every drug streams it
        got = _raw_stats(zz, ww, x, fl)
        check_stats(zz, ww, x, lists, None, 1e-4, 1.0, got, chain, what='nan row of ' + what)
        assert all(bool(torch.isnan(v).all()) for v in got), what
    # +-inf products (section 4q): z[7, 2] = inf makes the logits of partner 7 +-inf for every drug (x[:, 2] != 0, column 2 of
    # rel_w has no zero and both signs).  For the drugs with dense_w > 0 nothing finite is invented: the loss is non-finite,
    # and so are grad[2] and row 2 and column 2 of hess, where sigma' = 0 meets the infinite feature; every other entry is
    # finite.
    zi = z.clone()
    zi[7, 2] = float('inf')
    assert bool((x[:, 2] != 0).all()) and bool((rel_w[:, 2] != 0).all()) and bool((rel_w[:, 2] > 0).any()) \
        and bool((rel_w[:, 2] < 0).any())
    got = _raw_stats(zi, rel_w, x, fl)
    hit_g = torch.zeros((4, 16), dtype=torch.bool, device=DEV)
    hit_g[:, 2] = True
    hit_h = torch.zeros((4, 16, 16), dtype=torch.bool, device=DEV)
    hit_h[:, 2, :] = True
    hit_h[:, :, 2] = True
    assert not bool(torch.isfinite(got[0][:4]).any())
    assert torch.equal(~torch.isfinite(got[1][:4]), hit_g) and torch.equal(~torch.isfinite(got[2][:4]), hit_h)


def test_stats_prior_moves_loss_and_gradient_only():
    n, n_rel, dim, m, l2 = 65, 65, 16, 3, 0.25
    lists = [cases.random_cells(n, n_rel, 9 + i, 90 + i) for i in range(m)]
    z, rel_w, x, prior = _operands(n, n_rel, dim, m, 'random', 11, with_prior=True)
    fl = ops.drug_fit_csr(lists, n, n_rel)
    with_c, without = _raw_stats(z, rel_w, x, fl, prior, l2), _raw_stats(z, rel_w, x, fl, None, l2)
    zero_c = _raw_stats(z, rel_w, x, fl, torch.zeros_like(prior), l2)
    assert _same_bits(zero_c, without)                                   # NULL means zeros
    assert torch.equal(with_c[2].view(torch.int32), without[2].view(torch.int32))    # the Hessian does not know the centre
    assert not torch.equal(with_c[0], without[0]) and not bool((with_c[1] == without[1]).any())
    d = (x - prior).double()
    tol = 8 * U * (with_c[1].abs() + without[1].abs() + l2 * (d.abs() + x.abs().double()))
    assert bool(((with_c[1].double() - without[1].double() + l2 * prior.double()).abs() <= tol).all())
    # l2 itself: the stated diagonal and nothing else
    no_l2 = _raw_stats(z, rel_w, x, fl, prior, 0.0)
    eye = torch.eye(dim, dtype=torch.bool, device=DEV).expand(m, dim, dim)
    assert torch.equal(with_c[2][~eye].view(torch.int32), no_l2[2][~eye].view(torch.int32))
    assert torch.equal(with_c[2][eye], no_l2[2][eye] + torch.tensor(l2, device=DEV))


# ------------------------------------------------------------------ the fit
CASES = cases.convergence_cases()


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_fit_convergence_cases(case):
    name, z, rel_w, lists, prior, init, l2 = case
    z, rel_w, prior, init = z.to(DEV), rel_w.to(DEV), _dev(prior), _dev(init)
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]
    fl = ops.drug_fit_csr(lists, n, n_rel)
    x, loss, grad, info, hess = _raw_fit(z, rel_w, fl, prior, l2, init)
    print(name, 'info', info.tolist(), 'loss', loss.tolist())
    chain = _chain(n, dim, n_rel, 1)
    res = check_fit(z, rel_w, lists, prior, l2, 1.0, init, 16, 1e-5, (x, info), chain, what=name)
    assert info[:, 0].tolist() == [1], info.tolist()                     # the condition of the host test leaves a factor 2
    # the returned statistics are those of the returned row, and out_hess is a statistics call at out_x, bit for bit
    check_stats(z, rel_w, x, lists, prior, l2, 1.0, (loss, grad, hess), chain, what=name + ' returned', spec=res['at_x'])
    again = _raw_stats(z, rel_w, x, fl, prior, l2)
    assert _same_bits(again, (loss, grad, hess))
    # `ops.distmult_drug_fit` is the same call
    assert _same_bits(ops.distmult_drug_fit(z, rel_w, fl, prior, l2, init)[:3], (x, loss, grad))


def test_fit_batch_leaves_early_finishers_alone():
    """The cases that share (n, R, dim, l2) -- and two drugs that finish earlier -- as ONE call: the active mask leaves every
    drug bit-identical to its single-drug run (2 tiles: one slab per tile whatever M)."""
    group = [c for c in CASES if c[0] in ('n65_r8_d16_p40', 'n65_r8_d16_p3', 'n65_r8_d16_p1')]
    z, rel_w = group[0][1].to(DEV), group[0][2].to(DEV)
    assert all(torch.equal(c[1], group[0][1]) and torch.equal(c[2], group[0][2]) for c in group)
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]
    lists = [c[3][0] for c in group] + [cases.random_cells(n, n_rel, 30, 77), []]
    both = _raw_fit(z, rel_w, ops.drug_fit_csr(lists, n, n_rel))
    print('batch info', both[3].tolist())
    assert both[3][:, 0].tolist() == [1] * 5 and len(set(both[3][:, 1].tolist())) > 1       # they finish at different times
    check_fit(z, rel_w, lists, None, 1e-4, 1.0, None, 16, 1e-5, (both[0], both[3]), _chain(n, dim, n_rel, 5), what='batch')
    for i, lst in enumerate(lists):
        alone = _raw_fit(z, rel_w, ops.drug_fit_csr([lst], n, n_rel))
        assert torch.equal(alone[3], both[3][i:i + 1]), i
        assert _same_bits([a[0] for a in alone[:3]] + [alone[4][0]], [b[i] for b in both[:3]] + [both[4][i]]), i
    assert _same_bits(both, _raw_fit(z, rel_w, ops.drug_fit_csr(lists, n, n_rel)))           # and call to call


def test_fit_start_and_max_iter_zero():
    """max_iter = 0 evaluates the start only; the start is init, else the prior, else zeros."""
    name, z, rel_w, lists, _, _, l2 = CASES[3]
    z, rel_w = z.to(DEV), rel_w.to(DEV)
    fl = ops.drug_fit_csr(lists, z.shape[0], rel_w.shape[0])
    prior = cases.trial_rows(1, 16, 'random', 78).to(DEV)
    init = cases.trial_rows(1, 16, 'random', 79).to(DEV)
    for c, start, want in ((None, None, torch.zeros_like(prior)), (prior, None, prior), (prior, init, init), (None, init, init)):
        x, loss, grad, info, hess = _raw_fit(z, rel_w, fl, c, l2, start, max_iter=0)
        assert torch.equal(x, want) and info.tolist() == [[0, 1, 0, 0]]
        assert _same_bits(_raw_stats(z, rel_w, want, fl, c, l2), (loss, grad, hess))
    # a start that already satisfies gtol: status 1 at the first evaluation
    x, loss, grad, info, hess = _raw_fit(z, rel_w, fl, None, l2, init, max_iter=0, gtol=1e3)
    assert info.tolist() == [[1, 1, 0, 0]] and torch.equal(x, init)
    # init != prior moves away from init towards the data and the centre; no Hessian asked for: none written
    x, loss, grad, info, hess = _raw_fit(z, rel_w, fl, prior, 1e-2, init, hess=False)
    assert hess is None and info[:, 0].tolist() == [1]
    check_fit(z, rel_w, lists, prior, 1e-2, 1.0, init, 16, 1e-5, (x, info), _chain(z.shape[0], 16, rel_w.shape[0], 1), what='init')


def test_fit_m_zero_launches_nothing():
    L = _lib.lib()
    z, rel_w = cases.embeddings(5, 16, 1).to(DEV), cases.relations(3, 16, 2).to(DEV)
    assert L.tipk_distmult_drug_fit_stats(ptr(z), 5, 16, ptr(rel_w), 3, None, 0, None, None, None, None, None, None, 0, None,
                                          1e-4, None, None, None, None, None, stream_ptr(DEV)) == 0
    assert L.tipk_distmult_drug_fit(ptr(z), 5, 16, ptr(rel_w), 3, 0, None, None, None, None, None, None, 0, None, 1e-4, None, 3,
                                    1e-5, None, None, None, None, None, None, stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    x, loss, grad, info, hess = ops.distmult_drug_fit(z, rel_w, ops.drug_fit_csr([], 5, 3))
    assert x.shape == (0, 16) and loss.shape == (0,) and info.shape == (0, 4) and hess.shape == (0, 16, 16)


def test_fit_captured_and_replayed():
    name, z, rel_w, _, _, _, l2 = CASES[3]
    z, rel_w = z.to(DEV), rel_w.to(DEV)
    n, n_rel = z.shape[0], rel_w.shape[0]
    lists = [cases.planted_cells(z.cpu(), rel_w.cpu(), 30 + 10 * i, 700 + i) for i in range(5)]
    fl = ops.drug_fit_csr(lists, n, n_rel)
    fl = fl._replace(**{k: getattr(fl, k).to(DEV) for k in ('ptr', 'v', 'r', 'wpos', 'wneg', 'dense_w')})   # no copy inside
    a = ops.distmult_drug_fit(z, rel_w, fl)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # the single entry alone: sequential launches
        c = ops.distmult_drug_fit(z, rel_w, fl)
    for v in c:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(a, c), 'captured and replayed'
    assert a[3][:, 0].tolist() == [1] * 5


# ------------------------------------------------------------------ TIP.fit_new_drugs on the small pickle
_MODELS = {}


def _model():
    from tip_amd.layers import TIP, Setting
    if 'cat' not in _MODELS:
        torch.manual_seed(0)
        st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
        _MODELS['cat'] = TIP(st, torch.device(DEV), mod='cat', data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
    return _MODELS['cat']


def _planted_for(model, count, seed):
    z, w = model.embeddings.detach().cpu(), model.decoder.weight.detach().cpu()
    return cases.planted_cells(z, w, count, seed)


def test_tip_fit_new_drugs():
    from tip_amd.layers import FittedDrugs
    model = _model()
    d = model.data
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    inter = [_planted_for(model, 40, 5), [(3, 0), (4, 1), (4, 1)], []]
    fit = model.fit_new_drugs(inter)
    assert isinstance(fit, FittedDrugs) and fit.z.shape == (3, 16) and fit.hess.shape == (3, 16, 16)
    assert fit.loss.shape == fit.grad_norm.shape == (3,) and fit.n_interactions.tolist() == [40, 3, 0]
    assert fit.status.dtype == fit.evaluations.dtype == torch.int64 and fit.status.tolist() == [1, 1, 1], fit.status.tolist()
    chain = _chain(d.n_drug, 16, d.n_dd_et, 3)
    info = torch.stack([fit.status, fit.evaluations, fit.evaluations - 1, torch.zeros_like(fit.status)], 1)
    res = check_fit(z, w, inter, None, 1e-4, 1.0, None, 16, 1e-5, (fit.z, info), chain, what='tip')
    assert not fit.z.requires_grad and model.decoder.weight.requires_grad    # the model is frozen, not changed
    # recovery: the fitted row scores the cells it was given above the start (an inequality, not a tolerance)
    v, r = (torch.tensor(c, device=DEV) for c in zip(*inter[0]))
    logit_of = lambda row: float(((z[v] * w[r]).double() @ row.double()).mean())
    assert logit_of(fit.z[0]) > logit_of(torch.zeros(16, device=DEV))
    # the result goes wherever a NewDrugs goes: new drug i is node n_drug + i of the decoder's queries
    z_ext = torch.cat([model.embeddings.detach(), fit.z])
    pairs = torch.tensor([[d.n_drug, d.n_drug + 1, 0], [3, d.n_drug + 2, d.n_drug]], device=DEV)
    logits, rel = model.decoder.top_relations(z_ext, pairs, 5)           # what `side_effects` asks of the decoder
    assert logits.shape == (3, 5) and bool(torch.isfinite(logits).all())
    score = model.decoder(z_ext, pairs, torch.zeros(3, dtype=torch.int64, device=DEV))
    assert score.shape == (3,) and bool(torch.isfinite(score).all())
    prof = model.drug_profile([d.n_drug, 2, d.n_drug + 2], k=3, new=fit)
    assert prof.expected.shape[0] == 3 and bool(torch.isfinite(prof.expected).all())


def test_tip_fit_from_the_fold_in():
    """The intended call: start from the fold-in row and move it as far as the evidence says."""
    model = _model()
    d = model.data
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    inter = [_planted_for(model, 25, 6), [(3, 0)]]
    new = model.embed_new_drugs([[0, 1], []], inter)
    a, b = model.fit_new_drugs(inter, prior=new, l2=1e-2), model.fit_new_drugs(inter, prior=new.z, l2=1e-2)
    assert _same_bits([a.z, a.loss, a.grad_norm, a.hess], [b.z, b.loss, b.grad_norm, b.hess])
    assert torch.equal(a.status, b.status) and a.status.tolist() == [1, 1]
    chain = _chain(d.n_drug, 16, d.n_dd_et, 2)
    info = torch.stack([a.status, a.evaluations, a.evaluations - 1, torch.zeros_like(a.status)], 1)
    check_fit(z, w, inter, new.z, 1e-2, 1.0, None, 16, 1e-5, (a.z, info), chain, what='fold-in prior')
    c = model.fit_new_drugs(inter, prior=new, init=torch.zeros(2, 16), l2=1e-2)               # init != prior
    assert c.status.tolist() == [1, 1]
    # both ends approximate ONE minimiser: L is l2-strongly convex, so l2 |a - c|_2 <= |g64(a) - g64(c)|_2 (fp64 rounding only)
    ga, gc = (spec_stats(z, w, v.z, inter, new.z, 1e-2, 1.0, bounds=False)['g'] for v in (a, c))
    gap, room = (a.z.double() - c.z.double()).norm(dim=1), (ga - gc).norm(dim=1) / 1e-2
    print('init != prior: |a - c|', gap.tolist(), 'allowed', room.tolist())
    assert bool((gap <= room * (1 + 1e-9) + 1e-15).all())
    # a huge l2 holds the row at the prior.  The data terms are >= 0, so l2/2 |x - c|^2 <= L(x), and rule (b) of check_fit
    # bounds L(x) by the loss at the start c, which has no l2 term: |x - c|_2 <= sqrt(2 (L64(c) + bound_loss) / l2).
    big = 1e6
    h = model.fit_new_drugs(inter, prior=new, l2=big)
    at_c = spec_stats(z, w, new.z, inter, new.z, big, 1.0)
    at_x = spec_stats(z, w, h.z, inter, new.z, big, 1.0)
    acc = (h.evaluations - 1).double()
    start = at_c['loss'] + bound_of(at_c, 'loss', chain, C_DFIT)
    room = start + bound_of(at_x, 'loss', chain, C_DFIT) + 17 * U * acc * start
    dist = (h.z.double() - new.z.double()).norm(dim=1)
    print('huge l2: |x - c|', dist.tolist(), 'allowed', (2 * room / big).sqrt().tolist())
    assert bool((dist <= (2 * room / big).sqrt()).all())
    with pytest.raises(ValueError, match='prior'):
        model.fit_new_drugs(inter[:1], prior=new)
