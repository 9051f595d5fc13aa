"""-m gpu: the side-effect fit (include/tipk.h section 4m, tip_amd/csrc/tipk_side_effect_fit.hip) against the fp64 spec and the
acceptance rules of tests/fit_spec.py.  The statistics and the step are tested through the C entries themselves, each on its
own; then `tipk_distmult_fit` / `ops.distmult_fit` against `check_fit`, and `TIP.fit_side_effects` on the small pickle."""
import os

import pytest
import torch

import fit_cases as cases
from conftest import GOLDEN
from fit_spec import U, bound_of, check_fit, check_stats, newton_direction, spec_stats
from tip_amd import _lib, ops
from tip_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0


def _chain(n, dim, b):
    return _lib.lib().tipk_distmult_fit_max_chain(n, dim, max(b, 1))


def _raw_stats(z, w, fp, l2, active=None, out=None):
    """tipk_distmult_fit_stats on device tensors; the outputs are pre-filled with a sentinel."""
    L = _lib.lib()
    n, dim = z.shape
    b = fp.dense_w.numel()
    lists = [t.to(DEV).contiguous() for t in (fp.dense_w, fp.ptr, fp.u, fp.v, fp.wpos, fp.wneg)]
    if out is None:
        out = (torch.full((b,), SENTINEL, device=DEV), torch.full((b, dim), SENTINEL, device=DEV),
               torch.full((b, dim, dim), SENTINEL, device=DEV))
    nbytes = L.tipk_distmult_fit_workspace_bytes(n, dim, b)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    act = None if active is None else active.to(DEV, torch.int32).contiguous()
    st = L.tipk_distmult_fit_stats(ptr(z), n, dim, ptr(w), b, ptr(lists[0]), ptr(lists[1]), ptr(lists[2]), ptr(lists[3]),
                                   ptr(lists[4]), ptr(lists[5]), fp.u.numel(), l2, ptr(act), ptr(out[0]), ptr(out[1]),
                                   ptr(out[2]), ptr(ws), stream_ptr(DEV))
    _lib.check(st, 'fit stats')
    torch.cuda.synchronize()
    return out


def _bits(ts):
    return [t.contiguous().view(torch.int32).clone() for t in ts]


def _stats_case(n, dim, lists, kind, l2=1e-4, rho=1.0, seed=0, what=''):
    z = cases.embeddings(n, dim, 300 + seed, 2.0).to(DEV)
    w = cases.trial_rows(len(lists), dim, kind, 400 + seed).to(DEV)
    fp = ops.fit_pairs_csr(lists, n, rho)
    got = _raw_stats(z, w, fp, l2)
    t = check_stats(z, w, lists, l2, rho, got, _chain(n, dim, len(lists)), what=what)
    return z, w, fp, got, t


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 129])
def test_stats_tile_edges(n):
    """Tile edges, the masked diagonal tile, a second tile row; every list kind as its own relation, three kinds of rows."""
    kinds = cases.list_kinds(n, n)
    lists = [kinds[k] for k in ('empty', 'one', 'selfs', 'every', 'long')]
    for kind in ('zero', 'random', 'large'):
        z, w, fp, got, t = _stats_case(n, 16, lists, kind, seed=n, what='n%d %s' % (n, kind))
        assert bool(torch.isfinite(got[0]).all())
        if kind == 'zero':                                               # softplus(0) = log 2 on both classes
            want = torch.tensor([(len(l) > 0) + (float(fp.dense_w[i]) > 0) for i, l in enumerate(lists)], device=DEV) * 0.6931472
            torch.testing.assert_close(got[0], want.float(), rtol=1e-5, atol=0)


@pytest.mark.parametrize('dim', [4, 12, 16, 20, 32])
def test_stats_widths(dim):
    n = 65
    kinds = cases.list_kinds(n, dim)
    for kind in ('random', 'large'):
        _stats_case(n, dim, [kinds['long'], kinds['one'], kinds['selfs']], kind, l2=1e-2, rho=2.0, seed=dim,
                    what='dim%d %s' % (dim, kind))


@pytest.mark.parametrize('b', [1, 3, 4, 5, 9, 33])
def test_stats_relation_blocks(b):
    n = 65
    lists = [cases.random_pairs(n, 1 + 7 * i, 50 + i, selfs=True) for i in range(b)]
    z, w, fp, got, t = _stats_case(n, 16, lists, 'random', seed=b, what='b%d' % b)
    again = _raw_stats(z, w, fp, 1e-4)
    assert all(torch.equal(x, y) for x, y in zip(_bits(got), _bits(again)))           # two calls: equal bits
    # every relation on its own gives the bits it has in the block (loss, gradient and Hessian): with the same slab count
    # (3 tiles at n = 65: one slab per tile whatever n_fit) a relation's sums do not depend on its neighbours or its slot
    assert _lib.lib().tipk_distmult_fit_slabs(n, 16, 1) == _lib.lib().tipk_distmult_fit_slabs(n, 16, b) == 3
    alone = _raw_stats(z, w[b - 1:b].contiguous(), ops.fit_pairs_csr(lists[b - 1:], n), 1e-4)
    for name, x, y in zip(('loss', 'grad', 'hess'), _bits(alone), _bits(got)):
        assert torch.equal(x, y[b - 1:]), name


@pytest.mark.parametrize('n, tiles, slabs', [(129, 6, 3), (193, 10, 4)])
def test_stats_slabs(n, tiles, slabs):
    """More tiles than slabs (1 024 relations: 256 blocks; slabs of 2 of the 6 tiles at n = 129, of 3, 3, 3, 1 of the 10 tiles
    at n = 193, so a slab starts in the middle of a tile row and runs into the next one) and fewer tiles than the slab target
    (one relation: a slab per tile, 24 and 40 partials for the finish to add: whole batches and a tail); _max_chain bounds
    what the partial layout implies."""
    L = _lib.lib()
    dim, b = 16, 1024
    assert L.tipk_distmult_fit_slabs(n, dim, b) == slabs and L.tipk_distmult_fit_slabs(n, dim, 1) == tiles
    for bb in (1, b):
        s = L.tipk_distmult_fit_slabs(n, dim, bb)
        tps = -(-tiles // s)
        assert _chain(n, dim, bb) >= 16 * 64 * tps + 6 + 4 * s + 2
    z = cases.embeddings(n, dim, 305, 2.0).to(DEV)
    w = cases.trial_rows(b, dim, 'random', 405).to(DEV)
    pick = [0, 1, 514, b - 1]
    lists = [[] for _ in range(b)]
    for i in pick:
        lists[i] = cases.random_pairs(n, 40 + i % 7, 60 + i, selfs=True)
    got = _raw_stats(z, w, ops.fit_pairs_csr(lists, n), 1e-4)
    sub = tuple(v[pick] for v in got)
    check_stats(z, w[pick], [lists[i] for i in pick], 1e-4, 1.0, sub, _chain(n, dim, b), what='%d slabs' % slabs)
    assert all(bool(torch.isfinite(v).all()) for v in got)
    one = _raw_stats(z, w[:1].contiguous(), ops.fit_pairs_csr(lists[:1], n), 1e-4)
    check_stats(z, w[:1], lists[:1], 1e-4, 1.0, one, _chain(n, dim, 1), what='%d slabs' % tiles)


def test_stats_n_fit_zero_launches_nothing():
    L = _lib.lib()
    z = cases.embeddings(5, 16, 1).to(DEV)
    assert L.tipk_distmult_fit_stats(ptr(z), 5, 16, None, 0, None, None, None, None, None, None, 0, 1e-4, None, None, None, None,
                                     None, stream_ptr(DEV)) == 0
    assert L.tipk_distmult_fit(ptr(z), 5, 16, 0, None, None, None, None, None, None, 0, 1e-4, None, 3, 1e-5, None, None, None,
                                None, None, stream_ptr(DEV)) == 0
    assert L.tipk_newton_step(16, 0, None, None, None, 1e-5, None, None, None, None, None, None, None, None, stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    w, loss, grad, info = ops.distmult_fit(z, ops.fit_pairs_csr([], 5))
    assert w.shape == (0, 16) and loss.shape == (0,) and info.shape == (0, 4)


def test_stats_active_mask_leaves_rows_untouched():
    n, b = 65, 9
    lists = [cases.random_pairs(n, 5 + i, 70 + i) for i in range(b)]
    z, w, fp, full, t = _stats_case(n, 16, lists, 'random', seed=3, what='mask')
    active = torch.tensor([1, 0, 0, 0, 0, 1, 0, 1, 0])                   # relations 1..4: one whole block is inactive
    got = _raw_stats(z, w, fp, 1e-4, active=active)
    on = active.bool().to(DEV)
    for x, ref in zip(got, full):
        assert bool((x[~on] == SENTINEL).all())                          # bit-untouched
        assert torch.equal(x[on].view(torch.int32), ref[on].view(torch.int32))


def test_stats_nan_and_inf():
    n, b = 65, 5
    lists = [cases.random_pairs(n, 5 + i, 80 + i) for i in range(b)]
    z = cases.embeddings(n, 16, 9, 2.0).to(DEV)
    w = cases.trial_rows(b, 16, 'random', 10).to(DEV)
    fp = ops.fit_pairs_csr(lists, n)
    chain = _chain(n, 16, b)
    wn = w.clone()
    wn[2, 5] = float('nan')                                              # a NaN in one trial row: that relation alone
    got = _raw_stats(z, wn, fp, 1e-4)
    check_stats(z, wn, lists, 1e-4, 1.0, got, chain, what='nan row of w')
    for x in got:
        assert bool(torch.isnan(x[2]).all()) and bool(torch.isfinite(x[[0, 1, 3, 4]]).all())
    zn = z.clone()
    zn[64, 3] = float('nan')                                             # a NaN row of z: every relation
    got = _raw_stats(zn, w, fp, 1e-4)
    check_stats(zn, w, lists, 1e-4, 1.0, got, chain, what='nan row of z')
    assert all(bool(torch.isnan(x).all()) for x in got)
    # +-inf products (section 4m): z[7, 2] = inf makes the logits of row 7 +-inf in every relation (w[:, 2] != 0, column 2 of
    # z has no zero, both signs occur).  Nothing finite is invented: every loss is non-finite, and so are grad[2] and row 2
    # and column 2 of hess, where sigma' = 0 meets the infinite feature; every other entry is finite (its bound is not: the
    # logit sensitivity of a pair on row 7 is infinite, so the mask is what is held here).
    zi = z.clone()
    zi[7, 2] = float('inf')
    assert bool((w[:, 2] != 0).all()) and bool((z[:, 2] != 0).all()) and bool((z[:, 2] > 0).any()) and bool((z[:, 2] < 0).any())
    got = _raw_stats(zi, w, fp, 1e-4)
    t = check_stats(zi, w, lists, 1e-4, 1.0, got, chain, what='inf in z')
    hit_g = torch.zeros((b, 16), dtype=torch.bool, device=DEV)
    hit_g[:, 2] = True
    hit_h = torch.zeros((b, 16, 16), dtype=torch.bool, device=DEV)
    hit_h[:, 2, :] = True
    hit_h[:, :, 2] = True
    assert not bool(torch.isfinite(got[0]).any()) and not bool(torch.isfinite(t['loss']).any())
    for name, x, hit in (('g', got[1], hit_g), ('H', got[2], hit_h)):
        assert torch.equal(~torch.isfinite(x), hit), name                # the device: non-finite exactly there
        assert torch.equal(~torch.isfinite(t[name]), hit), name          # and so is the definition in fp64
    # the step ends such a relation with status 3 and keeps its row
    s = _step(16, _step_state(16, b, w.clone(), torch.ones(b), torch.ones(b, 16), -torch.ones(b, 16), torch.ones(b),
                              torch.tensor([[0, 2, 1, 0]] * b), w + 1), got[0], got[1], got[2])
    assert s['info'].tolist() == [[3, 3, 1, 1]] * b and torch.equal(s['w'], w)


# ------------------------------------------------------------------ the step, on hand-made statistics
def _step_state(dim, b, w, loss, grad, p, t, info, trial):
    f = lambda x, shape: torch.as_tensor(x, dtype=torch.float32).reshape(shape).to(DEV).contiguous()
    return {'w': f(w, (b, dim)), 'loss': f(loss, (b,)), 'grad': f(grad, (b, dim)), 'p': f(p, (b, dim)), 't': f(t, (b,)),
            'info': torch.as_tensor(info, dtype=torch.int32).reshape(b, 4).to(DEV).contiguous(), 'trial': f(trial, (b, dim)),
            'active': torch.full((b,), 9, dtype=torch.int32, device=DEV)}


def _step(dim, s, sl, sg, sh, gtol=1e-5):
    b = s['loss'].numel()
    f = lambda x, shape: torch.as_tensor(x, dtype=torch.float32).reshape(shape).to(DEV).contiguous()
    sl, sg, sh = f(sl, (b,)), f(sg, (b, dim)), f(sh, (b, dim, dim))
    st = _lib.lib().tipk_newton_step(dim, b, ptr(sl), ptr(sg), ptr(sh), gtol, ptr(s['w']), ptr(s['loss']), ptr(s['grad']),
                                     ptr(s['p']), ptr(s['t']), ptr(s['info']), ptr(s['trial']), ptr(s['active']), stream_ptr(DEV))
    _lib.check(st, 'newton step')
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize('dim', [4, 16, 20, 32])
def test_step_decisions(dim):
    g = torch.Generator().manual_seed(dim)
    a = torch.randn((dim, dim), generator=g, dtype=torch.float64)
    h = a @ a.t() / dim + torch.eye(dim, dtype=torch.float64)            # well conditioned, positive definite
    grad = torch.randn(dim, generator=g, dtype=torch.float64)
    w0 = torch.randn(dim, generator=g, dtype=torch.float64).float()
    zeros = torch.zeros(dim)
    newton = newton_direction(grad.float().double(), h.float().double())[0]

    # first call: the trial is taken as accepted, p = -H^-1 g, t = 1, the next trial is w + p
    s = _step(dim, _step_state(dim, 1, w0, 0.0, zeros, zeros, 1.0, [0, 0, 0, 0], w0), 2.0, grad, h)
    assert s['info'].tolist() == [[0, 1, 0, 0]] and s['active'].tolist() == [1] and s['t'].tolist() == [1.0]
    assert torch.equal(s['w'][0].cpu(), w0) and s['loss'].tolist() == [2.0] and torch.equal(s['grad'][0].cpu(), grad.float())
    tol = 64 * dim * U * float(torch.linalg.cond(h)) * float(newton.abs().max())
    assert float((s['p'][0].double().cpu() - newton).abs().max()) <= tol, (float((s['p'][0].double().cpu() - newton).abs().max()), tol)
    assert torch.equal(s['trial'][0], torch.addcmul(s['w'][0], s['p'][0], torch.ones((), device=DEV)))
    p0, trial0 = s['p'].clone(), s['trial'].clone()
    gp = float(grad.float().double() @ p0[0].double().cpu())
    assert gp < 0

    # reject: a trial loss above the Armijo line halves t; the trial row moves, the accepted row does not
    s = _step(dim, s, 2.0 + 1e-3, zeros, h)
    assert s['info'].tolist() == [[0, 2, 0, 1]] and s['t'].tolist() == [0.5] and s['active'].tolist() == [1]
    assert torch.equal(s['w'][0].cpu(), w0) and s['loss'].tolist() == [2.0] and torch.equal(s['p'], p0)
    assert torch.equal(s['trial'][0], torch.addcmul(s['w'][0], s['p'][0], torch.full((), 0.5, device=DEV)))
    assert not torch.equal(s['trial'], trial0)

    # accept: a trial loss well below the line; state <- trial, new direction from the trial's Hessian, t = 1
    half = s['trial'].clone()
    g2 = grad * 0.25
    s = _step(dim, s, 2.0 + 0.5 * gp * 0.5, g2, 2 * h)
    assert s['info'].tolist() == [[0, 3, 1, 1]] and s['t'].tolist() == [1.0]
    assert torch.equal(s['w'], half) and torch.equal(s['grad'][0].cpu(), g2.float())
    want = newton_direction(g2.float().double(), (2 * h).float().double())[0]
    assert float((s['p'][0].double().cpu() - want).abs().max()) <= tol

    # the 16 ulp of slack: a trial loss one ulp ABOVE the accepted loss is still accepted when the predicted decrease is tiny
    tiny = _step_state(dim, 1, w0, 1.0, grad * 1e-9, -grad * 1e-9, 1.0, [0, 3, 1, 1], w0 + 1)
    s = _step(dim, tiny, 1.0 + 2 * U, grad * 0.5, h, gtol=0.0)
    assert s['info'].tolist() == [[0, 4, 2, 1]]
    tiny = _step_state(dim, 1, w0, 1.0, grad * 1e-9, -grad * 1e-9, 1.0, [0, 3, 1, 1], w0 + 1)
    s = _step(dim, tiny, 1.0 + 64 * U, grad * 0.5, h, gtol=0.0)
    assert s['info'].tolist() == [[0, 4, 1, 2]]

    # convergence: the accepted gradient is within gtol; the relation goes inactive and stays so
    s = _step(dim, _step_state(dim, 1, w0, 0.0, zeros, zeros, 1.0, [0, 0, 0, 0], w0), 2.0, grad * 1e-7, h, gtol=1e-5)
    assert s['info'].tolist() == [[1, 1, 0, 0]] and s['active'].tolist() == [0] and torch.equal(s['trial'][0].cpu(), w0)
    s['active'].fill_(9)
    s = _step(dim, s, 1.0, grad, h)
    assert s['info'].tolist() == [[1, 1, 0, 0]] and s['active'].tolist() == [0] and s['loss'].tolist() == [2.0]

    # step underflow: t falls below 2^-20
    s = _step(dim, _step_state(dim, 1, w0, 2.0, grad, -grad, 2.0 ** -19, [0, 5, 2, 2], w0), 3.0, zeros, h)
    assert s['info'].tolist() == [[0, 6, 2, 3]] and s['t'].tolist() == [2.0 ** -20]
    s = _step(dim, s, 3.0, zeros, h)
    assert s['info'].tolist() == [[2, 7, 2, 4]] and s['active'].tolist() == [0] and torch.equal(s['w'][0].cpu(), w0)

    # a non-finite statistic: the accepted row is kept, status 3
    for bad in ('loss', 'grad', 'hess'):
        sl, sg, sh = float('nan') if bad == 'loss' else 1.0, grad.clone(), h.clone()
        if bad == 'grad':
            sg[dim - 1] = float('inf')
        if bad == 'hess':
            sh[dim - 1, 0] = float('nan')
        s = _step(dim, _step_state(dim, 1, w0, 2.0, grad, -grad, 1.0, [0, 2, 1, 0], w0 + 1), sl, sg, sh)
        assert s['info'].tolist() == [[3, 3, 1, 1]] and s['active'].tolist() == [0], bad
        assert torch.equal(s['w'][0].cpu(), w0) and s['loss'].tolist() == [2.0] and torch.equal(s['grad'][0].cpu(), grad.float())

    # a pivot that is not > 0: the scaled steepest-descent direction
    hbad = h.clone()
    hbad[dim // 2, dim // 2] = -1.0
    s = _step(dim, _step_state(dim, 1, w0, 0.0, zeros, zeros, 1.0, [0, 0, 0, 0], w0), 2.0, grad, hbad)
    want = -grad.float() / hbad.float().diagonal().max()
    assert s['info'].tolist() == [[0, 1, 0, 0]]
    torch.testing.assert_close(s['p'][0].cpu(), want, rtol=4 * U, atol=0)


def test_step_many_relations_are_independent():
    dim, b = 16, 70
    g = torch.Generator().manual_seed(1)
    a = torch.randn((b, dim, dim), generator=g, dtype=torch.float64)
    h = a @ a.transpose(1, 2) / dim + torch.eye(dim, dtype=torch.float64)
    grad = torch.randn((b, dim), generator=g, dtype=torch.float64)
    w0 = torch.randn((b, dim), generator=g).float()
    s = _step(dim, _step_state(dim, b, w0, torch.zeros(b), torch.zeros(b, dim), torch.zeros(b, dim), torch.ones(b),
                               torch.zeros(b, 4), w0), torch.ones(b), grad, h)
    want = -torch.linalg.solve(h.float().double(), grad.float().double())
    assert float((s['p'].double().cpu() - want).abs().max()) <= 64 * dim * U * float(torch.linalg.cond(h).max()) * float(want.abs().max())
    assert s['info'][:, 1].tolist() == [1] * b


# ------------------------------------------------------------------ the fit
def _fit(z, lists, l2=1e-4, rho=1.0, init=None, max_iter=16, gtol=1e-5):
    fp = ops.fit_pairs_csr(lists, z.shape[0], rho)
    w, loss, grad, info = ops.distmult_fit(z, fp, l2, init, max_iter, gtol)
    torch.cuda.synchronize()
    return w, loss, grad, info


@pytest.mark.parametrize('case', cases.convergence_cases(), ids=lambda c: c[0])
def test_fit_convergence_cases(case):
    name, z, lists = case
    z = z.to(DEV)
    w, loss, grad, info = _fit(z, lists)
    print(name, 'info', info.tolist(), 'loss', loss.tolist())
    chain = _chain(z.shape[0], z.shape[1], 1)
    res = check_fit(z, lists, 1e-4, 1.0, None, 16, 1e-5, (w, info), chain, what=name)
    assert info[:, 0].tolist() == [1], info.tolist()                     # the condition of the host test leaves a factor 2
    # the returned statistics are those of the returned row
    check_stats(z, w, lists, 1e-4, 1.0, (loss, grad, res['at_w']['H'].float()), chain, what=name + ' returned', spec=res['at_w'])


def test_fit_warm_start_forces_rejections():
    name, z, lists = cases.convergence_cases()[0]
    z = z.to(DEV)
    init = (50 * cases.trial_rows(1, z.shape[1], 'random', 77)).to(DEV)
    w, loss, grad, info = _fit(z, lists, init=init, max_iter=40)
    print('warm start info', info.tolist())
    check_fit(z, lists, 1e-4, 1.0, init, 40, 1e-5, (w, info), _chain(z.shape[0], z.shape[1], 1), what='warm start')
    assert int(info[0, 3]) > 0, info.tolist()


def test_fit_max_iter_zero_returns_init_with_its_statistics():
    name, z, lists = cases.convergence_cases()[3]
    z = z.to(DEV)
    init = cases.trial_rows(1, z.shape[1], 'random', 78).to(DEV)
    w, loss, grad, info = _fit(z, lists, init=init, max_iter=0)
    assert torch.equal(w, init) and info.tolist() == [[0, 1, 0, 0]]
    fp = ops.fit_pairs_csr(lists, z.shape[0])
    sl, sg, sh = ops.distmult_fit_stats(z, init, fp, 1e-4)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), sl.view(torch.int32)) and torch.equal(grad.view(torch.int32), sg.view(torch.int32))


def test_fit_is_repeatable_and_batches_do_not_mix():
    n, dim = 130, 16
    z = cases.embeddings(n, dim, 21, 1.0).to(DEV)
    lists = [cases.planted_pairs(z.cpu(), 20 + 15 * i, 500 + i) for i in range(6)] + [[]]
    a, b = _fit(z, lists), _fit(z, lists)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    print('batch info', a[3].tolist())
    check_fit(z, lists, 1e-4, 1.0, None, 16, 1e-5, (a[0], a[3]), _chain(n, dim, len(lists)), what='batch')
    assert a[3][:, 0].tolist() == [1] * 7


def test_fit_captured_and_replayed():
    n, dim = 130, 16
    z = cases.embeddings(n, dim, 23, 1.0).to(DEV)
    lists = [cases.planted_pairs(z.cpu(), 30 + 10 * i, 700 + i) for i in range(5)]
    fp = ops.fit_pairs_csr(lists, n)
    fp = fp._replace(**{k: getattr(fp, k).to(DEV) for k in ('ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w')})   # no copy inside
    a = ops.distmult_fit(z, fp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # the single entry alone: sequential launches
        c = ops.distmult_fit(z, fp)
    for x in c:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c)), 'captured and replayed'
    assert a[3][:, 0].tolist() == [1] * 5


def test_fit_biosnap_size():
    n, dim, b = 645, 16, 64
    z = cases.embeddings(n, dim, 22, 1.0).to(DEV)
    feats = cases.pair_features(z.cpu())
    lists = [cases.planted_pairs(z.cpu(), 250 + 20 * i, 600 + i, feats) for i in range(b)]
    w, loss, grad, info = _fit(z, lists)
    assert info[:, 0].tolist() == [1] * b, info.tolist()
    assert bool((info[:, 1] == info[:, 2] + info[:, 3] + 1).all()) and int(info[:, 1].max()) <= 17
    pick = list(range(0, b, 8))                                          # rule (a) of check_fit on every 8th row
    t = spec_stats(z, w[pick], [lists[i] for i in pick], 1e-4, 1.0)
    bg = 1e-5 + bound_of(t, 'g', _chain(n, dim, b))
    assert bool((t['g'].abs() <= bg).all()), float((t['g'].abs() - bg).max())


# ------------------------------------------------------------------ TIP.fit_side_effects on the small pickle
_MODELS = {}


def _model():
    from tip_amd.layers import TIP, Setting
    if 'cat' not in _MODELS:
        torch.manual_seed(0)
        st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
        _MODELS['cat'] = TIP(st, torch.device(DEV), mod='cat', data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'))
    return _MODELS['cat']


def _train_pairs(d, r):
    a, b = d.dd_train_range[r].tolist()
    blk = d.dd_train_idx[:, a:b].cpu()
    return list(zip(blk[0].tolist(), blk[1].tolist()))                   # both directions, as training lists them


def test_tip_refit_is_a_minimiser():
    from tip_amd.layers import NewSideEffects
    model = _model()
    d = model.data
    r = 1
    lists = [_train_pairs(d, r)]
    fit = model.fit_side_effects(lists)
    assert isinstance(fit, NewSideEffects) and fit.weight.shape == (1, 16) and fit.n_pairs.tolist() == [len(lists[0])]
    assert fit.status.dtype == torch.int64 and fit.evaluations.dtype == torch.int64
    z = model.embeddings.detach()
    chain = _chain(z.shape[0], 16, 1)
    old = model.decoder.weight.detach()[r:r + 1]
    at = {k: spec_stats(z, w, lists, 1e-4, 1.0) for k, w in (('fit', fit.weight), ('old', old), ('zero', torch.zeros_like(old)))}
    bl = bound_of(at['fit'], 'loss', chain)[0]
    print('refit: L(fit) %.6f L(trained row) %.6f L(0) %.6f status %s evaluations %s' % (
        float(at['fit']['loss'][0]), float(at['old']['loss'][0]), float(at['zero']['loss'][0]), fit.status.tolist(),
        fit.evaluations.tolist()))
    assert fit.status.tolist() == [1], fit.status.tolist()               # converged: the row stands for the minimiser
    for other in ('old', 'zero'):                                        # exact properties of a minimiser, up to bound_loss
        room = bl + bound_of(at[other], 'loss', chain)[0]                # the fp32 error of the two losses, nothing else
        print('refit vs %s: L(fit) - L(%s) = %.3e, room %.3e' % (other, other, float(at['fit']['loss'][0] - at[other]['loss'][0]),
                                                                  float(room)))
        assert float(at['fit']['loss'][0]) <= float(at[other]['loss'][0] + room), other
    assert fit.grad_norm.shape == (1,) and fit.loss.shape == (1,)
    assert torch.equal(fit.decoder.weight, fit.weight) and not fit.decoder.weight.requires_grad
    assert not any(p is fit.decoder.weight for p in model.parameters())


def test_tip_new_side_effect_is_screened_like_a_trained_one():
    model = _model()
    d = model.data
    z = model.embeddings.detach()
    lists = [_train_pairs(d, 0)[:40], cases.random_pairs(d.n_drug, 25, 5)]
    fit = model.fit_side_effects(lists, max_iter=16)
    k = 10
    logits, u, v = fit.decoder.screen(z, k, known=fit.known)
    assert logits.shape == (2, k)
    for i, lst in enumerate(lists):
        given = {(min(a, b), max(a, b)) for a, b in lst}
        got = {(min(a, b), max(a, b)) for a, b in zip(u[i].tolist(), v[i].tolist())}
        assert len(got) == k and not (got & given), i
        idx = torch.stack([u[i], v[i]]).long()
        want = ops.distmult(z, fit.weight, idx, torch.full((k,), i, dtype=torch.int64, device=DEV), sigmoid=False)
        torch.testing.assert_close(logits[i], want, rtol=1e-5, atol=1e-6)
    total, count, _, _ = fit.decoder.partner_sums(z, torch.arange(4, device=DEV), 0, known=fit.known)
    assert total.shape == (4, 2) and bool(torch.isfinite(total).all())
    ranked = torch.cat([model.decoder.weight.detach(), fit.weight])
    assert ranked.shape == (d.n_dd_et + 2, 16)


def test_tip_fit_with_new_drugs():
    model = _model()
    d = model.data
    new = model.embed_new_drugs([[0, 1], [2]], [[(3, 0)], [(4, 1), (5, 1)]])
    lists = [[(d.n_drug, 3), (d.n_drug + 1, 4), (5, 6)]]
    fit = model.fit_side_effects(lists, new=new)
    n_all = d.n_drug + 2
    assert fit.n_pairs.tolist() == [3] and fit.weight.shape == (1, 16)
    keys = fit.known[0].tolist()
    assert sorted(keys) == sorted([d.n_drug * n_all + 3, 3 * n_all + d.n_drug, (d.n_drug + 1) * n_all + 4,
                                   4 * n_all + d.n_drug + 1, 5 * n_all + 6, 6 * n_all + 5])
    z_ext = torch.cat([model.embeddings.detach(), new.z])
    check_fit(z_ext, lists, 1e-4, 1.0, None, 16, 1e-5, (fit.weight, torch.stack([fit.status, fit.evaluations,
              fit.evaluations - 1, torch.zeros_like(fit.status)], 1)), _chain(n_all, 16, 1), what='new drugs')
    with pytest.raises(ValueError, match='out of range'):
        model.fit_side_effects([[(d.n_drug + 2, 0)]], new=new)
    with pytest.raises(ValueError, match='out of range'):
        model.fit_side_effects([[(d.n_drug, 0)]])
