"""CPU tests of the new-drug fit (include/tipk.h section 4q): the symbols and the shape queries, argument validation of the two
C entries (every refusal happens before anything touches a device, so bogus device pointers are safe here), the Python surface
(`ops.drug_fit_csr`, the refusals of `TIP.fit_new_drugs` at the sizes of the small pickle), the fp64 spec
(tests/drug_fit_spec.py) against a plain loop and autograd, planted mistakes the acceptance rule must reject, and the
convergence condition of the specified cases."""
import ctypes
import math
import os
import pickle
import types

import pytest
import torch

import drug_fit_cases as cases
from conftest import GOLDEN
from drug_fit_spec import C_DFIT, check_stats, spec_fit, spec_stats
from tip_amd import _lib, layers, ops
from tip_amd.layers import TIP, FittedDrugs

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch
SYMBOLS = ('tipk_distmult_drug_fit_supported', 'tipk_distmult_drug_fit_slabs', 'tipk_distmult_drug_fit_max_chain',
           'tipk_distmult_drug_fit_workspace_bytes', 'tipk_distmult_drug_fit_stats', 'tipk_distmult_drug_fit')


def _stats(n=10, dim=16, n_rel=7, n_fit=3, n_rec=5, l2=1e-4, z=FAKE, rel_w=FAKE, x=FAKE, dense=FAKE, rptr=FAKE, rv=FAKE, rr=FAKE,
           wpos=FAKE, wneg=FAKE, prior=None, active=None, loss=FAKE, grad=FAKE, hess=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_drug_fit_stats(z, n, dim, rel_w, n_rel, x, n_fit, dense, rptr, rv, rr, wpos, wneg, n_rec,
                                                   prior, l2, active, loss, grad, hess, ws, None)


def _fit(n=10, dim=16, n_rel=7, n_fit=3, n_rec=5, l2=1e-4, max_iter=4, gtol=1e-5, z=FAKE, rel_w=FAKE, dense=FAKE, rptr=FAKE,
         rv=FAKE, rr=FAKE, wpos=FAKE, wneg=FAKE, prior=None, init=None, x=FAKE, loss=FAKE, grad=FAKE, info=FAKE, hess=None,
         ws=FAKE):
    return _lib.lib().tipk_distmult_drug_fit(z, n, dim, rel_w, n_rel, n_fit, dense, rptr, rv, rr, wpos, wneg, n_rec, prior, l2,
                                             init, max_iter, gtol, x, loss, grad, info, hess, ws, None)


# ------------------------------------------------------------------ symbols and statuses
def test_symbols_and_shape_queries():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30            # purely additive
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    sup, slabs, chain, wsb = (L.tipk_distmult_drug_fit_supported, L.tipk_distmult_drug_fit_slabs,
                              L.tipk_distmult_drug_fit_max_chain, L.tipk_distmult_drug_fit_workspace_bytes)
    top = 2 ** 31 - 1
    for n, n_rel in ((0, 5), (5, 0), (1, 1), (645, 1097), (1, top), (top, 1), (1, top + 1), (top + 1, 1), (46341, 46341),
                     (46340, 46341), (65536, 32768), (65536, 32767), (-1, 5), (2 ** 40, 2 ** 40)):
        for dim in (0, 2, 4, 6, 16, 20, 32, 36):
            for n_fit in (0, 1, 64, 65536, 65537):
                want = n >= 1 and n_rel >= 1 and n * n_rel < 2 ** 31 and dim % 4 == 0 and 4 <= dim <= 32 and 1 <= n_fit <= 65536
                assert sup(n, dim, n_rel, n_fit) == int(want), (n, n_rel, dim, n_fit)
                if not want:
                    assert slabs(n, dim, n_rel, n_fit) == -1 and chain(n, dim, n_rel, n_fit) == -1
                    assert wsb(n, dim, n_rel, n_fit) == (0 if n_fit == 0 and sup(n, dim, n_rel, 1) else -1)
    # BioSNAP: 11 x 18 = 198 rectangular tiles.  One drug: a slab per tile; 64 drugs: 16 blocks, 50 slabs of 4 tiles
    assert slabs(645, 16, 1097, 1) == 198 and slabs(645, 16, 1097, 64) == 50 and slabs(1, 4, 1, 1) == 1
    assert slabs(65, 16, 65, 4) == 4 and slabs(65, 16, 65, 65536) == 1 and slabs(1, 16, top, 1) == 1024
    assert chain(645, 16, 1097, 64) == 4 * 1024 + 6 + 4 * 50 + 2
    assert chain(645, 16, 1097, 1) == max(1024 + 6 + 4 * 198, 256 + math.ceil(645 * 1097 / 256)) + 2
    elems = 1 + 16 + 256
    state = lambda b: sum((v + 255) // 256 * 256 for v in (b * 64, b * 4, b * 64, b * 4, b * 4, b * 64, b * 1024))
    assert wsb(645, 16, 1097, 64) == (16 * 50 * 4 * 4 * elems * 4 + 255) // 256 * 256 + state(64)
    assert wsb(645, 16, 1097, 0) == 0


def test_status_order():
    for call in (_stats, _fit):
        assert call(n=0) == EINVAL and call(n_rel=0) == EINVAL and call(dim=0) == EINVAL and call(n_fit=-1) == EINVAL
        assert call(n_rec=-1) == EINVAL and call(n=-3) == EINVAL
        assert call(l2=-1.0) == EINVAL and call(l2=float('nan')) == EINVAL
        for name in ('z', 'rel_w', 'x', 'dense', 'rptr', 'rv', 'rr', 'wpos', 'wneg', 'loss', 'grad', 'ws'):
            assert call(**{name: None}) == EINVAL, name
        assert call(rv=None, rr=None, wpos=None, wneg=None, n_rec=0, dim=6) == EUNSUPPORTED      # no list: no pointers needed
        assert call(dim=6, z=None) == EINVAL                                # an argument error comes before the range
        assert call(dim=6) == EUNSUPPORTED and call(dim=36) == EUNSUPPORTED and call(n_fit=65537) == EUNSUPPORTED
        assert call(n=46341, n_rel=46341) == EUNSUPPORTED and call(n=2 ** 31, n_rel=1) == EUNSUPPORTED
        assert call(z=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED       # z and rel_w must be 16-byte aligned
        assert call(rel_w=ctypes.c_void_p((1 << 20) + 8)) == EUNSUPPORTED
        assert call(prior=FAKE, dim=6) == EUNSUPPORTED                      # (a prior changes nothing of the order)
        assert call(n_fit=0, z=None, rel_w=None, x=None, dense=None, rptr=None, loss=None, grad=None, ws=None) == 0
    assert _stats(hess=None) == EINVAL
    assert _fit(info=None) == EINVAL
    assert _fit(max_iter=-1) == EINVAL and _fit(gtol=-1.0) == EINVAL and _fit(gtol=float('nan')) == EINVAL
    assert _fit(max_iter=-1, dim=6) == EINVAL and _fit(hess=FAKE, dim=6) == EUNSUPPORTED


# ------------------------------------------------------------------ Python surface
def test_drug_fit_csr():
    n, nr = 5, 4
    fl = ops.drug_fit_csr([[(0, 1), (3, 2), (0, 1), (0, 1), (4, 3)], [], [(4, 0)]], n, nr)
    assert isinstance(fl, ops.DrugFitLists)
    assert fl.ptr.tolist() == [0, 3, 3, 4] and fl.n_interactions.tolist() == [5, 0, 1]
    assert fl.v.tolist() == [0, 3, 4, 4] and fl.r.tolist() == [1, 2, 3, 0] and fl.v.dtype == fl.r.dtype == torch.int32
    assert torch.allclose(fl.wpos, torch.tensor([3 / 5, 1 / 5, 1 / 5, 1.0]))                 # a duplicate adds multiplicity
    assert torch.allclose(fl.dense_w, torch.tensor([1 / 17, 1 / 20, 1 / 19]))                # N_a: DISTINCT cells taken out
    assert torch.allclose(fl.wneg, torch.tensor([1 / 17, 1 / 17, 1 / 17, 1 / 19]))
    keys, kptr = fl.known
    assert kptr.tolist() == [0, 3, 3, 4] and keys.tolist() == [1, 14, 19, 16] and keys.dtype == torch.int64
    # (v, r) is not symmetric: the cell (1, 0) is not the cell (0, 1)
    assert ops.drug_fit_csr([[(1, 0), (0, 1)]], n, nr).ptr.tolist() == [0, 2]
    # the tensor form, and neg_weight
    idx = torch.tensor([[0, 3, 0, 0, 4, 4], [1, 2, 1, 1, 3, 0]])
    fq = ops.drug_fit_csr((idx, torch.tensor([0, 5, 5, 6])), n, nr, neg_weight=2.0)
    assert torch.equal(fq.v, fl.v) and torch.equal(fq.r, fl.r) and torch.equal(fq.ptr, fl.ptr)
    assert torch.allclose(fq.wneg, 2 * fl.wneg) and torch.allclose(fq.dense_w, 2 * fl.dense_w) and torch.equal(fq.wpos, fl.wpos)
    # every cell recorded: N_a = 0
    every = [(v, r) for v in range(3) for r in range(2)]
    fe = ops.drug_fit_csr([every + every[:2]], 3, 2)
    assert fe.dense_w.tolist() == [0.0] and fe.wneg.tolist() == [0.0] * 6 and fe.n_interactions.tolist() == [8]
    assert fe.known[0].tolist() == list(range(6))
    empty = ops.drug_fit_csr([], 3, 2)
    assert empty.ptr.tolist() == [0] and empty.dense_w.numel() == 0
    for bad in ([[(5, 0)]], [[(0, 4)]], [[(-1, 0)]], [[(0, -1)]], [[(0, 1, 2)]], [[3]], 7, (idx, torch.tensor([0, 7])),
                (idx, torch.tensor([1, 6])), (idx.float(), torch.tensor([0, 6]))):
        with pytest.raises(ValueError):
            ops.drug_fit_csr(bad, n, nr)
    with pytest.raises(ValueError):
        ops.drug_fit_csr([[(0, 1)]], n, nr, neg_weight=0.0)
    with pytest.raises(ValueError):
        ops.drug_fit_csr([[(0, 1)]], n, 0)


def test_ops_refuse_cpu_tensors():
    fl = ops.drug_fit_csr([[(0, 1)]], 5, 3)
    assert ops.distmult_drug_fit_supported(5, 4, 3) and not ops.distmult_drug_fit_supported(5, 6, 3)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_drug_fit_stats(torch.ones(5, 4), torch.ones(3, 4), torch.ones(1, 4), fl)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_drug_fit(torch.ones(5, 4), torch.ones(3, 4), fl)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.distmult_drug_fit(torch.ones(5, 4, dtype=torch.float64), torch.ones(3, 4), fl)


def test_tip_fit_new_drugs_refusals():
    assert FittedDrugs._fields == ('z', 'loss', 'grad_norm', 'evaluations', 'status', 'n_interactions', 'hess')
    assert 'FittedDrugs' in layers.__all__
    with open(os.path.join(GOLDEN, 'data_dict_small.pkl'), 'rb') as f:
        dd = pickle.load(f)
    n, nr = int(dd['n_drug']), int(dd['n_dd_et'])                           # the sizes of the small pickle
    data = types.SimpleNamespace(n_drug=n, n_dd_et=nr)
    dec = types.SimpleNamespace(in_dim=16)
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.fit_new_drugs(types.SimpleNamespace(decoder_kind='nn', shard=None, data=data, decoder=dec), [[(0, 1)]], l2=-1)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.fit_new_drugs(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data, decoder=dec), [[(0, 1)]],
                          l2=-1)
    self = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=dec)
    for kw in ({'l2': -1e-3}, {'l2': float('nan')}, {'neg_weight': 0.0}, {'neg_weight': -1.0}, {'max_iter': -1}, {'gtol': -1.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TIP.fit_new_drugs(self, [[(0, 1)]], **kw)
    for bad in ([[(n, 0)]], [[(-1, 0)]], [[(0, nr)]], [[(0, -1)]]):          # partners are EXISTING drugs
        with pytest.raises(ValueError, match='out of range'):
            TIP.fit_new_drugs(self, bad)
    for name in ('prior', 'init'):
        for rows in (torch.zeros(2, 16), torch.zeros(16), torch.zeros(1, 8), types.SimpleNamespace(z=torch.zeros(3, 16))):
            with pytest.raises(ValueError, match=name):
                TIP.fit_new_drugs(self, [[(0, 1)]], **{name: rows})
    wide = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=types.SimpleNamespace(in_dim=40))
    with pytest.raises(NotImplementedError, match='4q'):
        TIP.fit_new_drugs(wide, [[(0, 1)]])


# ------------------------------------------------------------------ the spec
def _loop_stats(z, w, x, c, lst, l2, rho):
    """The definition as a plain Python loop over all cells, in floats."""
    n, n_rel, dim = len(z), len(w), len(x)
    rec = set(lst)
    p_a, n_a = len(lst), n * n_rel - len(rec)
    sp = lambda s: max(s, 0.0) + math.log1p(math.exp(-abs(s)))
    sg = lambda s: 1.0 / (1.0 + math.exp(-s)) if s >= 0 else math.exp(s) / (1.0 + math.exp(s))
    d = [x[k] - c[k] for k in range(dim)]
    loss, g, h = 0.5 * l2 * sum(v * v for v in d), [l2 * v for v in d], [[l2 * (i == j) for j in range(dim)] for i in range(dim)]
    terms = [(v, r, 1.0 / p_a, -1.0) for v, r in lst]
    terms += [(v, r, rho / n_a, 1.0) for v in range(n) for r in range(n_rel) if (v, r) not in rec]
    for v, r, coef, sign in terms:
        f = [z[v][k] * w[r][k] for k in range(dim)]
        s = sign * sum(f[k] * x[k] for k in range(dim))
        loss += coef * sp(s)
        for i in range(dim):
            g[i] += coef * sign * sg(s) * f[i]
            for j in range(dim):
                h[i][j] += coef * sg(s) * sg(-s) * f[i] * f[j]
    return loss, g, h


def test_spec_against_plain_loop():
    n, n_rel, dim = 7, 5, 4
    z, w = cases.embeddings(n, dim, 5, 2.0), cases.relations(n_rel, dim, 6)
    lst = [(0, 1), (0, 1), (1, 0), (2, 2), (6, 4), (6, 4), (6, 4), (3, 0)]
    x = cases.trial_rows(2, dim, 'random', 9) * 3
    c = cases.trial_rows(2, dim, 'random', 10)
    for rho, l2, prior in ((1.0, 1e-4, None), (2.5, 0.3, c), (1.0, 0.0, c)):
        t = spec_stats(z, w, x, [lst, []], prior, l2, rho)
        c0 = [0.0] * dim if prior is None else prior[0].double().tolist()
        loss, g, h = _loop_stats(z.double().tolist(), w.double().tolist(), x[0].double().tolist(), c0, lst, l2, rho)
        assert abs(float(t['loss'][0]) - loss) <= 1e-13 * (1 + abs(loss))
        assert torch.allclose(t['g'][0], torch.tensor(g, dtype=torch.float64), rtol=0, atol=1e-13)
        assert torch.allclose(t['H'][0], torch.tensor(h, dtype=torch.float64), rtol=0, atol=1e-13)
        # an empty list: negatives only, every cell
        s = ((z.double() * x[1].double()) @ w.double().t())
        c1 = torch.zeros(dim, dtype=torch.float64) if prior is None else prior[1].double()
        want = rho / (n * n_rel) * torch.nn.functional.softplus(s).sum() + 0.5 * l2 * ((x[1].double() - c1) ** 2).sum()
        assert abs(float(t['loss'][1] - want)) <= 1e-13
        assert bool((t['A_loss'] >= t['loss'] - 1e-15).all()) and bool((t['T_loss'] > 0).all())
    # every cell recorded: the negative sum is dropped
    every = [(v, r) for v in range(n) for r in range(n_rel)]
    t = spec_stats(z, w, x[:1], [every], None, 0.0, 1.0)
    s = ((z.double() * x[0].double()) @ w.double().t())
    assert abs(float(t['loss'][0] - torch.nn.functional.softplus(-s).mean())) <= 1e-13
    # a NaN logit on any cell: the whole drug, and that drug alone
    xn = x.clone()
    xn[1, 2] = float('nan')
    t = spec_stats(z, w, xn, [lst, []], None, 1e-4, 1.0)
    assert bool(torch.isnan(t['H'][1]).all()) and bool(torch.isnan(t['g'][1]).all()) and bool(torch.isfinite(t['H'][0]).all())


def test_spec_against_autograd():
    n, n_rel, dim = 9, 6, 4
    z, w = cases.embeddings(n, dim, 6, 2.0), cases.relations(n_rel, dim, 7)
    lst = cases.random_cells(n, n_rel, 12, 3) + [(0, 0), (0, 0)]
    x0 = cases.trial_rows(1, dim, 'random', 4)[0].double()
    c = cases.trial_rows(1, dim, 'random', 5)
    loss_of = lambda x: spec_stats(z, w, x[None], [lst], c, 1e-1, 1.5, bounds=False)['loss'][0]
    t = spec_stats(z, w, x0[None], [lst], c, 1e-1, 1.5)
    g = torch.autograd.functional.jacobian(loss_of, x0)
    h = torch.autograd.functional.hessian(loss_of, x0)
    assert torch.allclose(t['g'][0], g, rtol=0, atol=1e-13) and torch.allclose(t['H'][0], h, rtol=0, atol=1e-13)


# ------------------------------------------------------------------ the rule bites
def _decomposed(z, w, x, fl, prior, l2, drop_last_column=False):
    """The device's decomposition -- a dense stream over ALL cells with dense_w, then the sparse correction over the lists of
    a DrugFitLists, then the l2 terms -- evaluated in fp64 and rounded to fp32."""
    z64, w64, x64 = z.double(), w.double(), x.double()
    n, dim = z64.shape
    n_rel = w64.shape[0]
    keep = n_rel - 1 if drop_last_column else n_rel
    f = (z64[:, None, :] * w64[None, :keep, :]).reshape(-1, dim)
    c64 = torch.zeros_like(x64) if prior is None else prior.double()
    loss, grad, hess = [], [], []
    sp = torch.nn.functional.softplus
    for a in range(fl.dense_w.numel()):
        s = f @ x64[a]
        c = fl.dense_w[a].double()
        lo, hi = int(fl.ptr[a]), int(fl.ptr[a + 1])
        fs = z64[fl.v[lo:hi].long()] * w64[fl.r[lo:hi].long()]
        ss = fs @ x64[a]
        wp, wn = fl.wpos[lo:hi].double(), fl.wneg[lo:hi].double()
        d = x64[a] - c64[a]
        loss.append(c * sp(s).sum() + (wp * sp(-ss) - wn * sp(ss)).sum() + 0.5 * l2 * (d * d).sum())
        grad.append(c * torch.sigmoid(s) @ f + (-wp * torch.sigmoid(-ss) - wn * torch.sigmoid(ss)) @ fs + l2 * d)
        hd = torch.sigmoid(s) * torch.sigmoid(-s)
        hs = torch.sigmoid(ss) * torch.sigmoid(-ss)
        hess.append((f * (c * hd)[:, None]).t() @ f + (fs * ((wp - wn) * hs)[:, None]).t() @ fs
                    + l2 * torch.eye(dim, dtype=torch.float64))
    return torch.stack(loss).float(), torch.stack(grad).float(), torch.stack(hess).float()


def test_rule_accepts_the_decomposition_and_rejects_planted_mistakes():
    n, n_rel, dim, l2 = 33, 9, 8, 1e-1
    z, w = cases.embeddings(n, dim, 11, 2.0), cases.relations(n_rel, dim, 12)
    lst = cases.random_cells(n, n_rel, 60, 13)
    lst = lst + lst[:20] + [(4, 4), (4, 4)]
    x = cases.trial_rows(1, dim, 'random', 14) * 2
    prior = cases.trial_rows(1, dim, 'random', 15)
    d_chain = _lib.lib().tipk_distmult_drug_fit_max_chain(n, dim, n_rel, 1)
    fl = ops.drug_fit_csr([lst], n, n_rel)
    assert C_DFIT >= 4.0
    check_stats(z, w, x, [lst], prior, l2, 1.0, _decomposed(z, w, x, fl, prior, l2), d_chain, what='right')   # the right one passes
    distinct = int(fl.ptr[1])
    mistakes = {
        'a recorded cell not taken out of the dense stream': (fl._replace(wneg=torch.zeros_like(fl.wneg)), prior, False),
        'l2 pulling to 0 instead of c': (fl, None, False),
        'a dropped last tile column': (fl, prior, True),
        'N_a without the recorded cells taken out': (fl._replace(
            dense_w=fl.dense_w * (n * n_rel - distinct) / (n * n_rel), wneg=fl.wneg * (n * n_rel - distinct) / (n * n_rel)),
            prior, False),
        'wpos not divided by P_a': (fl._replace(wpos=fl.wpos * float(fl.n_interactions[0])), prior, False),
    }
    for name, (lists, c, drop) in mistakes.items():
        with pytest.raises(AssertionError, match='off fp64'):
            check_stats(z, w, x, [lst], prior, l2, 1.0, _decomposed(z, w, x, lists, c, l2, drop), d_chain, what=name)
    # NaN placement: a NaN that leaks into another drug, and one that is missing
    two = [lst, lst[:7]]
    fl2 = ops.drug_fit_csr(two, n, n_rel)
    x2 = torch.cat([x, x])
    x2[1, 3] = float('nan')
    good = _decomposed(z, w, x2, fl2, None, l2)
    assert bool(torch.isnan(good[0][1])) and not bool(torch.isnan(good[0][0]))
    check_stats(z, w, x2, two, None, l2, 1.0, good, d_chain, what='nan')
    leak = tuple(v.clone() for v in good)
    leak[1][0, 2] = float('nan')
    with pytest.raises(AssertionError, match='without a NaN logit'):
        check_stats(z, w, x2, two, None, l2, 1.0, leak, d_chain)
    miss = tuple(v.clone() for v in good)
    miss[2][1, 0, 0] = 0.0
    with pytest.raises(AssertionError, match='must be all NaN'):
        check_stats(z, w, x2, two, None, l2, 1.0, miss, d_chain)


# ------------------------------------------------------------------ condition, not measurement
@pytest.mark.parametrize('case', cases.convergence_cases(), ids=lambda c: c[0])
def test_convergence_cases_converge_within_8_evaluations(case):
    name, z, rel_w, lists, prior, init, l2 = case
    got = spec_fit(z, rel_w, lists, prior, l2=l2, rho=1.0, init=init, max_iter=16, gtol=1e-5)
    status, evals, acc, rej = got['info'][0].tolist()
    print(name, 'evaluations', evals, 'rejected', rej, 'loss', float(got['loss'][0]))
    assert status == 1 and evals <= 8 and evals == acc + rej + 1, (name, got['info'][0].tolist())
    # and in fp32-sized slack: the 16 ulp of the rule never make the fp64 iteration reject a step here
    assert rej == 0, (name, rej)
