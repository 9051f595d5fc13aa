"""CPU tests of the side-effect fit (include/tipk.h section 4m): the symbols and the shape queries, argument validation of the
three C entries (every refusal happens before anything touches a device, so bogus device pointers are safe here), the Python
surface (`ops.fit_pairs_csr`, the refusals of `TIP.fit_side_effects`), the fp64 spec (tests/fit_spec.py) against a plain loop
and autograd, planted mistakes the acceptance rule must reject, and the convergence condition of the specified cases."""
import ctypes
import math
import types

import pytest
import torch

import fit_cases as cases
from fit_spec import U, check_stats, newton_direction, spec_fit, spec_stats
from tip_amd import _lib, ops
from tip_amd import layers
from tip_amd.layers import TIP, NewSideEffects

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch
SYMBOLS = ('tipk_distmult_fit_supported', 'tipk_distmult_fit_slabs', 'tipk_distmult_fit_max_chain',
           'tipk_distmult_fit_workspace_bytes', 'tipk_distmult_fit_stats', 'tipk_newton_step', 'tipk_distmult_fit')


def _stats(n=10, dim=16, n_fit=3, n_pairs=5, l2=1e-4, z=FAKE, w=FAKE, dense=FAKE, pptr=FAKE, pu=FAKE, pv=FAKE, wpos=FAKE,
           wneg=FAKE, active=None, loss=FAKE, grad=FAKE, hess=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_fit_stats(z, n, dim, w, n_fit, dense, pptr, pu, pv, wpos, wneg, n_pairs, l2, active, loss,
                                              grad, hess, ws, None)


def _step(dim=16, n_fit=3, gtol=1e-5, sl=FAKE, sg=FAKE, sh=FAKE, w=FAKE, loss=FAKE, grad=FAKE, p=FAKE, t=FAKE, info=FAKE,
          trial=FAKE, active=FAKE):
    return _lib.lib().tipk_newton_step(dim, n_fit, sl, sg, sh, gtol, w, loss, grad, p, t, info, trial, active, None)


def _fit(n=10, dim=16, n_fit=3, n_pairs=5, l2=1e-4, max_iter=4, gtol=1e-5, z=FAKE, dense=FAKE, pptr=FAKE, pu=FAKE, pv=FAKE,
         wpos=FAKE, wneg=FAKE, init=None, w=FAKE, loss=FAKE, grad=FAKE, info=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_fit(z, n, dim, n_fit, dense, pptr, pu, pv, wpos, wneg, n_pairs, l2, init, max_iter, gtol, w,
                                        loss, grad, info, ws, None)


# ------------------------------------------------------------------ symbols and statuses
def test_symbols_and_shape_queries():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30            # purely additive
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    sup, slabs, chain, wsb = (L.tipk_distmult_fit_supported, L.tipk_distmult_fit_slabs, L.tipk_distmult_fit_max_chain,
                              L.tipk_distmult_fit_workspace_bytes)
    for n in (0, 1, 645, 46340, 46341):
        for dim in (0, 2, 4, 6, 16, 20, 32, 36):
            for n_fit in (0, 1, 1097, 65536, 65537):
                want = 1 <= n <= 46340 and dim % 4 == 0 and 4 <= dim <= 32 and 1 <= n_fit <= 65536
                assert sup(n, dim, n_fit) == int(want), (n, dim, n_fit)
                if not want:
                    assert slabs(n, dim, n_fit) == -1 and chain(n, dim, n_fit) == -1
                    assert wsb(n, dim, n_fit) == (0 if n_fit == 0 and sup(n, dim, 1) else -1)
    # BioSNAP: 11 tile rows, 66 tiles.  One relation: a slab per tile; 1 097 relations: 275 blocks, 4 slabs of 17 tiles
    assert slabs(645, 16, 1) == 66 and slabs(645, 16, 1097) == 4 and slabs(1, 4, 1) == 1 and slabs(65, 16, 4) == 3
    assert chain(645, 16, 1097) == 17 * 1024 + 6 + 16 + 2
    assert chain(645, 16, 1) == max(1024 + 6 + 4 * 66, 256 + math.ceil(645 * 646 / 2 / 256)) + 2
    elems = 1 + 16 + 256
    state = lambda b: sum((x + 255) // 256 * 256 for x in (b * 64, b * 4, b * 64, b * 4, b * 4, b * 64, b * 1024))
    assert wsb(645, 16, 1097) == (275 * 4 * 4 * 4 * elems * 4 + 255) // 256 * 256 + state(1097)
    assert wsb(645, 16, 0) == 0


def test_status_order():
    for call in (_stats, _fit):
        assert call(n=0) == EINVAL and call(dim=0) == EINVAL and call(n_fit=-1) == EINVAL and call(n_pairs=-1) == EINVAL
        assert call(l2=-1.0) == EINVAL and call(l2=float('nan')) == EINVAL
        for name in ('z', 'dense', 'pptr', 'pu', 'pv', 'wpos', 'wneg', 'loss', 'grad', 'ws'):
            assert call(**{name: None}) == EINVAL, name
        assert call(pu=None, pv=None, wpos=None, wneg=None, n_pairs=0, dim=6) == EUNSUPPORTED     # no list: no pointers needed
        assert call(dim=6, z=None) == EINVAL                                # an argument error comes before the range
        assert call(dim=6) == EUNSUPPORTED and call(dim=36) == EUNSUPPORTED and call(n=46341) == EUNSUPPORTED
        assert call(n_fit=65537) == EUNSUPPORTED
        assert call(z=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED      # z must be 16-byte aligned
        assert call(n_fit=0, z=None, dense=None, pptr=None, loss=None, grad=None, ws=None) == 0   # nothing to do, no launch
    assert _stats(w=None) == EINVAL and _stats(hess=None) == EINVAL
    assert _fit(w=None) == EINVAL and _fit(info=None) == EINVAL
    assert _fit(max_iter=-1) == EINVAL and _fit(gtol=-1.0) == EINVAL and _fit(gtol=float('nan')) == EINVAL
    assert _fit(max_iter=-1, dim=6) == EINVAL
    assert _step(dim=0) == EINVAL and _step(n_fit=-1) == EINVAL and _step(gtol=-1.0) == EINVAL
    for name in ('sl', 'sg', 'sh', 'w', 'loss', 'grad', 'p', 't', 'info', 'trial', 'active'):
        assert _step(**{name: None}) == EINVAL, name
    assert _step(dim=33) == EUNSUPPORTED and _step(dim=33, w=None) == EINVAL
    assert _step(n_fit=0, w=None) == 0


# ------------------------------------------------------------------ Python surface
def test_fit_pairs_csr():
    n = 5
    fp = ops.fit_pairs_csr([[(0, 1), (1, 0), (0, 1), (2, 2), (3, 4)], [], [(4, 4)]], n)
    assert fp.ptr.tolist() == [0, 3, 3, 4] and fp.n_pairs.tolist() == [5, 0, 1]
    assert fp.u.tolist() == [0, 2, 3, 4] and fp.v.tolist() == [1, 2, 4, 4] and fp.u.dtype == torch.int32
    n0 = 25 - (2 + 1 + 2)                                                   # duplicates and mirrors are ONE recorded pair
    assert torch.allclose(fp.wpos, torch.tensor([3 / 5, 1 / 5, 1 / 5, 1.0]))
    assert torch.allclose(fp.dense_w, torch.tensor([1 / n0, 1 / 25, 1 / 24]))
    assert torch.allclose(fp.wneg, torch.tensor([2 / n0, 1 / n0, 2 / n0, 1 / 24]))
    keys, kptr = fp.known
    assert kptr.tolist() == [0, 5, 5, 6] and keys.tolist() == [1, 5, 12, 19, 23, 24]
    # the tensor form, and neg_weight
    idx = torch.tensor([[0, 1, 0, 2, 3, 4], [1, 0, 1, 2, 4, 4]])
    fq = ops.fit_pairs_csr((idx, torch.tensor([0, 5, 5, 6])), n, neg_weight=2.0)
    assert torch.equal(fq.u, fp.u) and torch.equal(fq.v, fp.v) and torch.equal(fq.ptr, fp.ptr)
    assert torch.allclose(fq.wneg, 2 * fp.wneg) and torch.allclose(fq.dense_w, 2 * fp.dense_w) and torch.equal(fq.wpos, fp.wpos)
    # every pair listed: N_b = 0
    every = [(u, v) for u in range(3) for v in range(u, 3)]
    fe = ops.fit_pairs_csr([every], 3)
    assert fe.dense_w.tolist() == [0.0] and fe.wneg.tolist() == [0.0] * 6 and fe.n_pairs.tolist() == [6]
    assert fe.known[0].tolist() == list(range(9))
    assert ops.fit_pairs_csr([], 3).ptr.tolist() == [0]
    for bad in ([[(0, 5)]], [[(-1, 0)]], [[(0, 1, 2)]], [[3]], 7, (idx, torch.tensor([0, 7])), (idx, torch.tensor([1, 6])),
                (idx.float(), torch.tensor([0, 6]))):
        with pytest.raises(ValueError):
            ops.fit_pairs_csr(bad, n)
    with pytest.raises(ValueError):
        ops.fit_pairs_csr([[(0, 1)]], 5, neg_weight=0.0)


def test_ops_refuse_cpu_tensors():
    fp = ops.fit_pairs_csr([[(0, 1)]], 5)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_fit_stats(torch.ones(5, 4), torch.ones(1, 4), fp)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_fit(torch.ones(5, 4), fp)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.distmult_fit(torch.ones(5, 4, dtype=torch.float64), fp)


def test_tip_fit_side_effects_refusals():
    assert NewSideEffects._fields == ('weight', 'loss', 'grad_norm', 'evaluations', 'status', 'n_pairs', 'decoder', 'known')
    assert 'NewSideEffects' in layers.__all__
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    dec = types.SimpleNamespace(in_dim=16)
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.fit_side_effects(types.SimpleNamespace(decoder_kind='nn', shard=None, data=data, decoder=dec), [[(0, 1)]], l2=-1)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.fit_side_effects(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data, decoder=dec), [[(0, 1)]], l2=-1)
    self = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=dec)
    for kw in ({'l2': -1e-3}, {'l2': float('nan')}, {'neg_weight': 0.0}, {'neg_weight': -1.0}, {'max_iter': -1}, {'gtol': -1.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TIP.fit_side_effects(self, [[(0, 1)]], **kw)
    for bad in ([[(0, 10)]], [[(-1, 2)]]):
        with pytest.raises(ValueError, match='out of range'):
            TIP.fit_side_effects(self, bad)
    new = types.SimpleNamespace(z=torch.zeros(2, 16))
    with pytest.raises(ValueError, match='out of range'):
        TIP.fit_side_effects(self, [[(0, 12)]], new=new)                    # two new drugs: ids up to 11
    for init in (torch.zeros(2, 16), torch.zeros(16), torch.zeros(1, 8)):
        with pytest.raises(ValueError, match='init'):
            TIP.fit_side_effects(self, [[(0, 1)]], init=init)
    wide = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=types.SimpleNamespace(in_dim=40))
    with pytest.raises(NotImplementedError, match='4m'):
        TIP.fit_side_effects(wide, [[(0, 1)]])


# ------------------------------------------------------------------ the spec
def _loop_stats(z, w, lst, l2, rho):
    """The definition as a plain Python loop over the ordered pairs, in floats."""
    n, dim = len(z), len(z[0])
    rec = set()
    for u, v in lst:
        rec.add((u, v)); rec.add((v, u))
    p_b, n_b = len(lst), n * n - len(rec)
    sp = lambda s: max(s, 0.0) + math.log1p(math.exp(-abs(s)))
    sg = lambda s: 1.0 / (1.0 + math.exp(-s)) if s >= 0 else math.exp(s) / (1.0 + math.exp(s))
    loss, g, h = 0.5 * l2 * sum(x * x for x in w), [l2 * x for x in w], [[l2 * (i == j) for j in range(dim)] for i in range(dim)]
    terms = [(u, v, 1.0 / p_b, -1.0) for u, v in lst]
    terms += [(u, v, rho / n_b, 1.0) for u in range(n) for v in range(n) if (u, v) not in rec]
    for u, v, c, sign in terms:
        f = [z[u][k] * z[v][k] for k in range(dim)]
        s = sign * sum(f[k] * w[k] for k in range(dim))
        loss += c * sp(s)
        for i in range(dim):
            g[i] += c * sign * sg(s) * f[i]
            for j in range(dim):
                h[i][j] += c * sg(s) * sg(-s) * f[i] * f[j]
    return loss, g, h


def test_spec_against_plain_loop():
    n, dim = 7, 4
    z = cases.embeddings(n, dim, 5, 2.0)
    lst = [(0, 1), (1, 0), (0, 1), (2, 2), (3, 6), (6, 5)]
    w = cases.trial_rows(2, dim, 'random', 9) * 3
    for rho, l2 in ((1.0, 1e-4), (2.5, 0.0)):
        t = spec_stats(z, w, [lst, []], l2, rho)
        loss, g, h = _loop_stats(z.double().tolist(), w[0].double().tolist(), lst, l2, rho)
        assert abs(float(t['loss'][0]) - loss) <= 1e-13 * (1 + abs(loss))
        assert torch.allclose(t['g'][0], torch.tensor(g, dtype=torch.float64), rtol=0, atol=1e-13)
        assert torch.allclose(t['H'][0], torch.tensor(h, dtype=torch.float64), rtol=0, atol=1e-13)
        # an empty list: negatives only, every ordered pair
        s = (z.double()[:, None, :] * z.double()[None, :, :]) @ w[1].double()
        want = rho / 49 * torch.nn.functional.softplus(s).sum() + 0.5 * l2 * (w[1].double() ** 2).sum()
        assert abs(float(t['loss'][1] - want)) <= 1e-13
        assert bool((t['A_loss'] >= t['loss'] - 1e-15).all()) and bool((t['T_loss'] > 0).all())


def test_spec_against_autograd():
    n, dim = 9, 4
    z = cases.embeddings(n, dim, 6, 2.0)
    lst = cases.random_pairs(n, 12, 3, selfs=True)
    w0 = cases.trial_rows(1, dim, 'random', 4)[0].double()
    loss_of = lambda w: spec_stats(z, w[None], [lst], 1e-3, 1.5, bounds=False)['loss'][0]
    t = spec_stats(z, w0[None], [lst], 1e-3, 1.5)
    g = torch.autograd.functional.jacobian(loss_of, w0)
    h = torch.autograd.functional.hessian(loss_of, w0)
    assert torch.allclose(t['g'][0], g, rtol=0, atol=1e-13) and torch.allclose(t['H'][0], h, rtol=0, atol=1e-13)
    p, fallback = newton_direction(t['g'][0], t['H'][0])
    assert not fallback and torch.allclose(t['H'][0] @ p, -t['g'][0], atol=1e-12)
    p, fallback = newton_direction(t['g'][0], -t['H'][0])
    assert fallback and torch.equal(p, -t['g'][0])                           # max of -H_ii is not > 0: -g
    h2 = t['H'][0].clone()
    h2[0, 0] = -1.0
    p, fallback = newton_direction(t['g'][0], h2)
    assert fallback and torch.allclose(p, -t['g'][0] / h2.diagonal().max())


# ------------------------------------------------------------------ the rule bites
def _decomposed(z, w, fp, l2, drop_l2_hess=False):
    """The device's decomposition in fp64 from the lists of a FitPairs: dense stream over u <= v plus the sparse correction."""
    z64, w64 = z.double(), w.double()
    n, dim = z64.shape
    iu, iv = torch.triu_indices(n, n)
    m = torch.where(iu == iv, 1.0, 2.0).double()
    f = z64[iu] * z64[iv]
    loss, grad, hess = [], [], []
    sp = torch.nn.functional.softplus
    for b in range(fp.dense_w.numel()):
        s = f @ w64[b]
        c = fp.dense_w[b].double() * m
        lo, hi = int(fp.ptr[b]), int(fp.ptr[b + 1])
        fs = z64[fp.u[lo:hi].long()] * z64[fp.v[lo:hi].long()]
        ss = fs @ w64[b]
        wp, wn = fp.wpos[lo:hi].double(), fp.wneg[lo:hi].double()
        loss.append((c * sp(s)).sum() + (wp * sp(-ss) - wn * sp(ss)).sum() + 0.5 * l2 * (w64[b] ** 2).sum())
        grad.append((c * torch.sigmoid(s)) @ f + (-wp * torch.sigmoid(-ss) - wn * torch.sigmoid(ss)) @ fs + l2 * w64[b])
        hd = torch.sigmoid(s) * torch.sigmoid(-s)
        hs = torch.sigmoid(ss) * torch.sigmoid(-ss)
        h = (f * (c * hd)[:, None]).t() @ f + (fs * ((wp - wn) * hs)[:, None]).t() @ fs
        hess.append(h if drop_l2_hess else h + l2 * torch.eye(dim, dtype=torch.float64))
    return torch.stack(loss).float(), torch.stack(grad).float(), torch.stack(hess).float()


def test_rule_accepts_the_decomposition_and_rejects_planted_mistakes():
    n, dim, l2 = 33, 8, 1e-2
    z = cases.embeddings(n, dim, 11, 2.0)
    lst = cases.random_pairs(n, 60, 12, selfs=True)
    lst = lst + [(v, u) for u, v in lst[:20]] + lst[:10] + [(4, 4), (4, 4)]
    w = cases.trial_rows(1, dim, 'random', 13) * 2
    d_chain = _lib.lib().tipk_distmult_fit_max_chain(n, dim, 1)
    fp = ops.fit_pairs_csr([lst], n)
    check_stats(z, w, [lst], l2, 1.0, _decomposed(z, w, fp, l2), d_chain, what='right')           # the right one passes
    big_n = 1.0 / float(fp.dense_w[0])
    selfs = fp.u == fp.v
    mistakes = {
        'a recorded pair also counted as a negative': fp._replace(wneg=torch.zeros_like(fp.wneg)),
        'self pairs with multiplicity 2': fp._replace(wneg=torch.where(selfs, 2 * fp.wneg, fp.wneg)),
        'mirrored listing counted twice in N_b': fp._replace(
            dense_w=fp.dense_w * big_n / (big_n - 40), wneg=fp.wneg * big_n / (big_n - 40)),
        'wpos not divided by P_b': fp._replace(wpos=fp.wpos * float(fp.n_pairs[0])),
    }
    for name, wrong in mistakes.items():
        with pytest.raises(AssertionError, match='off fp64'):
            check_stats(z, w, [lst], l2, 1.0, _decomposed(z, w, wrong, l2), d_chain, what=name)
    with pytest.raises(AssertionError, match='off fp64'):
        check_stats(z, w, [lst], l2, 1.0, _decomposed(z, w, fp, l2, drop_l2_hess=True), d_chain, what='l2 left out of H')
    # NaN placement: a NaN that leaks into another relation, and one that is missing
    two = [lst, lst[:7]]
    fp2 = ops.fit_pairs_csr(two, n)
    w2 = torch.cat([w, w])
    w2[1, 3] = float('nan')
    good = _decomposed(z, w2, fp2, l2)
    assert bool(torch.isnan(good[0][1])) and not bool(torch.isnan(good[0][0]))
    check_stats(z, w2, two, l2, 1.0, good, d_chain, what='nan')
    leak = tuple(x.clone() for x in good)
    leak[1][0, 2] = float('nan')
    with pytest.raises(AssertionError, match='without a NaN logit'):
        check_stats(z, w2, two, l2, 1.0, leak, d_chain)
    miss = tuple(x.clone() for x in good)
    miss[2][1, 0, 0] = 0.0
    with pytest.raises(AssertionError, match='must be all NaN'):
        check_stats(z, w2, two, l2, 1.0, miss, d_chain)


# ------------------------------------------------------------------ condition, not measurement
@pytest.mark.parametrize('case', cases.convergence_cases(), ids=lambda c: c[0])
def test_convergence_cases_converge_within_8_evaluations(case):
    name, z, pairs = case
    got = spec_fit(z, pairs, l2=1e-4, rho=1.0, init=None, max_iter=16, gtol=1e-5)
    status, evals, acc, rej = got['info'][0].tolist()
    print(name, 'evaluations', evals, 'rejected', rej, 'loss', float(got['loss'][0]))
    assert status == 1 and evals <= 8 and evals == acc + rej + 1, (name, got['info'][0].tolist())
    # and in fp32-sized slack: the 16 ulp of the rule never make the fp64 iteration reject a step here
    assert rej == 0, (name, rej)
