"""CPU tests of the per-relation calibration (include/tipk.h section 4r): the symbols and the shape queries, argument validation
of the two C entries (every refusal happens before anything touches a device, so bogus device pointers are safe here), the
list builder `ops.calibration_lists` against a brute-force set construction, `Calibration.embed` and the widened decoder on
the CPU oracle, the refusals of `TIP.calibrate` and of the `calibration=` keyword, the fp64 spec (tests/calibration_spec.py)
against a plain loop and autograd, planted mistakes the acceptance rule must reject, and the convergence condition of the fit
cases."""
import ctypes
import inspect
import math
import os
import pickle
import types

import pytest
import torch

import calibration_cases as cases
from calibration_spec import C_CAL, U, cell_sets, check_stats, spec_fit, spec_stats
from conftest import GOLDEN
from oracle import tip_oracle as O
from tip_amd import _lib, layers, ops
from tip_amd.layers import TIP, Calibration, calibrated_operands

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch
SYMBOLS = ('tipk_distmult_calibrate_supported', 'tipk_distmult_calibrate_splits', 'tipk_distmult_calibrate_max_chain',
           'tipk_distmult_calibrate_workspace_bytes', 'tipk_distmult_calibrate_stats', 'tipk_distmult_calibrate')
QUERIES = ('side_effects', 'regimen_side_effects', 'add_on_risk', 'combination_risk', 'drug_profile', 'screen')


def _stats(n=10, dim=16, n_rel=7, n_q=3, n_pairs=5, l2=1e-6, z=FAKE, w=FAKE, qrel=FAKE, ab=FAKE, dense=FAKE, pptr=FAKE, pu=FAKE,
           pv=FAKE, wpos=FAKE, wneg=FAKE, active=None, loss=FAKE, grad=FAKE, hess=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_calibrate_stats(z, n, dim, w, n_rel, qrel, ab, n_q, dense, pptr, pu, pv, wpos, wneg, n_pairs,
                                                    l2, active, loss, grad, hess, ws, None)


def _fit(n=10, dim=16, n_rel=7, n_q=3, n_pairs=5, l2=1e-6, max_iter=4, gtol=1e-6, z=FAKE, w=FAKE, qrel=FAKE, dense=FAKE,
         pptr=FAKE, pu=FAKE, pv=FAKE, wpos=FAKE, wneg=FAKE, init=None, ab=FAKE, loss=FAKE, grad=FAKE, info=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_calibrate(z, n, dim, w, n_rel, qrel, n_q, dense, pptr, pu, pv, wpos, wneg, n_pairs, l2, init,
                                              max_iter, gtol, ab, loss, grad, info, ws, None)


# ------------------------------------------------------------------ symbols and statuses
def test_symbols_and_shape_queries():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30            # purely additive
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    sup, splits, chain, wsb = (L.tipk_distmult_calibrate_supported, L.tipk_distmult_calibrate_splits,
                               L.tipk_distmult_calibrate_max_chain, L.tipk_distmult_calibrate_workspace_bytes)
    for n in (-1, 0, 1, 2, 645, 46340, 46341, 2 ** 40):
        for dim in (0, 2, 4, 6, 16, 20, 36, 256, 260):
            for n_q in (0, 1, 64, 65536, 65537):
                want = 1 <= n <= 46340 and dim % 4 == 0 and 4 <= dim <= 256 and 1 <= n_q <= 65536
                assert sup(n, dim, n_q) == int(want), (n, dim, n_q)
                if want:
                    assert chain(n, dim, n_q) == 18                     # 16 cells of a thread in a tile, the rounding, fp64
                else:
                    assert splits(n, dim, n_q) == -1 and chain(n, dim, n_q) == -1
                    assert wsb(n, dim, n_q) == (0 if n_q == 0 and sup(n, dim, 1) else -1)
    # BioSNAP: 11 tile rows, 66 tiles.  1 097 queries: 3 parts each; 64: all 64; one query: no more parts than tiles
    assert splits(645, 16, 1097) == 3 and splits(645, 16, 64) == 64 and splits(645, 16, 1) == 64
    assert splits(130, 16, 1) == 6 and splits(64, 16, 1) == 1 and splits(65, 16, 5) == 3 and splits(130, 36, 70) == 6
    assert splits(130, 16, 4097) == 1 and splits(2, 4, 1) == 1
    state = lambda q: sum((v + 255) // 256 * 256 for v in (q * 8, q * 4, q * 8, q * 4, q * 4, q * 8, q * 16))
    assert wsb(645, 16, 1097) == (1097 * 3 * 6 * 8 + 255) // 256 * 256 + state(1097)
    assert wsb(645, 16, 0) == 0


def test_status_order():
    for call in (_stats, _fit):
        assert call(n_q=0) == 0                                            # nothing to do: OK with no launch
        assert call(n_q=0, z=None, ws=None) == 0
        for bad in ({'n': 0}, {'dim': 0}, {'n_rel': 0}, {'n_q': -1}, {'n_pairs': -1}, {'l2': -1e-3}, {'l2': math.nan},
                    {'z': None}, {'w': None}, {'qrel': None}, {'dense': None}, {'pptr': None}, {'loss': None}, {'grad': None},
                    {'ws': None}, {'pu': None}, {'pv': None}, {'wpos': None}, {'wneg': None}):
            assert call(**bad) == EINVAL, bad
        # EINVAL comes first: an unsupported shape with an invalid argument is invalid
        assert call(dim=6, l2=-1.0) == EINVAL and call(n=46341, z=None) == EINVAL
        for unsupported in ({'dim': 6}, {'dim': 260}, {'n': 46341}, {'n_q': 65537}, {'z': ctypes.c_void_p((1 << 20) + 4)}):
            assert call(**unsupported) == EUNSUPPORTED, unsupported
        assert call(n_pairs=0, pu=None, pv=None, wpos=None, wneg=None, dim=6) == EUNSUPPORTED     # the cell arrays may be NULL
    assert _stats(ab=None) == EINVAL and _stats(hess=None) == EINVAL
    for bad in ({'max_iter': -1}, {'gtol': -1.0}, {'gtol': math.nan}, {'ab': None}, {'info': None}):
        assert _fit(**bad) == EINVAL, bad
    assert _fit(max_iter=-1, dim=6) == EINVAL


# ------------------------------------------------------------------ the list builder
@pytest.mark.parametrize('case', cases.stats_cases(), ids=lambda c: c['name'])
def test_calibration_lists_against_sets(case):
    n, rel = case['z'].shape[0], case['relations']
    n_rel = case['w'].shape[0]
    cl = ops.calibration_lists(case['train'], case['given'], n, n_rel, rel)
    iu, iv, trn, pos, dropped = cell_sets(case['train'], case['given'], n, rel)
    assert cl.q_rel.dtype == torch.int32 and cl.q_rel.tolist() == rel.tolist()
    assert cl.ptr.dtype == torch.int64 and cl.u.dtype == cl.v.dtype == torch.int32
    assert cl.n_pos.dtype == cl.n_neg.dtype == cl.n_dropped.dtype == torch.int64
    assert cl.n_pos.tolist() == pos.sum(1).tolist() and cl.n_dropped.tolist() == dropped.tolist()
    assert cl.n_neg.tolist() == (~trn & ~pos).sum(1).tolist()
    for q in range(rel.numel()):
        lo, hi = int(cl.ptr[q]), int(cl.ptr[q + 1])
        listed = trn[q] | pos[q]
        want = list(zip(iu[listed].tolist(), iv[listed].tolist()))          # row-major u < v: sorted by (u, v)
        assert list(zip(cl.u[lo:hi].tolist(), cl.v[lo:hi].tolist())) == want, (case['name'], q)
        m = int(cl.n_pos[q] + cl.n_neg[q])
        inv = 1.0 / m if m else 0.0
        assert float(cl.dense_w[q]) == pytest.approx(inv, rel=1e-7, abs=0)
        assert torch.equal(cl.wneg[lo:hi], torch.full((hi - lo,), -inv).float())
        assert torch.equal(cl.wpos[lo:hi], torch.where(pos[q][listed], inv, 0.0).float())
    assert int(cl.ptr[-1]) == cl.u.numel() == cl.wpos.numel() == cl.wneg.numel()
    everyone = ops.calibration_lists(case['train'], case['given'], n, n_rel)                  # relations = None: all, ascending
    sub = ops.calibration_queries(everyone, rel)                         # a row subset is the list built for those queries
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(sub, cl))
    assert everyone.q_rel.tolist() == list(range(n_rel))
    assert everyone.n_pos.flip(0)[:rel.numel()].tolist() == cl.n_pos.tolist()


def test_calibration_lists_refusals():
    ok = (torch.tensor([[0, 1], [1, 2]]), torch.tensor([0, 1]))
    empty = (torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    cl = ops.calibration_lists(empty, empty, 4, 2)
    assert cl.n_pos.tolist() == [0, 0] and cl.n_neg.tolist() == [6, 6] and cl.u.numel() == 0
    assert ops.calibration_lists(ok, ok, 3, 2, []).ptr.tolist() == [0]
    for bad in ((torch.tensor([[0, 3], [1, 2]]), ok[1]), (torch.tensor([[0, -1], [1, 2]]), ok[1]), (ok[0], torch.tensor([0, 2])),
                (ok[0], torch.tensor([0, -1])), (ok[0].float(), ok[1]), (ok[0], ok[1][:1]), (ok[0][0], ok[1])):
        with pytest.raises(ValueError, match='train'):
            ops.calibration_lists(bad, ok, 3, 2)
        with pytest.raises(ValueError, match='given'):
            ops.calibration_lists(ok, bad, 3, 2)
    for rel in ([2], [-1], [0.5]):
        with pytest.raises(ValueError, match='relations'):
            ops.calibration_lists(ok, ok, 3, 2, rel)
    with pytest.raises(ValueError, match='n_nodes'):
        ops.calibration_lists(ok, ok, 0, 2)


def test_ops_refuse_cpu_tensors():
    e = (torch.tensor([[0], [1]]), torch.tensor([0]))
    cl = ops.calibration_lists(e, (torch.tensor([[1], [2]]), torch.tensor([0])), 5, 3)
    assert ops.distmult_calibrate_supported(5, 4, 3) and not ops.distmult_calibrate_supported(5, 6, 3)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_calibrate_stats(torch.ones(5, 4), torch.ones(3, 4), torch.ones(3, 2), cl)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_calibrate(torch.ones(5, 4), torch.ones(3, 4), cl)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.distmult_calibrate(torch.ones(5, 4, dtype=torch.float64), torch.ones(3, 4), cl)


# ------------------------------------------------------------------ applying the map: widened operands on the CPU oracle
def _calibration_for(z, w, ab):
    wide, dec = calibrated_operands(z, w, ab)
    r = w.shape[0]
    zf, zi = torch.zeros(r), torch.zeros(r, dtype=torch.int64)
    return Calibration(ab[:, 0].clone(), ab[:, 1].clone(), zf, zf, zf, zi, zi, zi, zi, zi, wide, dec)


@pytest.mark.parametrize('dim', [4, 16, 36])
def test_widened_operands_compute_a_s_plus_b(dim):
    n, r = 33, 7
    z, w = cases.embeddings(n, dim, 5 + dim), cases.decoder_rows(r, dim, 6 + dim)
    g = torch.Generator().manual_seed(dim)
    ab = torch.stack([torch.rand(r, generator=g) * 3 + 0.1, torch.randn(r, generator=g) * 4], 1).float()
    ab[0] = torch.tensor([1.0, 0.0])
    cal = _calibration_for(z, w, ab)
    assert cal.z.shape == (n, dim + 4) and torch.equal(cal.z[:, :dim], z) and not cal.z.requires_grad
    assert torch.equal(cal.z[:, dim:], torch.tensor([1.0, 0, 0, 0]).repeat(n, 1))
    assert isinstance(cal.decoder, layers.MultiInnerProductDecoder) and cal.decoder.in_dim == dim + 4 and cal.decoder.num_et == r
    assert not cal.decoder.weight.requires_grad and torch.equal(cal.decoder.weight[:, dim + 1:], torch.zeros(r, 3))
    idx = torch.randint(0, n, (2, 400), generator=g)
    et = torch.randint(0, r, (400,), generator=g)
    got = O.distmult_fwd(cal.z, idx, et, cal.decoder.weight.detach(), sigmoid=False)
    s = O.distmult_fwd(z.double(), idx, et, w.double(), sigmoid=False)
    want = ab[et, 0].double() * s + ab[et, 1].double()
    # fp32 rounding: a w is rounded once, then dim + 1 products and additions of terms bounded by sum |a z z w| + |b|
    room = (dim + 4) * U * (ab[et, 0].double().abs() * (z[idx[0]].double() * z[idx[1]].double() * w[et].double()).abs().sum(1)
                            + ab[et, 1].double().abs())
    assert bool(((got.double() - want).abs() <= room).all()), float(((got.double() - want).abs() - room).max())
    raw = O.distmult_fwd(z, idx, et, w, sigmoid=False)
    assert torch.allclose(got[et == 0], raw[et == 0], rtol=0, atol=float(room.max()))                # the identity map
    # embed pads further rows the same way, on the calibration's device and dtype
    more = cases.embeddings(5, dim, 77)
    wide = cal.embed(more)
    assert wide.shape == (5, dim + 4) and torch.equal(wide[:, :dim], more)
    assert torch.equal(wide[:, dim:], torch.tensor([1.0, 0, 0, 0]).repeat(5, 1))
    assert cal.embed(more.double()).dtype == torch.float32
    for bad in (torch.zeros(5, dim + 4), torch.zeros(dim), torch.zeros(2, 3, dim)):
        with pytest.raises(ValueError, match='embed'):
            cal.embed(bad)


# ------------------------------------------------------------------ the Python surface refuses before it touches a device
def _small_sizes():
    with open(os.path.join(GOLDEN, 'data_dict_small.pkl'), 'rb') as f:
        dd = pickle.load(f)
    return int(dd['n_drug']), int(dd['n_dd_et'])


def test_tip_calibrate_refusals():
    assert Calibration._fields == ('scale', 'offset', 'loss', 'loss_raw', 'expected_raw', 'n_pos', 'n_neg', 'n_dropped',
                                   'evaluations', 'status', 'z', 'decoder')
    assert 'Calibration' in layers.__all__
    sig = inspect.signature(TIP.calibrate)
    assert list(sig.parameters) == ['self', 'pairs', 'relations', 'l2', 'init', 'max_iter', 'gtol']
    assert sig.parameters['l2'].default == 1e-6 and sig.parameters['max_iter'].default == 32
    assert sig.parameters['gtol'].default >= 1e-6                          # above the fp32 noise floor
    n, nr = _small_sizes()
    data = types.SimpleNamespace(n_drug=n, n_dd_et=nr)
    dec = types.SimpleNamespace(in_dim=16)
    pairs = (torch.tensor([[0], [1]]), torch.tensor([0]))
    with pytest.raises(NotImplementedError, match='4r'):
        TIP.calibrate(types.SimpleNamespace(decoder_kind='nn', shard=None, data=data, decoder=dec), pairs, l2=-1)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.calibrate(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data, decoder=dec), pairs, l2=-1)
    self = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=dec)
    for kw in ({'l2': -1e-3}, {'l2': float('nan')}, {'gtol': -1.0}, {'gtol': float('nan')}, {'max_iter': -1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TIP.calibrate(self, pairs, **kw)
    for init in (torch.zeros(nr, 3), torch.zeros(nr), torch.zeros(nr + 1, 2)):
        with pytest.raises(ValueError, match='init'):
            TIP.calibrate(self, pairs, init=init)
    for bad in ((torch.tensor([[n], [0]]), torch.tensor([0])), (torch.tensor([[0], [-1]]), torch.tensor([0])),
                (torch.tensor([[0], [1]]), torch.tensor([nr])), (torch.tensor([[0.5], [1]]), torch.tensor([0])),
                (torch.tensor([[0, 1], [1, 2]]), torch.tensor([0]))):
        with pytest.raises(ValueError):
            TIP.calibrate(self, bad)
    for rel in ([nr], [-1]):
        with pytest.raises(ValueError, match='side-effect id'):
            TIP.calibrate(self, pairs, relations=rel)
    wide = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=types.SimpleNamespace(in_dim=256))
    with pytest.raises(NotImplementedError, match='4r'):                   # dim + 4 leaves the serving entries' range
        TIP.calibrate(wide, pairs)
    odd = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=types.SimpleNamespace(in_dim=18))
    with pytest.raises(NotImplementedError, match='4r'):
        TIP.calibrate(odd, pairs)


def test_calibration_keyword_and_mismatch():
    for name in QUERIES:
        params = list(inspect.signature(getattr(TIP, name)).parameters.values())
        assert params[-1].name == 'calibration' and params[-1].default is None, name          # at the END of the signature
        doc = getattr(TIP, name).__doc__
        assert 'SNAPSHOT' in doc and 'scale > 0' in doc, name
    n, r, dim = 12, 5, 16
    z, w = cases.embeddings(n, dim, 1), cases.decoder_rows(r, dim, 2)
    cal = _calibration_for(z, w, torch.tensor([[2.0, -1.0]]).repeat(r, 1))
    model = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=types.SimpleNamespace(n_drug=n, n_dd_et=r),
                                  decoder=types.SimpleNamespace(in_dim=dim, num_et=r), embeddings=z)
    assert layers._scoring_operands(model, None) == (z, model.decoder)        # None: the model's own, nothing looked at
    got = layers._scoring_operands(model, cal)
    assert got[0] is cal.z and got[1] is cal.decoder
    for other in (types.SimpleNamespace(n_drug=n + 1, n_dd_et=r), ):
        with pytest.raises(ValueError, match='calibration'):
            layers._scoring_operands(types.SimpleNamespace(**{**vars(model), 'data': other}), cal)
    for other in (types.SimpleNamespace(in_dim=dim + 4, num_et=r), types.SimpleNamespace(in_dim=dim, num_et=r + 1)):
        with pytest.raises(ValueError, match='calibration'):
            layers._scoring_operands(types.SimpleNamespace(**{**vars(model), 'decoder': other}), cal)
    with pytest.raises(ValueError, match='calibration'):
        layers._scoring_operands(model, (z, w))
    elsewhere = types.SimpleNamespace(**{**vars(model), 'embeddings': types.SimpleNamespace(device=torch.device('meta'))})
    with pytest.raises(ValueError, match='operands are on'):
        layers._scoring_operands(elsewhere, cal)
    with pytest.raises(NotImplementedError, match='NN decoder'):
        layers._scoring_operands(types.SimpleNamespace(**{**vars(model), 'decoder_kind': 'nn'}), cal)
    with pytest.raises(NotImplementedError, match='shard'):
        layers._scoring_operands(types.SimpleNamespace(**{**vars(model), 'shard': object()}), cal)


# ------------------------------------------------------------------ the spec
def _loop_stats(z, w_r, a, b, train, given, l2):
    """The definition as a plain Python loop over the cells of ONE relation, in floats; train, given: sets of (u, v), u < v."""
    n, dim = len(z), len(w_r)
    sp = lambda s: max(s, 0.0) + math.log1p(math.exp(-abs(s)))
    sg = lambda s: 1.0 / (1.0 + math.exp(-s)) if s >= 0 else math.exp(s) / (1.0 + math.exp(s))
    cells = [(u, v) for u in range(n) for v in range(u + 1, n) if (u, v) not in train]
    m = len(cells)
    loss, g, h = 0.5 * l2 * (a - 1) ** 2, [l2 * (a - 1), 0.0], [[l2, 0.0], [0.0, 0.0]]
    for u, v in cells:
        s = sum(z[u][k] * w_r[k] * z[v][k] for k in range(dim))
        t = a * s + b
        phi = (s, 1.0)
        sign = -1.0 if (u, v) in given else 1.0
        loss += sp(sign * t) / m
        for i in range(2):
            g[i] += sign * sg(sign * t) * phi[i] / m
            for j in range(2):
                h[i][j] += sg(t) * sg(-t) * phi[i] * phi[j] / m
    return loss, g, h


def test_spec_against_plain_loop_and_autograd():
    case = cases.make_case('loop', 9, 4, 3, ('mixed', 'planted', 'untrained'), 50)
    z, w, rel = case['z'], case['w'], case['relations']
    ab = torch.tensor([[1.3, -0.7], [0.4, 0.2], [-2.0, 1.0]])
    t = spec_stats(z, w, ab, case['train'], case['given'], rel, 1e-2)
    iu, iv, trn, pos, _ = cell_sets(case['train'], case['given'], 9, rel)
    for q in range(3):
        tr = {c for c, f in zip(zip(iu.tolist(), iv.tolist()), trn[q].tolist()) if f}
        gv = {c for c, f in zip(zip(iu.tolist(), iv.tolist()), pos[q].tolist()) if f}
        loss, g, h = _loop_stats(z.double().tolist(), w[int(rel[q])].double().tolist(), float(ab[q, 0]), float(ab[q, 1]), tr, gv,
                                 1e-2)
        assert float(t['loss'][q]) == pytest.approx(loss, rel=1e-12)
        assert t['g'][q].tolist() == pytest.approx(g, rel=1e-10, abs=1e-14)
        assert t['H'][q].reshape(-1).tolist() == pytest.approx(sum(h, []), rel=1e-10, abs=1e-14)
        one = lambda x: spec_stats(z, w, x[None], case['train'], case['given'], rel[q:q + 1], 1e-2, bounds=False)['loss'][0]
        x0 = ab[q].double()
        assert torch.allclose(t['g'][q], torch.autograd.functional.jacobian(one, x0), rtol=0, atol=1e-13)
        assert torch.allclose(t['H'][q], torch.autograd.functional.hessian(one, x0), rtol=0, atol=1e-13)
    # the identity (e): dL/db = (expected - n_pos) / M
    m = (t['n_pos'] + t['n_neg']).double()
    assert torch.allclose(t['g'][:, 1] * m, t['expected'] - t['n_pos'].double(), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ the rule bites
def _decomposed(z, w, ab, cl, l2, n_cells_dropped=0):
    """The device's decomposition -- dense_w times a stream over ALL cells, the correction over the listed cells, the l2 term
    -- evaluated in fp64 and rounded to fp32."""
    z64, w64, ab64 = z.double(), w.double(), ab.double()
    n = z64.shape[0]
    iu, iv = torch.triu_indices(n, n, 1)
    iu, iv = iu[:iu.numel() - n_cells_dropped], iv[:iv.numel() - n_cells_dropped]
    sp, sg = torch.nn.functional.softplus, torch.sigmoid
    loss, grad, hess = [], [], []
    for q in range(cl.q_rel.numel()):
        wr, (a, b) = w64[int(cl.q_rel[q])], ab64[q]
        lo, hi = int(cl.ptr[q]), int(cl.ptr[q + 1])

        def terms(u, v):
            s = ((z64[u] * wr) * z64[v]).sum(1)
            return s, a * s + b, torch.stack([s, torch.ones_like(s)], 1)
        s, t, phi = terms(iu, iv)
        ss, ts, phis = terms(cl.u[lo:hi].long(), cl.v[lo:hi].long())
        c, wp, wn = cl.dense_w[q].double(), cl.wpos[lo:hi].double(), cl.wneg[lo:hi].double()
        da = a - 1.0
        loss.append(c * sp(t).sum() + (wp * sp(-ts) + wn * sp(ts)).sum() + 0.5 * l2 * da * da)
        grad.append(c * sg(t) @ phi + (wn * sg(ts) - wp * sg(-ts)) @ phis + l2 * da * torch.tensor([1.0, 0.0], dtype=torch.float64))
        hd, hs = sg(t) * sg(-t), sg(ts) * sg(-ts)
        hess.append((phi * (c * hd)[:, None]).t() @ phi + (phis * ((wp + wn) * hs)[:, None]).t() @ phis
                    + l2 * torch.tensor([[1.0, 0.0], [0.0, 0.0]], dtype=torch.float64))
    return torch.stack(loss).float(), torch.stack(grad).float(), torch.stack(hess).float()


def test_rule_accepts_the_decomposition_and_rejects_planted_mistakes():
    case = cases.make_case('rule', 33, 8, 2, ('mixed', 'planted'), 60)
    z, w, rel = case['z'], case['w'], case['relations']
    n, l2 = 33, 1e-3
    ab = torch.tensor([[1.4, -1.0], [0.8, -2.0]])
    cl = ops.calibration_lists(case['train'], case['given'], n, w.shape[0], rel)
    spec = spec_stats(z, w, ab, case['train'], case['given'], rel, l2)
    d_chain = _lib.lib().tipk_distmult_calibrate_max_chain(n, 8, 2)
    assert C_CAL >= 4.0
    check_stats(_decomposed(z, w, ab, cl, l2), spec, d_chain, what='right')                   # the right one passes
    is_pos = cl.wpos > 0
    m = (cl.n_pos + cl.n_neg).double()
    cells = n * (n - 1) / 2
    per_cell = torch.repeat_interleave(m / cells, cl.ptr[1:] - cl.ptr[:-1]).float()
    mistakes = {
        'a training cell not taken out of the stream': (cl._replace(wneg=torch.where(is_pos, cl.wneg, torch.zeros_like(cl.wneg))), 0),
        'a positive still counted as a negative': (cl._replace(wneg=torch.where(is_pos, torch.zeros_like(cl.wneg), cl.wneg)), 0),
        'M with the training cells left in': (cl._replace(dense_w=(cl.dense_w.double() * m / cells).float(),
                                                          wpos=cl.wpos * per_cell, wneg=cl.wneg * per_cell), 0),
        'a dropped last tile row': (cl, 3),
        'the wrong relation': (cl._replace(q_rel=cl.q_rel.flip(0)), 0),
    }
    for name, (lists, drop) in mistakes.items():
        with pytest.raises(AssertionError, match='off fp64'):
            check_stats(_decomposed(z, w, ab, lists, l2, drop), spec, d_chain, what=name)
    with pytest.raises(AssertionError, match='off fp64'):                                      # l2 pulling a to 0, not to 1
        check_stats(_decomposed(z, w, ab - torch.tensor([[1.0, 0.0]]), cl, l2), spec_stats(
            z, w, ab - torch.tensor([[1.0, 0.0]]), case['train'], case['given'], rel, 1e3), d_chain, what='l2 centre')
    # NaN placement: a NaN that leaks into another query, and one that is missing
    ab2 = ab.clone()
    ab2[1, 1] = float('nan')
    spec2 = spec_stats(z, w, ab2, case['train'], case['given'], rel, l2)
    good = _decomposed(z, w, ab2, cl, l2)
    assert bool(torch.isnan(good[0][1])) and not bool(torch.isnan(good[0][0]))
    check_stats(good, spec2, d_chain, what='nan')
    leak = tuple(v.clone() for v in good)
    leak[1][0, 1] = float('nan')
    with pytest.raises(AssertionError, match='without a NaN logit'):
        check_stats(leak, spec2, d_chain)
    miss = tuple(v.clone() for v in good)
    miss[2][1, 0, 0] = 0.0
    with pytest.raises(AssertionError, match='must be all NaN'):
        check_stats(miss, spec2, d_chain)


# ------------------------------------------------------------------ condition, not measurement
@pytest.mark.parametrize('case', cases.fit_cases(), ids=lambda c: c['name'])
def test_fit_cases_converge_within_16_evaluations(case):
    """What the GPU tests rely on: from the prevalence start the fp64 step rule reaches max |g| <= gtol within 16 evaluations
    on every fit case (a case that needs more is replaced, not given a longer limit)."""
    z, w, rel = case['z'], case['w'], case['relations']
    sets = cell_sets(case['train'], case['given'], z.shape[0], rel)
    at = spec_stats(z, w, torch.tensor([[1.0, 0.0]]).repeat(rel.numel(), 1), case['train'], case['given'], rel, cases.L2,
                    bounds=False, sets=sets)
    assert bool((at['n_pos'] > 0).all()) and bool((at['n_neg'] > 0).all())   # both classes present: the fit takes them
    start = cases.prevalence_start(at['n_pos'], at['n_neg'])
    got = spec_fit(z, w, case['train'], case['given'], rel, cases.L2, init=start, max_iter=cases.MAX_EVALUATIONS - 1,
                   gtol=cases.GTOL, sets=sets)
    info = got['info']
    print(case['name'], 'evaluations', info[:, 1].tolist(), 'scale', got['ab'][:, 0].tolist())
    assert bool((info[:, 0] == 1).all()) and int(info[:, 1].max()) <= cases.MAX_EVALUATIONS, info.tolist()
    assert bool((got['g'].abs().amax(1) <= cases.GTOL).all())
    assert bool((info[:, 1] == info[:, 2] + info[:, 3] + 1).all())
