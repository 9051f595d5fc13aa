"""Host tests of the confidence path (include/tipk.h section 4p; no GPU): the fp64 spec against a direct inverse, the cases'
conditioning, the binding, and every refusal of `TIP.decoder_posterior` / `TIP.side_effects_confidence`."""
import math
import types

import pytest
import torch

import conf_cases as cases
from conf_spec import KAPPA_CAP, U, check_factor, conf_tables, kappa2, logical, posterior64, spec_pair_conf, sym_lower
from fit_spec import spec_stats
from tip_amd import _lib, layers, ops
from tip_amd.layers import TIP, ConfidentSideEffects, DecoderPosterior


def test_spec_variance_is_the_quadratic_form_of_the_inverse():
    n, dim = 9, 8
    z, lists, w = cases.end_to_end_case(n, dim, 'random')
    t = spec_stats(z, w, lists, 1e-3, 1.5, bounds=False)
    n_pairs = torch.tensor([len(l) for l in lists], dtype=torch.int64)
    chol, w64 = posterior64(t['H'], n_pairs)
    iu, iv = torch.triu_indices(n, n)
    tab = conf_tables(z, w, w64, iu, iv, 0, 0.0)
    phi = z.double()[iu] * z.double()[iv]
    for b in range(len(lists)):
        sigma = torch.linalg.inv(float(n_pairs[b]) * t['H'][b])
        want = torch.einsum('pi,ij,pj->p', phi, sigma, phi)
        assert torch.allclose(tab['var'][:, b], want, rtol=1e-10, atol=1e-300)
        assert torch.allclose(w64[b].t() @ w64[b], sigma, rtol=1e-10, atol=1e-300)
        assert torch.allclose(tab['s'][:, b], phi @ w[b].double(), rtol=1e-13, atol=1e-300)
    key = tab['s'] / (1 + math.pi / 8 * tab['var']).sqrt()
    assert torch.equal(tab['key'], key)
    assert torch.equal(conf_tables(z, w, w64, iu, iv, 1, -1.645)['key'], tab['s'] - 1.645 * tab['var'].sqrt())
    assert bool((tab['tau_key'] >= 0).all()) and bool(torch.isfinite(tab['tau_key']).all())


def test_tau_key_stays_finite_at_zero_variance():
    z = torch.zeros((3, 4))
    z[1] = 1.0
    w = torch.ones((2, 4))
    fac = torch.eye(4).expand(2, 4, 4)
    u, v = torch.tensor([0, 1]), torch.tensor([0, 1])
    for mode, c in ((0, 0.0), (1, -1.645), (1, 2.0)):
        t = conf_tables(z, w, fac, u, v, mode, c)
        assert bool(torch.isfinite(t['tau_key']).all()) and float(t['var'][0, 0]) == 0 and float(t['tau_key'][0, 0]) == 0


def test_spec_topk_orders_and_filters():
    z, rel_w, w_phys = cases.query_case(6, 4, 5, 3)
    known = (torch.tensor([0 * 6 + 1]), torch.tensor([0, 2]), torch.tensor([1, 3], dtype=torch.int32))
    key, rel, s, var = spec_pair_conf(z, rel_w, logical(w_phys), torch.tensor([[1, 2], [0, 3]]), 4, 0, 0.0, known)
    assert sorted(rel[0].tolist()) == [-1, 0, 2, 4] and rel[0, 3] == -1               # pair (1, 0): relations 1 and 3 known
    assert len(set(rel[1].tolist())) == 4 and int(rel[1].min()) >= 0                  # pair (2, 3): nothing known, a full row
    assert bool((key[:, :-1] >= key[:, 1:]).all()) and float(var[0, 3]) == float('inf') and float(s[0, 3]) == float('-inf')


@pytest.mark.parametrize('name,n,dim,kind,l2', cases.END_TO_END)
def test_end_to_end_cases_are_well_conditioned(name, n, dim, kind, l2):
    z, lists, w = cases.end_to_end_case(n, dim, kind)
    h = spec_stats(z, w, lists, l2, 1.0, bounds=False)['H']
    worst = float((dim * U * kappa2(h)).max())
    print('%s: dim U kappa_2 = %.3g' % (name, worst))
    assert worst <= KAPPA_CAP / 2, (name, worst)                          # (room for the device's Hessian to differ)


def test_factor_rule_accepts_fp64_factors_and_rejects_planted_mistakes():
    h = cases.spd_matrices(5, 12, 7)
    r = torch.tensor([1.0, 3.0 ** -0.5, 7600.0 ** -0.5, 1.0, 1.0])
    chol, w64 = posterior64(h, r.double() ** -2)
    good = (chol.float(), w64.transpose(1, 2).contiguous().float(), torch.ones(5, dtype=torch.int32))
    check_factor(h, r, good)
    wrong = chol.float().clone()
    wrong[2, 5, 3] *= 1 + 1e-4
    with pytest.raises(AssertionError, match='L L'):
        check_factor(h, r, (wrong, good[1], good[2]))
    with pytest.raises(AssertionError, match='upper triangle'):
        check_factor(h, r, (good[0], w64.contiguous().float(), good[2]))          # the logical layout, not the physical one
    wrong = good[1].clone()
    wrong[1, 2, 7] *= 1 + 1e-4                                                    # W[7][2] of row 1
    with pytest.raises(AssertionError, match='L W'):
        check_factor(h, r, (good[0], wrong, good[2]))
    with pytest.raises(AssertionError, match='L W'):
        check_factor(h, torch.ones(5), good)                                      # the row scale is part of the rule
    bad_zero = (good[0].clone(), good[1].clone(), torch.tensor([1, 0, 1, 1, 1], dtype=torch.int32))
    with pytest.raises(AssertionError, match='bad row'):
        check_factor(h, r, bad_zero)
    assert torch.equal(sym_lower(torch.tensor([[1.0, 9.0], [2.0, 3.0]])), torch.tensor([[1.0, 2.0], [2.0, 3.0]]))


def test_binding_has_both_entries_and_the_abi_is_30():
    assert _lib.ABI_VERSION == 30
    for name in ('tipk_spd_factor', 'tipk_distmult_pair_conf_topk', 'tipk_distmult_pair_conf_topk_supported'):
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['tipk_spd_factor'][1]) == 8 and len(_lib.SIGNATURES['tipk_distmult_pair_conf_topk'][1]) == 23
    assert _lib._CONSTANTS['CONF_MODERATED'] == 0 and _lib._CONSTANTS['CONF_BOUND'] == 1
    assert ops.CONF_MODES == {'moderated': 0, 'bound': 1}
    L = _lib.lib()
    assert L.tipk_abi_version() == 30
    assert ops.distmult_pair_conf_topk_supported(645, 16, 1097, 10) and ops.distmult_pair_conf_topk_supported(10, 32, 1, 0)
    for n, dim, r, k in ((10, 40, 5, 1), (10, 6, 5, 1), (10, 16, 5, 129), (10, 16, 5, -1), (10, 16, 0, 1), (50000, 16, 5, 1)):
        assert not ops.distmult_pair_conf_topk_supported(n, dim, r, k), (n, dim, r, k)
    # argument checks come before anything touches a device: EINVAL = the status of a NULL pointer with work to do
    assert L.tipk_spd_factor(None, None, 0, 16, None, None, None, None) == 0
    assert L.tipk_spd_factor(None, None, 1, 16, None, None, None, None) != 0
    assert L.tipk_spd_factor(None, None, 0, 0, None, None, None, None) != 0
    assert L.tipk_distmult_pair_conf_topk(None, 5, 16, None, None, 3, None, None, 0, None, None, None, 0, 5, 0, 0.0, None, None,
                                          None, None, None, None, None) == 0
    for mode, c in ((2, 0.0), (1, float('inf')), (1, float('nan'))):
        assert L.tipk_distmult_pair_conf_topk(None, 5, 16, None, None, 3, None, None, 0, None, None, None, 0, 5, mode, c, None,
                                              None, None, None, None, None, None) != 0


def test_tip_result_types():
    assert DecoderPosterior._fields == ('weight', 'factor', 'n_pairs', 'relation', 'known')
    assert ConfidentSideEffects._fields == ('probability', 'mean_probability', 'logit', 'std', 'relation', 'dense_logit', 'dense_std')
    assert 'DecoderPosterior' in layers.__all__ and 'ConfidentSideEffects' in layers.__all__
    w64 = torch.tril(torch.randn((2, 4, 4), generator=torch.Generator().manual_seed(1), dtype=torch.float64)).float()
    post = DecoderPosterior(torch.zeros(2, 4), w64.transpose(1, 2).contiguous(), torch.ones(2), torch.arange(2), None)
    assert torch.allclose(post.covariance(), w64.transpose(1, 2) @ w64) and torch.equal(post.covariance(), post.covariance().transpose(1, 2))


def test_tip_decoder_posterior_refusals():
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    dec = types.SimpleNamespace(in_dim=16)
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.decoder_posterior(types.SimpleNamespace(decoder_kind='nn', shard=None, data=data, decoder=dec), [[(0, 1)]], l2=-1)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.decoder_posterior(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data, decoder=dec), [[(0, 1)]], l2=-1)
    self = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=dec)
    w = torch.zeros(1, 16)
    for kw in ({'l2': 0.0}, {'l2': -1e-3}, {'l2': float('nan')}, {'neg_weight': 0.0}, {'neg_weight': -1.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TIP.decoder_posterior(self, [[(0, 1)]], w, **kw)
    for bad in ([[(0, 10)]], [[(-1, 2)]]):
        with pytest.raises(ValueError, match='out of range'):
            TIP.decoder_posterior(self, bad, w)
    new = types.SimpleNamespace(z=torch.zeros(2, 16))
    with pytest.raises(ValueError, match='out of range'):
        TIP.decoder_posterior(self, [[(0, 12)]], w, new=new)                 # two new drugs: ids up to 11
    for weight in (torch.zeros(2, 16), torch.zeros(16), torch.zeros(1, 8), None):
        with pytest.raises(ValueError, match='weight'):
            TIP.decoder_posterior(self, [[(0, 1)]], weight)
    with pytest.raises(ValueError, match='out of range'):
        TIP.decoder_posterior(self, relations=[5])
    with pytest.raises(ValueError, match='relations'):
        TIP.decoder_posterior(self, [[(0, 1)]], w, relations=[0])
    with pytest.raises(ValueError, match='weight'):
        TIP.decoder_posterior(self, weight=w)
    with pytest.raises(ValueError, match='at least one recorded pair'):
        TIP.decoder_posterior(self, [[(0, 1)], []], torch.zeros(2, 16))
    wide = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data, decoder=types.SimpleNamespace(in_dim=40))
    with pytest.raises(NotImplementedError, match='4m'):
        TIP.decoder_posterior(wide, [[(0, 1)]], torch.zeros(1, 40))


def test_tip_side_effects_confidence_refusals():
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    pairs = torch.tensor([[0], [1]])
    model_post = DecoderPosterior(torch.zeros(5, 16), torch.zeros(5, 16, 16), torch.ones(5), torch.arange(5), None)
    given_post = model_post._replace(known=(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64),
                                            torch.zeros(0, dtype=torch.int32)))
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.side_effects_confidence(types.SimpleNamespace(decoder_kind='nn', shard=None, data=data), pairs, model_post, k=-1)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.side_effects_confidence(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data), pairs, model_post, k=-1)
    self = types.SimpleNamespace(decoder_kind='distmult', shard=None, data=data)
    for kw in ({'rank_by': 'mean'}, {'rank_by': None}, {'z_score': float('inf')}, {'z_score': float('nan')}, {'k': -1}, {'k': 129}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TIP.side_effects_confidence(self, pairs, model_post, **kw)
    with pytest.raises(ValueError, match='exclude'):
        TIP.side_effects_confidence(self, pairs, model_post, exclude='test')
    with pytest.raises(ValueError, match='exclude'):
        TIP.side_effects_confidence(self, pairs, given_post, exclude='train')
    for bad in (torch.tensor([[0], [10]]), torch.tensor([[-1], [2]])):
        with pytest.raises(ValueError, match='out of range'):
            TIP.side_effects_confidence(self, bad, model_post)
    with pytest.raises(ValueError, match='pairs'):
        TIP.side_effects_confidence(self, torch.zeros(3, 2, dtype=torch.int64), model_post)
    new = types.SimpleNamespace(z=torch.zeros(2, 16))
    with pytest.raises(ValueError, match='out of range'):
        TIP.side_effects_confidence(self, torch.tensor([[0], [12]]), model_post, new=new)
    wide = DecoderPosterior(torch.zeros(5, 40), torch.zeros(5, 40, 40), torch.ones(5), torch.arange(5), None)
    with pytest.raises(NotImplementedError, match='4p'):
        TIP.side_effects_confidence(self, pairs, wide)
