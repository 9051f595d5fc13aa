"""CPU tests of the partner sum (include/tipk.h section 4l): the symbols, the `_supported` predicates, the route query and its
option, argument validation of both C entries (every refusal happens before anything touches a device, so bogus device
pointers are safe here), the fp64 spec and the acceptance rule (tests/partner_sum_spec.py) against a plain triple loop and
planted mistakes, the mirroring helper of the ops, and the refusals of `TIP.drug_profile`."""
import ctypes
import math
import types

import pytest
import torch

import partner_sum_cases as cases
from partner_rank_cases import known_from_dict
from partner_sum_spec import C_PROFILE, check_partner_sum, check_top, expected_top, loop_partner_sum, spec_partner_sum
from tip_amd import _lib, ops
from tip_amd.layers import TIP, DrugProfile

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch
SYMBOLS = ('tipk_distmult_partner_sum', 'tipk_pair_table_partner_sum', 'tipk_distmult_partner_sum_supported',
           'tipk_pair_table_partner_sum_supported', 'tipk_distmult_partner_sum_lds_route')


def _dm(n=10, dim=16, n_rel=3, n_q=4, n_sel=3, k=2, z=FAKE, w=FAKE, q=FAKE, rel=None, pw=None, keys=None, kptr=None,
        out_sum=FAKE, out_cnt=FAKE, top_v=FAKE, top_p=FAKE):
    return _lib.lib().tipk_distmult_partner_sum(z, n, dim, w, n_rel, q, n_q, rel, n_sel, pw, keys, kptr, k, out_sum, out_cnt,
                                                top_v, top_p, None)


def _tb(n=10, n_rel=3, ld=None, n_q=4, n_sel=3, k=2, s1=FAKE, s2=FAKE, q=FAKE, rel=None, pw=None, keys=None, kptr=None,
        out_sum=FAKE, out_cnt=FAKE, top_v=FAKE, top_p=FAKE):
    return _lib.lib().tipk_pair_table_partner_sum(s1, s2, n if ld is None else ld, n, n_rel, q, n_q, rel, n_sel, pw, keys,
                                                  kptr, k, out_sum, out_cnt, top_v, top_p, None)


def test_symbols_and_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30            # purely additive
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    dm, tb = L.tipk_distmult_partner_sum_supported, L.tipk_pair_table_partner_sum_supported
    rank_dm, rank_tb = L.tipk_distmult_partner_rank_supported, L.tipk_pair_table_partner_rank_supported
    for n in (0, 1, 645, 46340, 46341):                                    # the range of 4g, point for point
        for n_rel in (0, 1, 1097, 65536, 65537):
            assert tb(n, n_rel) == rank_tb(n, n_rel), (n, n_rel)
            for dim in (0, 2, 4, 6, 16, 20, 256, 260):
                assert dm(n, dim, n_rel) == rank_dm(n, dim, n_rel), (n, dim, n_rel)
    assert dm(645, 16, 1097) == 1 and tb(645, 1097) == 1 and dm(46341, 16, 4) == 0 and dm(645, 6, 4) == 0


def test_route_query_and_option():
    L = _lib.lib()
    route = L.tipk_distmult_partner_sum_lds_route
    assert _lib.get_option('partner_sum_global') == 0
    assert route(645, 16) == 1                                           # BioSNAP: 645 rows of 80 B beside the waves' state
    assert route(2600, 16) == 0                                          # 2 600 rows of 80 B do not fit
    assert route(700, 16) == 1 and route(700, 32) == 1 and route(645, 6) == 0
    _lib.set_option('partner_sum_global', 1)
    try:
        assert _lib.get_option('partner_sum_global') == 1
        assert route(645, 16) == 0
        assert _lib.get_option('partner_rank_global') == 0 and L.tipk_distmult_partner_rank_lds_route(645, 16) == 1
    finally:
        _lib.set_option('partner_sum_global', 0)
    assert route(645, 16) == 1 and _lib.get_option('partner_sum_global') == 0


def test_status_order():
    for call in (_dm, _tb):
        assert call(k=-1) == EINVAL and call(k=129) == EINVAL              # k outside 0..128 is an argument error
        assert call(n_q=-1) == EINVAL and call(n_sel=-1) == EINVAL
        assert call(n=0) == EINVAL and call(n=-5) == EINVAL and call(n_rel=0) == EINVAL
        assert call(n_sel=2) == EINVAL                                     # no rel_ids: the columns are the n_rel relations
        assert call(n_sel=2, rel=FAKE, n_q=0) == 0
        assert call(keys=FAKE) == EINVAL and call(kptr=FAKE) == EINVAL     # keys without offsets and the reverse
        assert call(q=None) == EINVAL and call(out_sum=None) == EINVAL and call(out_cnt=None) == EINVAL
        assert call(top_v=None) == EINVAL and call(top_p=None) == EINVAL   # top outputs missing with k > 0
        assert call(k=0, top_v=None, top_p=None, n=46341) == EUNSUPPORTED  # ... and not missed with k = 0
        assert call(k=-1, n=46341) == EINVAL and call(k=129, n_rel=65537) == EINVAL   # argument errors come first
        assert call(n=46341) == EUNSUPPORTED and call(n_rel=65537, n_sel=65537) == EUNSUPPORTED
        assert call(n_q=0) == 0 and call(n_sel=0, rel=FAKE) == 0           # nothing to do, nothing launched
        assert call(n_q=0, q=None, out_sum=None, out_cnt=None, top_v=None, top_p=None) == 0
        assert call(n_q=0, keys=FAKE, kptr=FAKE, pw=FAKE) == 0
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL and _tb(s1=None) == EINVAL and _tb(s2=None) == EINVAL
    assert _dm(dim=0) == EINVAL and _dm(dim=-4) == EINVAL
    assert _tb(ld=9) == EINVAL                                            # row stride below n_nodes
    assert _dm(dim=2) == EUNSUPPORTED and _dm(dim=6) == EUNSUPPORTED and _dm(dim=260) == EUNSUPPORTED
    assert _dm(z=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED          # z must be 16-byte aligned
    assert _dm(n_q=0, z=None, w=None) == 0 and _tb(n_q=0, s1=None, s2=None) == 0


def test_ops_refuse_cpu_and_half_tensors():
    q = torch.tensor([0, 1])
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_partner_sum(torch.ones(5, 4), torch.ones(2, 4), q, 2)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.pair_table_partner_sum(torch.ones(3, 5), torch.ones(3, 5), q, 2)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.distmult_partner_sum(torch.ones(5, 4, dtype=torch.float16), torch.ones(2, 4), q, 2)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.pair_table_partner_sum(torch.ones(3, 5, dtype=torch.float64), torch.ones(3, 5), q, 2)


# ------------------------------------------------------------------ the spec and the rule
def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_spec_by_hand():
    """The line graph: z = (1, 2, 3), w = 1: the logits of (0,1), (0,2), (1,2) are 2, 3 and 6."""
    m = ('distmult', torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[1.0]]))
    t = spec_partner_sum(m, torch.tensor([0, 1, 2, 3, -1]))
    assert t['E64'][:3, 0].tolist() == pytest.approx([_sig(2) + _sig(3), _sig(2) + _sig(6), _sig(3) + _sig(6)], rel=1e-15)
    assert t['count'][:, 0].tolist() == [2, 2, 2, 0, 0] and bool(torch.isnan(t['E64'][3:]).all())
    t = spec_partner_sum(m, torch.tensor([0]), torch.tensor([0, 1, 0, -1]), torch.tensor([5.0, 0.5, 0.0]))
    assert t['E64'][0, [0, 2]].tolist() == pytest.approx([0.5 * _sig(2)] * 2, rel=1e-15)
    assert t['count'][0].tolist() == [1, 0, 1, 0] and bool(torch.isnan(t['E64'][0, [1, 3]]).all())
    fwd = known_from_dict({0: [(0, 1)]}, 3, 1)                            # only the forward key is looked up
    t = spec_partner_sum(m, torch.tensor([0, 1]), known=fwd)
    assert t['E64'][:, 0].tolist() == pytest.approx([_sig(3), _sig(2) + _sig(6)], rel=1e-15) and t['count'][:, 0].tolist() == [1, 2]
    every = known_from_dict({0: [(0, 1), (0, 2), (0, 0)]}, 3, 1)
    t = spec_partner_sum(m, torch.tensor([0]), known=every)
    assert float(t['E64'][0, 0]) == 0.0 and int(t['count'][0, 0]) == 0   # no candidates: exactly 0
    nan = ('distmult', torch.tensor([[1.0], [float('nan')], [3.0]]), torch.tensor([[1.0]]))
    t = spec_partner_sum(nan, torch.tensor([0, 0, 0]), torch.tensor([0]))
    assert bool(torch.isnan(t['E64']).all())
    t = spec_partner_sum(nan, torch.tensor([0]), partner_w=torch.tensor([1.0, 0.0, 1.0]))
    assert float(t['E64'][0, 0]) == pytest.approx(_sig(3), rel=1e-15)    # weight 0: skipped, its NaN does not count
    t = spec_partner_sum(nan, torch.tensor([0]), known=fwd)
    assert float(t['E64'][0, 0]) == pytest.approx(_sig(3), rel=1e-15)    # recorded: skipped as well
    inf = ('table', torch.tensor([[0.0, 1.0, 0.0]]), torch.tensor([[0.0, float('inf'), float('-inf')]]))
    t = spec_partner_sum(inf, torch.tensor([0]), partner_w=torch.tensor([1.0, 2.5, 7.0]))
    assert float(t['E64'][0, 0]) == 2.5 and float(t['T_tau'][0, 0]) == 0.0    # +inf: exactly the weight, -inf: exactly 0


@pytest.mark.parametrize('kind', cases.KINDS)
def test_spec_matches_triple_loop(kind):
    for n, dim, col_mode, w_mode in ((1, 4, 'all', 'none'), (2, 4, 'repeats', 'zeros'), (9, 8, 'subset', 'zeros'),
                                     (12, 4, 'repeats', 'none'), (12, 4, 'all', 'all_zero')):
        c = cases.small_case(kind, n, dim, col_mode, w_mode, n_q=7, n_rel=4)
        t = spec_partner_sum(c['model'], c['q_drug'], c['rel_ids'], c['partner_w'], c['known'])
        E, count = loop_partner_sum(c['model'], c['q_drug'], c['rel_ids'], c['partner_w'], c['known'])
        assert torch.equal(count, t['count']) and torch.equal(torch.isnan(E), torch.isnan(t['E64']))
        ok = ~torch.isnan(E)
        assert bool(((E - t['E64']).abs()[ok] <= 1e-13 * (1 + E[ok].abs())).all())
    # one-direction lists: the loop and the spec drop the listed direction only
    c = cases.known_case(kind, 'one_way', n=14)
    t = spec_partner_sum(c['model'], c['q_drug'], None, None, c['known'])
    E, count = loop_partner_sum(c['model'], c['q_drug'], None, None, c['known'])
    assert torch.equal(count, t['count']) and bool(((E - t['E64']).abs() <= 1e-13 * (1 + E.abs())).all())
    assert int(count.min()) < 13 and not torch.equal(count, loop_partner_sum(c['model'], c['q_drug'], None, None, c['known'],
                                                                               reverse_only=True)[1])


def _as_result(E, count, k):
    S = E.float()
    top_v, top_p = expected_top(S, k)
    return S, count.int(), top_v, top_p.int()


@pytest.mark.parametrize('kind', cases.KINDS)
def test_rule_rejects_planted_mistakes(kind):
    """The rule accepts the contract's own loop rounded to fp32 and rejects: u counted as its own partner, a weight of 0
    multiplied instead of skipped, the reverse key looked up instead of the forward one, top-k ties broken descending."""
    c = cases.known_case(kind, 'one_way', n=20)
    g = torch.Generator().manual_seed(3)
    pw = cases.weights(20, 'zeros', g)
    rel = torch.tensor([0, 1, 2, 3, 4, 2, 2, 0])                           # repeated columns: exact ties
    z = c['model'][1].clone()
    nan_row = int(torch.nonzero(pw == 0)[0])
    if kind == 'distmult':
        z[nan_row] = float('nan')                                         # a NaN partner with weight 0
        model = (kind, z, c['model'][2])
    else:
        s2 = c['model'][2].clone()
        s2[:, nan_row] = float('nan')
        model = (kind, c['model'][1], s2)
    q = torch.tensor([0, 7, 7, 19, 20, 1 if nan_row != 1 else 2])
    k = 5
    args = dict(rel_ids=rel, partner_w=pw, known=c['known'])
    good = _as_result(*loop_partner_sum(model, q, **args), k)
    t = check_partner_sum(model, q, k, good, **args)
    assert t['observed_c'] <= 1.0                                         # fp64 rounded once to fp32
    check_partner_sum(model, q, 0, good[:2] + (None, None), **args)
    for flag, match in (('count_self', 'count'), ('reverse_only', 'count'), ('multiply_zero', 'NaN placement')):
        bad = _as_result(*loop_partner_sum(model, q, **{flag: True}, **args), k)
        with pytest.raises(AssertionError, match=match):
            check_partner_sum(model, q, k, bad, **args)
    # the same mistakes with the counts put right: the sums alone give them away
    for flag in ('count_self', 'reverse_only'):
        bad = _as_result(loop_partner_sum(model, q, **{flag: True}, **args)[0], good[1], k)
        with pytest.raises(AssertionError, match='sum off fp64'):
            check_partner_sum(model, q, k, bad, **args)
    # ties broken descending by position: columns 2, 5 and 6 are the same relation
    S = good[0]
    assert bool((S[0, 2] == S[0, 5]) & (S[0, 5] == S[0, 6]))
    top_p = good[3].clone()
    for row in range(top_p.shape[0]):
        hit = [i for i, p in enumerate(top_p[row].tolist()) if p in (2, 5, 6)]
        if len(hit) >= 2:
            top_p[row, hit] = top_p[row, hit].flip(0)
    assert not torch.equal(top_p, good[3])
    with pytest.raises(AssertionError, match='selection'):
        check_partner_sum(model, q, k, (good[0], good[1], good[2], top_p), **args)
    vals = good[2].clone()
    vals[0, 0] = torch.nextafter(vals[0, 0], torch.tensor(0.0))
    with pytest.raises(AssertionError, match='bit-equal'):
        check_top(S, k, vals, good[3])
    assert C_PROFILE >= 4.0


def test_expected_top_by_hand():
    nan, inf = float('nan'), float('inf')
    s = torch.tensor([[3.0, nan, 1.0, 1.0, 0.5], [nan, nan, nan, nan, nan], [-0.0, 0.0, 2.0, nan, -inf]])
    vals, pos = expected_top(s, 3)
    assert pos.tolist() == [[0, 2, 3], [-1, -1, -1], [2, 0, 1]]           # ties (and -0 == +0) by position
    assert vals[1].tolist() == [-inf] * 3 and math.copysign(1, float(vals[2, 1])) == -1.0
    vals, pos = expected_top(s, 7)
    assert pos[0].tolist() == [0, 2, 3, 4, -1, -1, -1] and pos[2].tolist() == [2, 0, 1, 4, -1, -1, -1]
    assert vals[2, 3] == -inf and vals[0, 4:].tolist() == [-inf] * 3
    check_top(s, 3, *expected_top(s, 3))
    assert expected_top(torch.zeros(2, 0), 2)[1].tolist() == [[-1, -1], [-1, -1]]


# ------------------------------------------------------------------ the mirroring helper
def test_symmetric_known():
    n, n_rel = 6, 3
    one_way = known_from_dict({0: [(0, 1), (2, 5), (3, 3)], 2: [(4, 1), (1, 4), (5, 0)]}, n, n_rel)
    both = ops.symmetric_known(one_way, n)
    want = known_from_dict({0: [(0, 1), (1, 0), (2, 5), (5, 2), (3, 3)], 2: [(4, 1), (1, 4), (5, 0), (0, 5)]}, n, n_rel)
    assert torch.equal(both[0], want[0]) and torch.equal(both[1], want[1])
    assert both[0].dtype == torch.int64 and both[1].dtype == torch.int64
    assert ops.symmetric_known(both, n) is both                           # already symmetric: the input itself
    assert ops.symmetric_known(both, n) is both                           # ... from the cache as well
    again = ops.symmetric_known(one_way, n)                               # cached by identity
    assert again[0] is both[0] and again[1] is both[1]
    dup = (torch.tensor([1, 1, 6, 30], dtype=torch.int64), torch.tensor([0, 3, 3, 4], dtype=torch.int64))   # (0,1) twice, (1,0); (5,0)
    out = ops.symmetric_known(dup, n)
    assert out[0].tolist() == [1, 6, 5, 30] and out[1].tolist() == [0, 2, 2, 4]
    assert ops.symmetric_known(None, n) is None
    empty = (torch.zeros(0, dtype=torch.int64), torch.zeros(n_rel + 1, dtype=torch.int64))
    assert ops.symmetric_known(empty, n) is empty
    only_self = known_from_dict({1: [(2, 2), (4, 4)]}, n, n_rel)
    assert ops.symmetric_known(only_self, n) is only_self


# ------------------------------------------------------------------ TIP.drug_profile
def test_tip_drug_profile_refusals():
    assert DrugProfile._fields == ('expected', 'candidates', 'top_expected', 'top_relation')
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.drug_profile(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data), [0, 1], exclude='bad')
    new = types.SimpleNamespace(z=torch.zeros(2, 4))
    for kind in ('distmult', 'nn'):
        self = types.SimpleNamespace(decoder_kind=kind, shard=None, data=data)
        for bad in ('test', 'none', 0):
            with pytest.raises(ValueError, match='exclude'):
                TIP.drug_profile(self, [0, 99], exclude=bad)                # the mode is refused before the ids
        for bad in (-1, 129):
            with pytest.raises(ValueError, match='k must'):
                TIP.drug_profile(self, [0, 1], k=bad)
        for bad in ([0, 10], [-1], torch.tensor([3, 11])):
            with pytest.raises(ValueError, match='out of range'):
                TIP.drug_profile(self, bad)
        with pytest.raises(ValueError, match='out of range'):
            TIP.drug_profile(self, [0, 12], new=new)                        # two new drugs: ids up to 11
        with pytest.raises(ValueError, match='drugs'):
            TIP.drug_profile(self, [0.5])
        for bad in ([5], [-1, 0]):
            with pytest.raises(ValueError, match='side-effect id out of range'):
                TIP.drug_profile(self, [0, 1], relations=bad)
        for w in ([1.0] * 9, [1.0] * 11, [[1.0] * 10], [1] * 9 + [-0.5], [1] * 9 + [float('nan')], [1] * 9 + [float('inf')],
                  'heavy'):
            with pytest.raises(ValueError, match='partner_weights'):
                TIP.drug_profile(self, [0, 1], partner_weights=w)
        with pytest.raises(ValueError, match='partner_weights'):            # one per TRAINING drug, also with new ones
            TIP.drug_profile(self, [0, 11], partner_weights=[1.0] * 12, new=new)
