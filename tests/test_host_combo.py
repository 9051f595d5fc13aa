"""CPU tests of the combination burden (include/tipk.h section 4n): the symbols, the `_supported` predicates, the limit and
workspace queries and the two options, argument validation of both C entries (every refusal happens before anything touches
a device, so bogus device pointers are safe here), the host plan and normalisation and the refusals of
`TIP.combination_risk`, the fp64 spec and the acceptance rule (tests/combo_spec.py) on hand-worked cases, and the conditions
the unsaturated inputs of tests/combo_cases.py must meet."""
import ctypes
import itertools
import math
import types

import pytest
import torch

import combo_cases as cases
from combo_spec import (C_COMBO, check_combo_burden, combination_count, combo_ptr, query_legal, query_lists,
                        spec_combo_burden)
from addon_spec import check_selection, expected_selection
from pair_topk_spec import known_from_dict
from tip_amd import _lib, layers, ops
from tip_amd.layers import TIP, CombinationRisk, normalize_combination_queries

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _lists(n_q, n_fix, n_alt, n_slots, n_comb, n_rows, fix, fptr, alt, aptr, sptr, cptr, rptr):
    return (fix, fptr, n_fix, alt, aptr, n_alt, sptr, n_slots, cptr, rptr, n_q, n_comb, n_rows)


def _dm(n=10, dim=16, n_rel=3, n_q=4, n_fix=5, n_alt=6, n_slots=3, n_comb=20, n_rows=30, k=5, agg=0, keys=None, kptr=None,
        krel=None, n_known=0, z=FAKE, w=FAKE, fix=FAKE, fptr=FAKE, alt=FAKE, aptr=FAKE, sptr=FAKE, cptr=FAKE, rptr=FAKE,
        wts=None, out_b=FAKE, best_b=FAKE, best_c=FAKE, ws=FAKE):
    return _lib.lib().tipk_distmult_combo_burden(
        z, n, dim, w, n_rel, *_lists(n_q, n_fix, n_alt, n_slots, n_comb, n_rows, fix, fptr, alt, aptr, sptr, cptr, rptr), wts,
        keys, kptr, krel, n_known, agg, k, out_b, best_b, best_c, ws, None)


def _tb(n=10, n_rel=3, ld=None, n_q=4, n_fix=5, n_alt=6, n_slots=3, n_comb=20, n_rows=30, k=5, agg=0, keys=None, kptr=None,
        krel=None, n_known=0, s1=FAKE, s2=FAKE, fix=FAKE, fptr=FAKE, alt=FAKE, aptr=FAKE, sptr=FAKE, cptr=FAKE, rptr=FAKE,
        wts=None, out_b=FAKE, best_b=FAKE, best_c=FAKE, ws=FAKE):
    return _lib.lib().tipk_pair_table_combo_burden(
        s1, s2, n_rel if ld is None else ld, n, n_rel,
        *_lists(n_q, n_fix, n_alt, n_slots, n_comb, n_rows, fix, fptr, alt, aptr, sptr, cptr, rptr), wts, keys, kptr, krel,
        n_known, agg, k, out_b, best_b, best_c, ws, None)


def _limits():
    return ops.combo_limits()


def test_symbols_limits_and_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30          # the section is purely additive
    for name in ('tipk_combo_max_slots', 'tipk_combo_max_alternatives', 'tipk_combo_max_combinations',
                 'tipk_distmult_combo_burden_supported', 'tipk_distmult_combo_burden_workspace_bytes',
                 'tipk_distmult_combo_burden', 'tipk_pair_table_combo_burden_supported',
                 'tipk_pair_table_combo_burden_workspace_bytes', 'tipk_pair_table_combo_burden'):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    lim = _limits()
    assert lim == (L.tipk_addon_max_context(), L.tipk_combo_max_slots(), L.tipk_combo_max_alternatives(),
                   L.tipk_combo_max_combinations())
    assert lim == (64, 10, 64, 1 << 24)          # ten slots, not eight: de-prescribing a 10-drug list is one query
    assert 1 + lim.max_slots * (lim.max_slots + 1) // 2 <= 64            # a lane per term of the level order
    dm, tb = L.tipk_distmult_combo_burden_supported, L.tipk_pair_table_combo_burden_supported
    assert dm(645, 4, 1097, 10) == 1 and dm(645, 16, 1097, 0) == 1 and dm(645, 256, 1097, 128) == 1
    for dim in (0, 2, 6, 260):
        assert dm(645, dim, 1097, 10) == 0
    assert dm(645, 16, 1097, -1) == 0 and dm(645, 16, 1097, 129) == 0
    assert dm(645, 16, 0, 4) == 0 and dm(645, 16, 65537, 4) == 0 and dm(0, 16, 4, 4) == 0 and dm(46341, 16, 4, 4) == 0
    assert tb(1, 1, 0) == 1 and tb(46340, 65536, 128) == 1
    assert tb(0, 4, 4) == 0 and tb(46341, 4, 4) == 0 and tb(645, 0, 4) == 0 and tb(645, 65537, 4) == 0 and tb(645, 4, 129) == 0
    wd, wt = L.tipk_distmult_combo_burden_workspace_bytes, L.tipk_pair_table_combo_burden_workspace_bytes
    # a row is n_rel floats rounded up to 16 bytes: 1 097 -> 1 100
    assert wd(645, 16, 1097, 0, 10) == 0 and wd(645, 16, 1097, 3, 10) == 3 * 1100 * 4 and wt(645, 1097, 3, 10) == 3 * 1100 * 4
    assert wd(645, 16, 64, 5, 0) == 5 * 64 * 4 and wt(645, 1, 5, 0) == 5 * 4 * 4
    assert wd(645, 6, 4, 1, 4) == -1 and wd(46341, 16, 4, 1, 4) == -1 and wd(645, 16, 4, -1, 4) == -1 and wd(645, 16, 4, 1, 129) == -1
    assert wt(0, 4, 1, 4) == -1 and wt(645, 4, -1, 4) == -1
    # the full table of one query at BioSNAP size: 1 + 64 + 64 * 64 rows at most (in fact fewer: pairs of one slot have none)
    assert wd(645, 16, 1097, 1 + 64 + 64 * 64, 10) == 4161 * 4400


def test_options():
    for name in ('combo_no_prefix', 'combo_run'):
        assert _lib.get_option(name) == 0
        _lib.set_option(name, 1)
        try:
            assert _lib.get_option(name) == 1
            assert _lib.get_option('addon_global') == 0
        finally:
            _lib.set_option(name, 0)
        assert _lib.get_option(name) == 0


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(k=-1) == EINVAL
        for size in ('n_q', 'n_fix', 'n_alt', 'n_slots', 'n_comb', 'n_rows', 'n_known'):
            assert call(**{size: -1}) == EINVAL, size
        assert call(n=0) == EINVAL and call(n=-5) == EINVAL and call(n_rel=0) == EINVAL
        assert call(agg=2) == EINVAL and call(agg=-1) == EINVAL           # unknown aggregate
        assert call(keys=FAKE, n_known=2) == EINVAL                       # known arrays given only in part
        assert call(keys=FAKE, kptr=FAKE, n_known=2) == EINVAL
        assert call(krel=FAKE) == EINVAL
        for ptr in ('fptr', 'aptr', 'sptr', 'cptr', 'rptr', 'fix', 'alt', 'out_b', 'ws', 'best_b', 'best_c'):
            assert call(**{ptr: None}) == EINVAL, ptr
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(s2=None) == EINVAL
    assert _dm(dim=0) == EINVAL and _dm(dim=-4) == EINVAL
    assert _tb(ld=2) == EINVAL                                           # row stride below n_rel
    assert _dm(k=-1, dim=6) == EINVAL                                    # argument errors come before shape limits
    assert _dm(agg=7, n=46341) == EINVAL and _tb(k=-1, n=46341) == EINVAL


def test_unsupported_shapes_and_empty_calls():
    assert _dm(k=129) == EUNSUPPORTED and _tb(k=129) == EUNSUPPORTED
    assert _dm(dim=2) == EUNSUPPORTED and _dm(dim=6) == EUNSUPPORTED and _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED and _tb(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED and _tb(n_rel=65537) == EUNSUPPORTED
    assert _dm(w=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # rel_w must be 16-byte aligned
    assert _dm(ws=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED and _tb(ws=ctypes.c_void_p((1 << 20) + 8)) == EUNSUPPORTED
    assert _dm(n_comb=1 << 31) == EUNSUPPORTED and _tb(n_comb=1 << 31) == EUNSUPPORTED   # combinations per call < 2^31
    for agg in (0, 1):
        assert _dm(n_q=0, agg=agg) == 0 and _tb(n_q=0, agg=agg) == 0     # nothing to do, nothing launched
    none = dict(fix=None, fptr=None, alt=None, aptr=None, sptr=None, cptr=None, rptr=None, out_b=None, best_b=None, best_c=None,
                ws=None)
    assert _dm(n_q=0, z=None, w=None, **none) == 0 and _tb(n_q=0, s1=None, s2=None, **none) == 0
    assert _dm(n_q=0, keys=FAKE, kptr=FAKE, krel=FAKE, n_known=3) == 0


def test_ops_refuse_cpu_tensors_bad_plans_and_bad_aggregate():
    plan = ops.combo_plan([0, 1], [0, 2], [2, 3], [0, 2], [0, 1], 'cpu')
    assert (plan.n_q, plan.n_fix, plan.n_alt, plan.n_slots, plan.n_comb, plan.n_rows) == (1, 2, 2, 1, 2, 3)
    with pytest.raises(_lib.TipkError):
        ops.distmult_combo_burden(torch.ones(5, 4), torch.ones(2, 4), plan, 2, 'max')
    with pytest.raises(_lib.TipkError):
        ops.pair_table_combo_burden(torch.ones(5, 3), torch.ones(5, 3), plan, 2, 'noisy_or')
    with pytest.raises(_lib.TipkError, match='1-d int'):
        ops.combo_plan([0.5], [0, 1], [], [0], [0, 0], 'cpu')
    with pytest.raises(_lib.TipkError, match='entries'):
        ops.combo_plan([], [0, 0, 0], [], [0], [0, 0], 'cpu')


def test_combo_plan_counts_match_the_spec():
    """The plan's offsets are the convention of the spec: prod A_s entries and 1 + sum A + sum_{s<t} A_s A_t rows for a
    query whose structure is legal, one NaN entry and no row otherwise."""
    lim = _limits()
    queries = [([1, 2], [[3, 4], [5, -1, 6]]), ([], []), ([7], [[8]]), ([1], [[2], []]), ([], [[1]] * 11),
               ([], [list(range(33)), list(range(33, 65))]), ([0, 0, 99], [[1, 2, 3, 4]]), ([], [[1, 2]] * 8)]
    plan = ops.combo_plan(*query_lists(queries), 'cpu')
    assert plan.host_comb_ptr.tolist() == combo_ptr(queries, 70, lim).tolist() == [0, 6, 7, 8, 9, 10, 11, 15, 15 + 256]
    rows = [1 + 5 + 6, 1, 1 + 1, 0, 0, 0, 1 + 4, 1 + 16 + 4 * 28]
    assert (plan.host_row_ptr[1:] - plan.host_row_ptr[:-1]).tolist() == rows
    assert [query_legal(f, s, 70, lim) for f, s in queries] == [(True, True), (True, True), (True, True), (False, False),
                                                                 (False, False), (False, False), (False, True), (True, True)]
    assert combination_count([], [list(range(64))] * 4, 70, lim) == 1    # 64 alternatives at most in all slots


# ------------------------------------------------------------------ the spec and the rule, by hand
def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def _sp(x):
    return math.log1p(math.exp(x))


def _line():
    """The line graph: z = (1, 2, 3), w = 1, so the logits of (0,1), (0,2), (1,2) are 2, 3 and 6."""
    return ('distmult', torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[1.0]]))


def test_spec_by_hand():
    m, lim = _line(), _limits()
    B = lambda q, agg, known=None, w=None: spec_combo_burden(m, [q], agg, lim, w, known)['B64'].tolist()
    # no slots: the plain regimen burden of the fixed list; 0 or 1 drugs: exactly +0
    assert B(([0, 1, 2], []), 'noisy_or') == pytest.approx([1 - math.exp(-(_sp(2) + _sp(3) + _sp(6)))], rel=1e-14)
    assert B(([0, 1, 2], []), 'max') == pytest.approx([_sig(6)], rel=1e-14)
    assert B(([], []), 'noisy_or') == [0.0] and B(([1], []), 'max') == [0.0]
    # fixed 0, slot (1, 2, -1): pairs (0,1) | (0,2) | none
    assert B(([0], [[1, 2, -1]]), 'max') == pytest.approx([_sig(2), _sig(3), 0.0], rel=1e-14)
    # two slots, last fastest: (1,2) -> 6; (1,-1) -> 0; (-1,2) -> 0; (-1,-1) -> 0
    assert B(([], [[1, -1], [2, -1]]), 'max') == pytest.approx([_sig(6), 0.0, 0.0, 0.0], rel=1e-14)
    # fixed 0 and two slots: all three pairs under noisy-or; the repeated and the fixed drug are NaN
    got = B(([0], [[1, 2], [2, 0]]), 'noisy_or')
    assert got[0] == pytest.approx(1 - math.exp(-(_sp(2) + _sp(3) + _sp(6))), rel=1e-14)
    assert math.isnan(got[1]) and math.isnan(got[2]) and math.isnan(got[3])          # (1,0): 0 is fixed; (2,2); (2,0)
    # weights and the known filter, in either direction
    known = known_from_dict({(2, 1): [0]}, 3)
    assert B(([0], [[1], [2]]), 'noisy_or', known, [2.0]) == pytest.approx([2 * (1 - math.exp(-(_sp(2) + _sp(3))))], rel=1e-14)
    assert B(([], [[1], [2]]), 'max', known) == [0.0]
    # illegal queries: every entry NaN; a structural one owns one entry
    for q, count in ((([3], [[1, 2]]), 2), (([0, 0], [[1, 2]]), 2), (([0], [[1, 5]]), 2), (([0], [[1, 2], []]), 1),
                     (([0], [[1, -2]]), 2)):
        got = B(q, 'max')
        assert len(got) == count and all(math.isnan(x) for x in got), q
    # a NaN logit of a triple that is not known: NaN; known: it does not count
    nan_m = ('distmult', torch.tensor([[1.0], [float('nan')], [3.0]]), torch.tensor([[1.0]]))
    t = spec_combo_burden(nan_m, [([0], [[1, 2]])], 'max', lim, [0.0], None)
    assert math.isnan(float(t['B64'][0])) and float(t['B64'][1]) == 0.0
    t = spec_combo_burden(nan_m, [([0], [[1, 2]])], 'max', lim, None, known_from_dict({(0, 1): [0]}, 3))
    assert float(t['B64'][0]) == 0.0 and float(t['B64'][1]) == pytest.approx(_sig(3))


def _case():
    g = torch.Generator().manual_seed(5)
    model = cases.ac.unsat_dm(9, 8, g)
    queries = [([1, 2], [[3, 4], [5, 6, 7]]), ([8], [[9, 10, 11, 8]]), ([], [[12, 13], [13, 14]])]
    return model, queries, cases.weights_for(9, g)


def test_check_combo_burden_catches_mistakes():
    model, queries, w = _case()
    lim = _limits()
    for agg in cases.AGGS:
        t = spec_combo_burden(model, queries, agg, lim, w)
        B = t['B64'].float()
        assert int(torch.isnan(B).sum()) == 2                            # (8 | 8) and (13, 13)
        best = expected_selection(B, t['ptr'], 3)
        check_combo_burden(model, queries, 3, agg, (B, best[0], best[1]), lim, w)
        check_combo_burden(model, queries, 0, agg, (B, None, None), lim, w)
        # a NaN in the wrong place, both ways
        wrong = B.clone(); wrong[0] = float('nan')
        with pytest.raises(AssertionError, match='NaN placement'):
            check_combo_burden(model, queries, 0, agg, (wrong, None, None), lim, w)
        wrong = B.clone(); wrong[torch.isnan(B)] = 1.0
        with pytest.raises(AssertionError, match='NaN placement'):
            check_combo_burden(model, queries, 0, agg, (wrong, None, None), lim, w)
        # the first slot running fastest: query 0's 2 x 3 block transposed
        wrong = B.clone(); wrong[:6] = B[:6].reshape(2, 3).t().reshape(-1)
        with pytest.raises(AssertionError, match='burden off'):
            check_combo_burden(model, queries, 0, agg, (wrong, None, None), lim, w)
        # an off-by-one combination order inside a query
        wrong = B.clone(); wrong[:6] = torch.roll(B[:6], 1)
        with pytest.raises(AssertionError, match='burden off'):
            check_combo_burden(model, queries, 0, agg, (wrong, None, None), lim, w)
        # a dropped pair: query 0's burdens without the fixed pair (1, 2)
        less = spec_combo_burden(model, [([1], queries[0][1])], agg, lim, w)['B64'].float()
        wrong = B.clone(); wrong[:6] = less
        with pytest.raises(AssertionError, match='burden off'):
            check_combo_burden(model, queries, 0, agg, (wrong, None, None), lim, w)
        # selection: a swapped tie, a value that is not the burden's bits, wrong padding
        tie = B.clone(); tie[1] = tie[0]
        tb, tp = expected_selection(tie, t['ptr'], 6)
        check_selection(tie, t['ptr'], 6, tb, tp)
        sw = tp.clone(); at = (tp[0] == 0).nonzero()[0, 0]
        assert int(tp[0, at + 1]) == 1
        sw[0, at], sw[0, at + 1] = 1, 0
        with pytest.raises(AssertionError, match='positions'):
            check_selection(tie, t['ptr'], 6, tb, sw)
        with pytest.raises(AssertionError, match='bit-equal'):
            check_selection(B, t['ptr'], 3, best[0] * (1 + 2.0 ** -23), best[1])
        pb, pp = expected_selection(B, t['ptr'], 5)                       # query 1 has 3 applicable combinations: 2 pads
        assert pp[1].tolist()[3:] == [-1, -1] and torch.isinf(pb[1, 3:]).all()
        bad = pp.clone(); bad[1, 4] = 3                                   # the NaN combination selected
        with pytest.raises(AssertionError):
            check_selection(B, t['ptr'], 5, pb, bad)


# ------------------------------------------------------------------ input conditions of the unsaturated cases
def _conditions(model, queries, weights, kd):
    lim = _limits()
    for agg in cases.AGGS:
        for known in (None, known_from_dict(kd, cases.N)):
            med, ratio = cases.input_conditions(model, queries, weights, agg, lim, known)
            assert 0.02 <= med <= 0.5, (agg, known is not None, med)
            assert ratio <= 0.25, (agg, known is not None, ratio)
    sizes = [len(f) + len(s) for f, s in queries]
    assert min(sizes) >= 2 and max(sizes) <= 4                            # whole regimens of 2 to 4 drugs


@pytest.mark.parametrize('dim,n_rel', cases.DM_EDGES)
def test_unsaturated_distmult_inputs(dim, n_rel):
    model, queries, weights, kd = cases.edge_case('distmult', n_rel, dim, 'unsat')
    _conditions(model, queries, weights, kd)


@pytest.mark.parametrize('n_rel', cases.TABLE_EDGES)
def test_unsaturated_table_inputs(n_rel):
    model, queries, weights, kd = cases.edge_case('table', n_rel, 0, 'unsat')
    _conditions(model, queries, weights, kd)


# ------------------------------------------------------------------ the Python face
def test_normalize_combination_queries():
    lim = _limits()
    f = lambda slots, fixed=None, n=10: tuple(t.tolist() for t in normalize_combination_queries(slots, fixed, n, lim))
    assert f([[1, 2], [3, -1]]) == ([], [0, 0], [1, 2, 3, -1], [0, 2, 4], [0, 2])
    assert f([[1, 2], [3, -1]], [4, 5]) == ([4, 5], [0, 2], [1, 2, 3, -1], [0, 2, 4], [0, 2])
    assert f([[[1, 2], [3, -1]], []], [[4], [5, 6]]) == ([4, 5, 6], [0, 1, 3], [1, 2, 3, -1], [0, 2, 4], [0, 2, 2])
    assert f([[[1]], [[2]]], [7]) == ([7, 7], [0, 1, 2], [1, 2], [0, 1, 2], [0, 1, 2])       # one fixed list, shared
    assert f([], [1, 2, 3]) == ([1, 2, 3], [0, 3], [], [0], [0, 0])                          # no slots: the regimen burden
    assert f([[]], [1, 2, 3]) == f([], [1, 2, 3])
    assert f((torch.tensor([1, 2]), (3,)), torch.tensor([4])) == ([4], [0, 1], [1, 2, 3], [0, 2, 3], [0, 2])
    assert f([[1, 1], [1, 0]], [0]) == ([0], [0, 1], [1, 1, 1, 0], [0, 2, 4], [0, 2])        # legal: those combinations are NaN
    for slots, fixed, match in (([[1, 2], []], None, 'query 0: slot 1 is empty'), ([[[1]], [[1, 2], []]], None, 'query 1'),
                                ([[1, 10]], None, 'query 0, slot 0'), ([[1, -2]], None, 'out of range'),
                                ([[1]] * 11, None, '11 slots'), ([list(range(10))] * 7, None, '70 alternatives'),
                                ([[1]], [3, 3], 'repeated'), ([[1]], [10], 'out of range'), ([[1]], [-1], 'out of range'),
                                ([[[1]], [[2]]], [[1], [2], [3]], '3 lists for 2'), ([[[1]], [[2]]], [[1], [10]], 'query 1'),
                                (5, None, 'slots'), ([[1.5]], None, 'drug ids'), ([['a']], None, 'drug ids'),
                                ([[1]], 'ab', 'drug ids')):
        with pytest.raises(ValueError, match=match):
            f(slots, fixed)
    with pytest.raises(ValueError, match='65 fixed'):
        f([[1]], list(range(65)), n=100)
    small = ops.ComboLimits(64, 8, 64, 100)
    with pytest.raises(ValueError, match='125 combinations'):
        normalize_combination_queries([[0, 1, 2, 3, 4]] * 3, None, 10, small)
    # the order is that of itertools.product
    slots = [[1, 2], [3], [4, 5, -1]]
    _, _, alt, aptr, _ = normalize_combination_queries(slots, None, 10, lim)
    assert [alt[aptr[s]:aptr[s + 1]].tolist() for s in range(3)] == slots
    assert len(list(itertools.product(*slots))) == 6


def test_tip_combination_risk_refusals():
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.combination_risk(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data), [[0, 1]], k=5)
    for kind in ('distmult', 'nn'):
        self = types.SimpleNamespace(decoder_kind=kind, shard=None, data=data)
        for bad in ('test', 'none', 0):
            with pytest.raises(ValueError, match='exclude'):
                TIP.combination_risk(self, [[0, 1]], k=5, exclude=bad)
        for bad in ('sum', 'noisy-or', None, 1):
            with pytest.raises(ValueError, match='aggregate'):
                TIP.combination_risk(self, [[0, 1]], k=5, aggregate=bad)
        with pytest.raises(ValueError, match='k must'):
            TIP.combination_risk(self, [[0, 1]], k=-1)
        for w in ([1.0] * 4, [1.0] * 6, [[1.0] * 5], [1, 1, -0.5, 1, 1], [1, 1, float('nan'), 1, 1], 'heavy'):
            with pytest.raises(ValueError, match='weights'):
                TIP.combination_risk(self, [[0, 1]], k=5, weights=w)
        with pytest.raises(ValueError, match='weights'):                  # one per entry of `relations`
            TIP.combination_risk(self, [[0, 1]], k=5, weights=[1.0] * 5, relations=[0, 3])
        with pytest.raises(ValueError, match='query 1'):
            TIP.combination_risk(self, [[[0, 1]], [[3, 10]]], k=5)
        with pytest.raises(ValueError, match='repeated'):
            TIP.combination_risk(self, [[0, 1]], fixed=[2, 2], k=5)
        with pytest.raises(ValueError, match='empty'):
            TIP.combination_risk(self, [[0, 1], []], k=5)
    assert CombinationRisk._fields == ('burden', 'ptr', 'best_burden', 'best_combination', 'best_drugs')
    assert 'CombinationRisk' in layers.__all__
