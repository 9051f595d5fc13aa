"""CPU tests of the add-on burden (include/tipk.h section 4i): the symbols, the `_supported` predicates, the route query and
its option, argument validation of both C entries (every refusal happens before anything touches a device, so bogus device
pointers are safe here), the host normalisation and the refusals of `TIP.add_on_risk`, the fp64 spec and the acceptance rule
(tests/addon_spec.py) on hand-worked cases, and the conditions the unsaturated inputs of tests/addon_cases.py must meet."""
import ctypes
import math
import types

import pytest
import torch

import addon_cases as cases
from addon_spec import C_BURDEN, check_addon_burden, check_selection, expected_selection, spec_addon_burden
from pair_topk_spec import known_from_dict
from tip_amd import _lib, ops
from tip_amd.layers import TIP, AddOnRisk, normalize_add_on_queries

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _dm(n=10, dim=16, n_rel=3, n_q=4, n_cand=6, k=5, agg=0, keys=None, kptr=None, krel=None, n_known=0, z=FAKE, w=FAKE,
        ctx=FAKE, cptr=FAKE, cand=FAKE, dptr=FAKE, wts=None, out_b=FAKE, best_b=FAKE, best_p=FAKE):
    return _lib.lib().tipk_distmult_addon_burden(z, n, dim, w, n_rel, ctx, cptr, n_q, cand, dptr, n_cand, wts, keys, kptr,
                                                 krel, n_known, agg, k, out_b, best_b, best_p, None, None)


def _tb(n=10, n_rel=3, ld=None, n_q=4, n_cand=6, k=5, agg=0, keys=None, kptr=None, krel=None, n_known=0, s1=FAKE, s2=FAKE,
        ctx=FAKE, cptr=FAKE, cand=FAKE, dptr=FAKE, wts=None, out_b=FAKE, best_b=FAKE, best_p=FAKE):
    return _lib.lib().tipk_pair_table_addon_burden(s1, s2, n_rel if ld is None else ld, n, n_rel, ctx, cptr, n_q, cand, dptr,
                                                   n_cand, wts, keys, kptr, krel, n_known, agg, k, out_b, best_b, best_p, None)


def test_symbols_and_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() >= 30
    for name in ('tipk_addon_max_context', 'tipk_distmult_addon_burden_supported',
                 'tipk_distmult_addon_burden_workspace_bytes', 'tipk_distmult_addon_burden_lds_route',
                 'tipk_distmult_addon_burden', 'tipk_pair_table_addon_burden_supported', 'tipk_pair_table_addon_burden'):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.tipk_addon_max_context() == 64 and ops.addon_max_context() == 64
    dm, tb = L.tipk_distmult_addon_burden_supported, L.tipk_pair_table_addon_burden_supported
    assert dm(645, 4, 1097, 10) == 1 and dm(645, 16, 1097, 10) == 1 and dm(645, 256, 1097, 10) == 1
    for dim in (0, 2, 6, 260):
        assert dm(645, dim, 1097, 10) == 0
    assert dm(645, 16, 1097, 0) == 1 and dm(645, 16, 1097, 128) == 1     # k = 0: burdens only
    assert dm(645, 16, 1097, -1) == 0 and dm(645, 16, 1097, 129) == 0
    assert dm(645, 16, 1, 4) == 1 and dm(645, 16, 65536, 4) == 1
    assert dm(645, 16, 0, 4) == 0 and dm(645, 16, 65537, 4) == 0
    assert dm(1, 16, 4, 4) == 1 and dm(46340, 256, 65536, 128) == 1
    assert dm(0, 16, 4, 4) == 0 and dm(46341, 16, 4, 4) == 0
    assert tb(1, 1, 0) == 1 and tb(46340, 65536, 128) == 1
    assert tb(0, 4, 4) == 0 and tb(46341, 4, 4) == 0 and tb(645, 0, 4) == 0 and tb(645, 65537, 4) == 0
    assert tb(645, 1097, -1) == 0 and tb(645, 1097, 129) == 0
    ws = L.tipk_distmult_addon_burden_workspace_bytes
    assert ws(645, 16, 1097, 256, 645, 10) == 0 and ws(645, 16, 1097, 0, 0, 0) == 0
    assert ws(46341, 16, 4, 1, 1, 4) == -1 and ws(645, 6, 4, 1, 1, 4) == -1 and ws(645, 16, 4, 1, 1, 129) == -1
    assert ws(645, 16, 4, -1, 1, 4) == -1 and ws(645, 16, 4, 1, -1, 4) == -1


def test_route_query_and_option():
    L = _lib.lib()
    route = L.tipk_distmult_addon_burden_lds_route
    assert _lib.get_option('addon_global') == 0
    assert route(16, 1097) == 1                                          # BioSNAP: 1 097 rows of 80 B beside the waves' state
    assert route(64, 640) == 0                                           # 640 rows of 272 B
    assert route(16, 300) == 1 and route(32, 300) == 1
    assert route(256, 700) == 0 and route(6, 10) == 0
    _lib.set_option('addon_global', 1)
    try:
        assert _lib.get_option('addon_global') == 1
        assert route(16, 1097) == 0
        assert _lib.get_option('regimen_global') == 0 and L.tipk_distmult_regimen_topk_lds_route(16, 1097) == 1
    finally:
        _lib.set_option('addon_global', 0)
    assert route(16, 1097) == 1 and _lib.get_option('addon_global') == 0


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(k=-1) == EINVAL and call(k=-3) == EINVAL
        assert call(n_q=-1) == EINVAL and call(n_cand=-1) == EINVAL
        assert call(n=0) == EINVAL and call(n=-5) == EINVAL
        assert call(n_rel=0) == EINVAL
        assert call(n_known=-1) == EINVAL
        assert call(agg=2) == EINVAL and call(agg=-1) == EINVAL           # unknown aggregate
        assert call(agg=1, n_q=0) == 0                                  # (an empty call: a full one is not refused and,
                                                                          # where a device is present, launches on FAKE)
        assert call(keys=FAKE, n_known=2) == EINVAL                       # known arrays given only in part
        assert call(keys=FAKE, kptr=FAKE, n_known=2) == EINVAL
        assert call(kptr=FAKE, krel=FAKE, n_known=2) == EINVAL
        assert call(krel=FAKE) == EINVAL
        assert call(cptr=None) == EINVAL and call(ctx=None) == EINVAL and call(cand=None) == EINVAL
        assert call(out_b=None) == EINVAL
        assert call(best_b=None) == EINVAL and call(best_p=None) == EINVAL   # best outputs missing with k > 0
        assert call(k=0, best_b=None, best_p=None, n=46341) == EUNSUPPORTED  # ... and not missed with k = 0
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(s2=None) == EINVAL
    assert _dm(dim=0) == EINVAL and _dm(dim=-4) == EINVAL
    assert _tb(ld=2) == EINVAL                                           # row stride below n_rel
    assert _dm(k=-1, dim=6) == EINVAL                                    # argument errors come before shape limits
    assert _dm(agg=7, n=46341) == EINVAL
    assert _tb(k=-1, n=46341) == EINVAL


def test_unsupported_shapes_and_empty_calls():
    assert _dm(k=129) == EUNSUPPORTED
    assert _dm(dim=2) == EUNSUPPORTED and _dm(dim=6) == EUNSUPPORTED and _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED
    assert _dm(w=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # rel_w must be 16-byte aligned
    assert _dm(n_cand=1 << 31) == EUNSUPPORTED and _tb(n_cand=1 << 31) == EUNSUPPORTED   # positions are int32
    assert _tb(k=129) == EUNSUPPORTED
    assert _tb(n=46341) == EUNSUPPORTED
    assert _tb(n_rel=65537) == EUNSUPPORTED
    for agg in (0, 1):
        for dptr in (FAKE, None):
            assert _dm(n_q=0, agg=agg, dptr=dptr) == 0 and _tb(n_q=0, agg=agg, dptr=dptr) == 0    # nothing to do,
            assert _dm(n_cand=0, agg=agg, dptr=dptr) == 0 and _tb(n_cand=0, agg=agg, dptr=dptr) == 0   # nothing launched
    assert _dm(n_q=0, z=None, ctx=None, cptr=None, cand=None, out_b=None, best_b=None, best_p=None) == 0
    assert _tb(n_cand=0, s1=None, ctx=None, cptr=None, cand=None, out_b=None, best_b=None, best_p=None) == 0
    assert _dm(n_q=0, keys=FAKE, kptr=FAKE, krel=FAKE, n_known=3) == 0


def test_ops_refuse_cpu_tensors_and_bad_aggregate():
    ctx, cptr, cand = torch.tensor([0, 1, 2]), torch.tensor([0, 3]), torch.tensor([3, 4])
    with pytest.raises(_lib.TipkError):
        ops.distmult_addon_burden(torch.ones(5, 4), torch.ones(2, 4), ctx, cptr, cand, None, 2, 'max')
    with pytest.raises(_lib.TipkError):
        ops.pair_table_addon_burden(torch.ones(5, 3), torch.ones(5, 3), ctx, cptr, cand, None, 2, 'noisy_or')


# ------------------------------------------------------------------ the spec and the rule, by hand
def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def _line():
    """The line graph: z = (1, 2, 3), w = 1, so the logits of (0,1), (0,2), (1,2) are 2, 3 and 6."""
    return ('distmult', torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[1.0]]))


def test_spec_by_hand():
    m = _line()
    one = lambda ctx, c, agg, known=None, w=None: float(spec_addon_burden(
        m, torch.tensor(ctx), torch.tensor([0, len(ctx)]), torch.tensor([c]), None, agg, w, known)['B64'][0])
    for agg in cases.AGGS:
        assert one([0], 1, agg) == pytest.approx(_sig(2), rel=1e-15)
        assert one([1], 0, agg) == pytest.approx(_sig(2), rel=1e-15)     # the pair, not its direction
    assert one([0, 1], 2, 'noisy_or') == pytest.approx(1 - (1 - _sig(3)) * (1 - _sig(6)), rel=1e-14)
    assert one([0, 1], 2, 'max') == pytest.approx(_sig(6), rel=1e-15)
    for agg in cases.AGGS:
        for pair in ((1, 2), (2, 1)):                                    # (1, 2) known for r, in either direction
            assert one([0, 1], 2, agg, known_from_dict({pair: [0]}, 3)) == pytest.approx(_sig(3), rel=1e-14)
        both = known_from_dict({(1, 2): [0], (2, 0): [0]}, 3)
        assert one([0, 1], 2, agg, both) == 0.0                          # no contributing triple: P = 0
        assert one([0, 1], 2, agg, None, torch.tensor([2.5])) == pytest.approx(2.5 * one([0, 1], 2, agg), rel=1e-15)
        # not applicable: a member, an id out of range, an empty context, a bad id in the context, a NaN logit
        for ctx, c in (([0, 1], 1), ([0, 1], 3), ([0, 1], -1), ([], 2), ([0, 3], 2), ([0, -1], 2)):
            assert math.isnan(one(ctx, c, agg)), (ctx, c)
    nan_model = ('distmult', torch.tensor([[1.0], [float('nan')], [3.0]]), torch.tensor([[1.0]]))
    t = spec_addon_burden(nan_model, torch.tensor([0, 1, 0]), torch.tensor([0, 2, 3]), torch.tensor([2]), None, 'max',
                          torch.tensor([0.0]))
    assert math.isnan(float(t['B64'][0])) and float(t['B64'][1]) == 0.0  # the NaN rule holds under max and a weight of 0
    t = spec_addon_burden(nan_model, torch.tensor([0, 1]), torch.tensor([0, 2]), torch.tensor([2]), None, 'noisy_or', None,
                          known_from_dict({(2, 1): [0]}, 3))
    assert float(t['B64'][0]) == pytest.approx(_sig(3), rel=1e-14)       # a known triple's NaN does not count
    # the two candidate forms number the same tasks
    a = spec_addon_burden(m, torch.tensor([0, 1]), torch.tensor([0, 1, 2]), torch.tensor([2, 0]), None, 'max')
    b = spec_addon_burden(m, torch.tensor([0, 1]), torch.tensor([0, 1, 2]), torch.tensor([2, 0, 2, 0]),
                          torch.tensor([0, 2, 4]), 'max')
    assert a['task_ptr'].tolist() == [0, 2, 4] and b['task_ptr'].tolist() == [0, 2, 4]
    for t in (a, b):                                                     # (q0, 2), (q0, 0): a member, (q1, 2), (q1, 0)
        assert t['applicable'].tolist() == [True, False, True, True] and math.isnan(float(t['B64'][1]))
        assert t['B64'][[0, 2, 3]].tolist() == pytest.approx([_sig(3), _sig(6), _sig(2)], rel=1e-15)


def test_expected_selection_by_hand():
    nan, inf = float('nan'), float('inf')
    b = torch.tensor([3.0, nan, 1.0, 1.0, 0.5, nan, nan, 2.0, -0.0, 0.0])
    ptr = torch.tensor([0, 5, 5, 7, 10])
    vals, pos = expected_selection(b, ptr, 3)
    assert pos.tolist() == [[4, 2, 3], [-1, -1, -1], [-1, -1, -1], [1, 2, 0]]     # ties (and -0 == +0) by position
    assert vals[0].tolist() == [0.5, 1.0, 1.0] and vals[1].tolist() == [inf] * 3 and vals[3].tolist() == [-0.0, 0.0, 2.0]
    assert math.copysign(1, float(vals[3, 0])) == -1.0                   # the value at that position, bit for bit
    vals, pos = expected_selection(b, ptr, 6)
    assert pos[0].tolist() == [4, 2, 3, 0, -1, -1] and vals[0, 4:].tolist() == [inf, inf]
    check_selection(b, ptr, 3, *expected_selection(b, ptr, 3))
    for plant in ((0, 1, 3), (1, 0, 0), (3, 0, 2)):
        vals, pos = expected_selection(b, ptr, 3)
        pos[plant[0], plant[1]] = plant[2]
        with pytest.raises(AssertionError):
            check_selection(b, ptr, 3, vals, pos)
    vals, pos = expected_selection(b, ptr, 3)
    vals[3, 0] = 0.0                                                     # +0 where the burden is -0
    with pytest.raises(AssertionError, match='bit-equal'):
        check_selection(b, ptr, 3, vals, pos)


def test_check_addon_burden_catches_mistakes():
    """The rule on an unsaturated case with the fp64 burdens rounded to fp32 as the result, and with planted mistakes: a
    dropped and a doubled relation, a dropped context drug, NaN moved, the selection off."""
    model, ctx, cands, weights, kd = cases.edge_case('distmult', 65, 16, 'unsat', count=12)
    ctx[3] = []
    drugs, ptr = cases.csr(ctx)
    cand, cptr = cases.csr(cands)
    known = known_from_dict(kd, cases.N)
    k = 7
    for agg in cases.AGGS:
        t = spec_addon_burden(model, drugs, ptr, cand, cptr, agg, weights, known)
        B = t['B64'].float()
        good = (B, *[x.to(torch.float32 if i == 0 else torch.int32) for i, x in enumerate(expected_selection(B, cptr, k))])
        check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, good, weights, known)
        check_addon_burden(model, drugs, ptr, cand, cptr, 0, agg, (B, None, None), weights, known)
        assert bool(torch.isnan(B[cptr[3]:cptr[4]]).all()) and bool((good[2][3] == -1).all())
        ok = torch.nonzero(t['applicable']).reshape(-1)
        task = int(ok[5])
        heavy = int((t['P64'][task] * weights.double()).argmax())

        def planted(change, match):
            bad = B.clone()
            change(bad)
            sel = expected_selection(bad, cptr, k)
            with pytest.raises(AssertionError, match=match):
                check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, (bad, sel[0], sel[1].int()), weights, known)

        share = float(t['P64'][task, heavy] * weights[heavy])
        planted(lambda b: b.__setitem__(task, float(b[task]) - share), 'off fp64')          # a relation dropped
        planted(lambda b: b.__setitem__(task, float(b[task]) + share), 'off fp64')          # ... doubled
        planted(lambda b: b.__setitem__(task, float(b[task]) - float(t['B64'][task]) / t['R']), 'off fp64')   # an average one
        planted(lambda b: b.__setitem__(task, float('nan')), 'NaN placement')
        planted(lambda b: b.__setitem__(int(cptr[3]), 1.0), 'NaN placement')
        q = int(t['query'][task])
        if int(ptr[q + 1] - ptr[q]) > 1:                                  # the query's last context drug dropped
            short = [c[:-1] if i == q else c for i, c in enumerate(ctx)]
            t2 = spec_addon_burden(model, *cases.csr(short), cand, cptr, agg, weights, known)
            wrong = torch.where(t['applicable'], t2['B64'], t['B64']).float()
            with pytest.raises(AssertionError, match='off fp64'):
                check_addon_burden(model, drugs, ptr, cand, cptr, 0, agg, (wrong, None, None), weights, known)
        bad_pos = good[2].clone()
        bad_pos[0, [0, 1]] = bad_pos[0, [1, 0]]
        with pytest.raises(AssertionError, match='selection'):
            check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, (B, good[1], bad_pos), weights, known)


# ------------------------------------------------------------------ the inputs
def _hold_conditions(model, ctx, cands, weights, kd, what):
    known = known_from_dict(kd, cases.N)
    for agg in cases.AGGS:
        for kn in (None, known):
            med, ratio = cases.input_conditions(model, ctx, cands, weights, agg, kn)
            assert 0.02 <= med <= 0.5, (what, agg, 'median P_r', med)
            assert ratio <= 0.25, (what, agg, 'T_B * R / B64', ratio)


@pytest.mark.parametrize('dim,n_rel', cases.DM_EDGES)
def test_unsaturated_distmult_inputs(dim, n_rel):
    _hold_conditions(*cases.edge_case('distmult', n_rel, dim, 'unsat'), what='dm dim%d R%d' % (dim, n_rel))


@pytest.mark.parametrize('n_rel', cases.TABLE_EDGES)
def test_unsaturated_table_inputs(n_rel):
    _hold_conditions(*cases.edge_case('table', n_rel, 0, 'unsat'), what='table R%d' % n_rel)


@pytest.mark.parametrize('n_rel,dim,m', cases.DM_WIDE)
def test_unsaturated_wide_inputs(n_rel, dim, m):
    g = torch.Generator().manual_seed(n_rel + dim)
    model = cases.unsat_dm(n_rel, dim, g)
    ctx, cands = cases.random_queries(12, g, lo=m, hi=m)
    _hold_conditions(model, ctx, cands, cases.weights_for(n_rel, g), {}, what='dm wide dim%d R%d' % (dim, n_rel))
    assert C_BURDEN >= 4.0


# ------------------------------------------------------------------ host normalisation, TIP refusals
def test_normalize_add_on_queries():
    regs = [[5, 3, 3, 1], [], [7], [9, 2]]
    drugs, ptr, cand, cptr = normalize_add_on_queries(regs, None, None, 10, 64)
    assert drugs.dtype == torch.int32 and ptr.dtype == torch.int64 and cand.dtype == torch.int32
    assert drugs.tolist() == [1, 3, 5, 7, 2, 9] and ptr.tolist() == [0, 3, 3, 4, 6]
    assert cand.tolist() == list(range(10)) and cptr is None             # every drug, shared
    drugs, ptr, cand, cptr = normalize_add_on_queries(regs, [4, 1, 1, 0], [3, -1, 7, -1], 10, 64)
    assert drugs.tolist() == [1, 5, 2, 9] and ptr.tolist() == [0, 2, 2, 2, 4]    # 3 and 7 taken out: an empty context is legal
    assert cand.tolist() == [4, 1, 1, 0] and cptr is None                # shared list: order and repeats kept
    d2, p2, c2, cp2 = normalize_add_on_queries(regs, torch.tensor([4, 1, 1, 0]), torch.tensor([3, -1, 7, -1]), 10, 64)
    assert (d2.tolist(), p2.tolist(), c2.tolist(), cp2) == (drugs.tolist(), ptr.tolist(), cand.tolist(), None)
    drugs, ptr, cand, cptr = normalize_add_on_queries(regs, [[3, 0], [], [7, 7, 1], (2,)], [3, -1, -1, 9], 10, 64)
    assert drugs.tolist() == [1, 5, 7, 2] and ptr.tolist() == [0, 2, 2, 3, 4]
    assert cand.tolist() == [3, 0, 7, 7, 1, 2] and cptr.tolist() == [0, 2, 2, 5, 6] and cptr.dtype == torch.int64
    d3 = normalize_add_on_queries((torch.tensor([5, 3, 3, 1, 7, 9, 2]), torch.tensor([0, 4, 4, 5, 7])), None, None, 10, 64)
    assert d3[0].tolist() == [1, 3, 5, 7, 2, 9] and d3[1].tolist() == [0, 3, 3, 4, 6]
    d4 = normalize_add_on_queries([], None, None, 10, 64)
    assert d4[0].tolist() == [] and d4[1].tolist() == [0] and d4[2].numel() == 10
    assert normalize_add_on_queries(regs, [], None, 10, 64)[2].numel() == 0
    # 65 distinct drugs are a legal regimen only when one of them is replaced
    d5 = normalize_add_on_queries([list(range(65))], [70], [64], 100, 64)
    assert d5[0].tolist() == list(range(64)) and d5[1].tolist() == [0, 64]
    with pytest.raises(ValueError, match='at most 64'):
        normalize_add_on_queries([list(range(65))], [70], None, 100, 64)
    with pytest.raises(ValueError, match='at most 64'):
        normalize_add_on_queries([list(range(65))], [70], [-1], 100, 64)
    with pytest.raises(ValueError, match='at most'):
        normalize_add_on_queries([list(range(66))], [70], [0], 100, 64)
    for rep in ([4, -1, 7, -1], [3, 0, 7, -1], [3, -1, 7, 10]):
        with pytest.raises(ValueError, match='not a member'):
            normalize_add_on_queries(regs, None, rep, 10, 64)
    for rep in ([3, -1, 7], 3, [[3], [-1], [7], [-1]], [3.0, -1.0, 7.0, -1.0]):
        with pytest.raises(ValueError, match='replace'):
            normalize_add_on_queries(regs, None, rep, 10, 64)
    for bad in ([0, 10], [-1], [[0], [1], [2], [10]], torch.tensor([11])):
        with pytest.raises(ValueError, match='out of range'):
            normalize_add_on_queries(regs, bad, None, 10, 64)
    for bad in ([[0], [1]], 'ab', [['a'], [1], [2], [3]], torch.tensor([0.5]), torch.tensor([[1, 2]])):
        with pytest.raises(ValueError, match='candidates'):
            normalize_add_on_queries(regs, bad, None, 10, 64)
    with pytest.raises(ValueError, match='out of range'):
        normalize_add_on_queries([[0, 10]], None, None, 10, 64)


def test_tip_add_on_risk_refusals():
    data = types.SimpleNamespace(n_drug=10, n_dd_et=5)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.add_on_risk(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data), [[0, 1]], k=5)
    for kind in ('distmult', 'nn'):
        self = types.SimpleNamespace(decoder_kind=kind, shard=None, data=data)
        for bad in ('test', 'none', 0):
            with pytest.raises(ValueError, match='exclude'):
                TIP.add_on_risk(self, [[0, 1]], k=5, exclude=bad)
        for bad in ('sum', 'noisy-or', None, 1):
            with pytest.raises(ValueError, match='aggregate'):
                TIP.add_on_risk(self, [[0, 1]], k=5, aggregate=bad)
        with pytest.raises(ValueError, match='k must'):
            TIP.add_on_risk(self, [[0, 1]], k=-1)
        for w in ([1.0] * 4, [1.0] * 6, [[1.0] * 5], [1, 1, -0.5, 1, 1], [1, 1, float('nan'), 1, 1],
                  [1, 1, float('inf'), 1, 1], 'heavy'):
            with pytest.raises(ValueError, match='weights'):
                TIP.add_on_risk(self, [[0, 1]], k=5, weights=w)
        with pytest.raises(ValueError, match='weights'):                  # one per entry of `relations`
            TIP.add_on_risk(self, [[0, 1]], k=5, weights=[1.0] * 5, relations=[0, 3])
        with pytest.raises(ValueError, match='not a member'):
            TIP.add_on_risk(self, [[0, 1], [2, 3]], k=5, replace=[0, 4])
        with pytest.raises(ValueError, match='out of range'):
            TIP.add_on_risk(self, [[0, 1], [3, 10]], k=5)
        with pytest.raises(ValueError, match='out of range'):
            TIP.add_on_risk(self, (torch.tensor([0, -1]), torch.tensor([0, 2])), k=5)
        with pytest.raises(ValueError, match='out of range'):
            TIP.add_on_risk(self, [[0, 1]], candidates=[2, 10], k=5)
        with pytest.raises(ValueError, match='out of range'):
            TIP.add_on_risk(self, [[0, 1]], candidates=[[-1]], k=5)
        big = types.SimpleNamespace(decoder_kind=kind, shard=None, data=types.SimpleNamespace(n_drug=100, n_dd_et=5))
        with pytest.raises(ValueError, match='at most'):
            TIP.add_on_risk(big, [list(range(ops.addon_max_context() + 1))], k=5)
    assert AddOnRisk._fields == ('burden', 'candidate', 'ptr', 'best_burden', 'best_drug')
