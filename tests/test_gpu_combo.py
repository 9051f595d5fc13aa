"""-m gpu: `tipk_distmult_combo_burden` / `tipk_pair_table_combo_burden` (include/tipk.h section 4n) and
`TIP.combination_risk` against the fp64 acceptance rule of tests/combo_spec.py -- small shapes around the 64-relation lane
groups and the relation window with saturating and unsaturated inputs (tests/combo_cases.py), every slot count, slot size,
fixed-list length and combination count at which the kernels take another path, the persistent loops' second round, -1
alternatives, illegal queries beside legal ones, weights, NaN and infinite logits, k from 0 to 128, every route (prefix reuse
on and off, every run length) bit-equal, repeat runs and graph capture, the results pinned to the regimen and pair top-k
entries that already ship, and both decoder kinds of the model face on the bundled graph."""
import contextlib
import ctypes
import itertools

import pytest
import torch

import combo_cases as cases
from addon_spec import expected_selection
from combo_cases import AGGS, N
from combo_spec import check_combo_burden, combo_ptr, query_lists, spec_combo_burden
from pair_topk_spec import U, known_from_dict, logits64
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _lim():
    return ops.combo_limits()


def _dev(model):
    return (model[0], model[1].to(DEV), model[2].to(DEV))


def _known(d, n=N):
    return tuple(t.to(DEV) for t in known_from_dict(d, n))


def _run(model, queries, k, agg, weights=None, known=None):
    plan = ops.combo_plan(*query_lists(queries), DEV)
    fn = ops.distmult_combo_burden if model[0] == 'distmult' else ops.pair_table_combo_burden
    burden, ptr, best_b, best_c = fn(model[1], model[2], plan, k, agg, weights, known)
    assert ptr.tolist() == combo_ptr(queries, model[1].shape[0], _lim()).tolist()
    return burden, best_b, best_c


def _same(a, b):
    """Bit-equal results (NaN included)."""
    return all((x is None and y is None) or torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(a, b))


@contextlib.contextmanager
def _route(no_prefix, run):
    assert _lib.get_option('combo_no_prefix') == 0 and _lib.get_option('combo_run') == 0
    _lib.set_option('combo_no_prefix', no_prefix)
    _lib.set_option('combo_run', run)
    try:
        yield
    finally:
        _lib.set_option('combo_no_prefix', 0)
        _lib.set_option('combo_run', 0)


def _hold(model, queries, weights, kd, ks, what):
    """The rule for both aggregates, with and without the known list and the weights; the small calls of these tests get
    runs of one combination, so every result is also taken with runs of 5 (prefix reuse) and must be the same bits."""
    model, weights = _dev(model), weights.to(DEV)
    known = _known(kd)
    for agg in AGGS:
        for k in ks:
            for kn in (None, known):
                for w in (None, weights):
                    got = _run(model, queries, k, agg, w, kn)
                    with _route(0, 5):
                        assert _same(got, _run(model, queries, k, agg, w, kn)), (what, agg, 'runs of 5')
                    check_combo_burden(model, queries, k, agg, got, _lim(), w, kn, what='%s %s k=%d' % (what, agg, k))


def _n_cu():
    n_cu = ctypes.c_int(0)
    assert _lib.lib().tipk_device_info(0, ctypes.byref(n_cu), None, None, None, 0) == 0
    return n_cu.value


def _model(kind, n_rel, g, dim=16):
    return _dev(cases.ac.mixed_dm(n_rel, dim, g) if kind == 'distmult' else cases.ac.mixed_table(n_rel, g))


# ------------------------------------------------------------------ lane and window edges
@pytest.mark.parametrize('recipe', ['mixed', 'unsat'])
@pytest.mark.parametrize('dim,n_rel', cases.DM_EDGES)
def test_distmult_lane_and_window_edges(dim, n_rel, recipe):
    _hold(*cases.edge_case('distmult', n_rel, dim, recipe), ks=[5], what='dm %s dim%d R%d' % (recipe, dim, n_rel))


@pytest.mark.parametrize('recipe', ['mixed', 'unsat'])
@pytest.mark.parametrize('n_rel', cases.TABLE_EDGES)
def test_table_lane_and_window_edges(n_rel, recipe):
    _hold(*cases.edge_case('table', n_rel, 0, recipe), ks=[5], what='table %s R%d' % (recipe, n_rel))


# ------------------------------------------------------------------ query shapes
def _shape_queries(g):
    perm = lambda m: torch.randperm(N, generator=g)[:m].tolist()
    p = perm(N)
    q = []
    for m in (0, 1, 2, 64):                                              # S = 0: the regimen burden of the fixed list
        q.append((perm(m), []))
    q.append(([], [[p[0]]]))                                             # one slot of one alternative, nothing fixed
    q.append((p[60:63], [[p[0]]]))
    q.append((p[60:62], [[p[0], p[1]]]))
    q.append((p[64:66], [p[:64]]))                                       # 64 alternatives in one slot
    q.append((p[60:61], [[p[0], p[1]], [p[2], p[3], -1]]))               # S = 2
    q.append((p[60:62], [[p[0]], [p[1], p[2]], [p[3], p[4], p[5]]]))     # S = 3
    q.append((p[60:61], [[p[2 * s], p[2 * s + 1]] for s in range(8)]))   # S = 8: 256 combinations, 37 terms each
    q.append(([], [[p[2 * s], -1] for s in range(8)]))
    q.append((p[60:61], [[p[s], -1] for s in range(10)]))                # S = 10, the most: 1 024 combinations, 56 terms
    q.append((p[:64], [[p[64], p[65], -1]]))                             # 64 fixed drugs: 2 016 base pairs
    q.append((perm(65), [[0, 1]]))                                       # 65 fixed drugs: illegal
    q.append(([], [p[:63]]))                                             # 63, 64, 65 and 1 025 combinations
    q.append((p[65:67], [p[:64]]))
    q.append(([], [p[:5], p[5:18]]))
    q.append((p[60:61], [p[:5], p[5:10], p[10:51]]))
    return q


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_slot_counts_sizes_fixed_lengths_and_combination_counts(kind):
    g = torch.Generator().manual_seed(8)
    n_rel = 65
    model = _model(kind, n_rel, g)
    queries = _shape_queries(g)
    lim = _lim()
    assert (lim.max_fixed, lim.max_slots, lim.max_alternatives) == (64, 10, 64)       # the shapes above sit on these limits
    sizes = (combo_ptr(queries, N, lim)[1:] - combo_ptr(queries, N, lim)[:-1]).tolist()
    assert sizes[-4:] == [63, 64, 65, 1025] and sizes[10] == 256 and sizes[12] == 1024 and sizes[14] == 2
    weights = cases.weights_for(n_rel, g).to(DEV)
    known = _known(cases.known_for(queries[4:12], n_rel, g))
    for agg in AGGS:
        got = _run(model, queries, 7, agg, weights, known)
        t = check_combo_burden(model, queries, 7, agg, got, lim, weights, known, what='%s shapes %s' % (kind, agg))
        assert bool(torch.isnan(got[0][t['ptr'][14]:t['ptr'][15]]).all())              # the 65-drug list
        for no_prefix, run in ((0, 64), (1, 64), (0, 7), (1, 1)):
            with _route(no_prefix, run):
                assert _same(got, _run(model, queries, 7, agg, weights, known)), (agg, no_prefix, run)


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_many_small_queries_second_round(kind):
    """More (query, row) tasks and more runs than the persistent grids hold in one round: 40 distinct queries, repeated."""
    g = torch.Generator().manual_seed(9)
    n_rel = 20
    model = _model(kind, n_rel, g)
    block = cases.mixed_queries(40, g)
    per_block = int(combo_ptr(block, N, _lim())[-1])
    rows_block = ops.combo_plan(*query_lists(block), 'cpu').n_rows
    repeats = (8 * _n_cu() * 4) // min(per_block, rows_block) + 2         # both grids: at most 8 workgroups of 4 waves per CU
    queries = block * repeats
    for agg in AGGS:
        with _route(0, 1):                                                # a run is one combination: the call has > grid runs
            got = _run(model, queries, 3, agg)
        assert _same(got, _run(model, queries, 3, agg))
        first = (got[0][:per_block], got[1][:40], got[2][:40])
        check_combo_burden(model, block, 3, agg, first, _lim(), what='%s second round %s' % (kind, agg))
        assert torch.equal(got[0].view(torch.int32).reshape(repeats, per_block),
                           first[0].view(torch.int32)[None, :].expand(repeats, -1))
        assert torch.equal(got[2].reshape(repeats, 40, 3), first[2][None].expand(repeats, -1, -1))


# ------------------------------------------------------------------ -1 alternatives, repeated and fixed alternatives
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_empty_slots_repeated_drugs_and_fixed_alternatives(kind):
    g = torch.Generator().manual_seed(10)
    n_rel = 65
    model = _model(kind, n_rel, g)
    drugs = [3, 9, 27, 50]
    weights = cases.weights_for(n_rel, g).to(DEV)
    for agg in AGGS:
        # every slot [d, -1]: which drugs to stop.  The all-empty and the single-drug combinations are +0 exactly
        q = ([], [[d, -1] for d in drugs])
        b = _run(model, [q], 0, agg, weights)[0]
        check_combo_burden(model, [q], 0, agg, (b, None, None), _lim(), weights)
        combos = list(itertools.product(*q[1]))
        few = torch.tensor([sum(d >= 0 for d in c) <= 1 for c in combos], device=DEV)
        assert int(few.sum()) == 5 and bool((b.view(torch.int32)[few] == 0).all()) and bool((b[~few] > 0).all())
        # a drug repeated across slots: NaN exactly where both slots take it
        q = ([1], [[3, 9], [9, 27], [3, -1]])
        b = _run(model, [q], 0, agg)[0]
        twice = torch.tensor([len([d for d in c if d >= 0]) != len(set(d for d in c if d >= 0)) for c in itertools.product(*q[1])])
        assert torch.equal(torch.isnan(b).cpu(), twice) and int(twice.sum()) == 4
        check_combo_burden(model, [q], 0, agg, (b, None, None), _lim())
        # a drug both fixed and alternative: NaN where it is chosen
        q = ([9, 50], [[3, 9], [27, 50, -1]])
        b = _run(model, [q], 0, agg)[0]
        assert torch.isnan(b).cpu().tolist() == [False, True, False, True, True, True]
        check_combo_burden(model, [q], 0, agg, (b, None, None), _lim())


# ------------------------------------------------------------------ illegal queries beside legal ones
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_illegal_queries_in_one_call(kind):
    g = torch.Generator().manual_seed(11)
    n_rel, k = 65, 4
    model = _model(kind, n_rel, g)
    legal = cases.mixed_queries(6, g)
    illegal = [([N], [[1, 2]]), ([-1, 3], [[1, 2]]), ([4, 4], [[1, 2]]), ([0], [[1, N]]), ([0], [[1, -2], [3]]),
               ([0], [[1, 2], []]), ([0], [[1]] * (_lim().max_slots + 1)), ([], [list(range(33)), list(range(33, 66))]),
               (list(range(65)), []), ([], [list(range(16))] * 7)]       # 16^7 > 2^24 and 112 alternatives
    queries = []
    for i, q in enumerate(illegal):
        queries += [legal[i % len(legal)], q]
    known = _known(cases.known_for(legal, n_rel, g))
    for agg in AGGS:
        got = _run(model, queries, k, agg, None, known)
        t = check_combo_burden(model, queries, k, agg, got, _lim(), None, known, what='%s illegal %s' % (kind, agg))
        ptr = t['ptr'].tolist()
        for i, q in enumerate(queries):
            if i % 2:
                assert bool(torch.isnan(got[0][ptr[i]:ptr[i + 1]]).all()) and got[2][i].tolist() == [-1] * k
            else:                                                          # a legal row is what its query gives alone
                alone = _run(model, [q], k, agg, None, known)
                assert _same(alone, (got[0][ptr[i]:ptr[i + 1]], got[1][i:i + 1], got[2][i:i + 1])), (agg, i)


# ------------------------------------------------------------------ weights, NaN and infinities
def test_zero_weights_nan_and_infinite_logits():
    g = torch.Generator().manual_seed(12)
    n_rel = 70
    queries = [([1, 2], [[3, 4], [5, 6, -1]]), ([], [[7, 8], [9]]), ([10], [[11, 12]])]
    weights = cases.weights_for(n_rel, g)
    weights[::3] = 0.0
    # DistMult: drug 4 has a NaN coordinate: every combination that takes it is NaN, zero weights or not ...
    kind, z, w = cases.ac.mixed_dm(n_rel, 16, g)
    z[4, 3] = float('nan')
    model = _dev((kind, z, w))
    for agg in AGGS:
        for wts in (None, weights.to(DEV), torch.zeros(n_rel, device=DEV)):
            got = _run(model, queries, 3, agg, wts)
            check_combo_burden(model, queries, 3, agg, got, _lim(), wts)
            assert torch.isnan(got[0][:6]).tolist() == [False] * 3 + [True] * 3
        # ... unless every triple of its pairs is known
        known = _known({(4, d): list(range(n_rel)) for d in (1, 2, 5, 6)})
        got = _run(model, queries, 3, agg, weights.to(DEV), known)
        check_combo_burden(model, queries, 3, agg, got, _lim(), weights.to(DEV), known)
        assert not bool(torch.isnan(got[0]).any())
    # tables: single NaN, +inf and -inf logits
    kind, s1, s2 = cases.ac.mixed_table(n_rel, g)
    s1, s2 = s1.clone(), s2.clone()
    s1[7, 5] = float('inf')            # pair (7, 9): P_5 = 1 exactly
    s2[9, 6] = float('-inf')           # pair (7, 9) and (8, 9): contributes nothing / never the maximum
    s1[11, 64] = float('nan')          # pair (11, 10)?  10 < 11: the first argument is drug 10 -- s1[11] is not read
    s2[12, 69] = float('nan')          # pair (10, 12): NaN
    model = _dev((kind, s1, s2))
    for agg in AGGS:
        for wts in (None, weights.to(DEV)):
            got = _run(model, queries, 2, agg, wts)
            check_combo_burden(model, queries, 2, agg, got, _lim(), wts)
            assert torch.isnan(got[0][-2:]).tolist() == [False, True] and bool(torch.isfinite(got[0][6:8]).all())


# ------------------------------------------------------------------ k
def test_k_values():
    g = torch.Generator().manual_seed(13)
    n_rel = 40
    model = _model('distmult', n_rel, g)
    p = torch.randperm(N, generator=g).tolist()
    queries = [([p[0]], [p[1:9], p[9:17], p[17:21]]), ([], [[p[1], p[2]]]), ([p[3], p[4]], []), ([p[5]], [[p[5]]]),
               ([], [p[1:6], p[3:8]])]                                   # 256, 2, 1, 1 (NaN) and 25 (3 NaN) combinations
    for k in (0, 1, 3, 128):
        for agg in AGGS:
            got = _run(model, queries, k, agg)
            check_combo_burden(model, queries, k, agg, got, _lim())
            if k == 128:
                assert (got[2] >= 0).sum(1).tolist() == [128, 2, 1, 0, 22]
    with pytest.raises(_lib.TipkError):
        _run(model, queries, 129, 'max')


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_routes_identical(kind):
    """Prefix reuse on and off and runs of 1, 3, 16 and 64 combinations give the same bits as the default; so does a relation
    count above the prefix rows' LDS budget (2 048), where the kernel reads every level."""
    g = torch.Generator().manual_seed(14)
    for n_rel in (300, 2049):
        model = _model(kind, n_rel, g)
        queries = cases.mixed_queries(10, g) + [([1, 2], [[3, 4, 5], [6, 7], [8, 9, 10, -1]]), ([], [[11, 12]] * 4)]
        weights = cases.weights_for(n_rel, g).to(DEV)
        known = _known(cases.known_for(queries, n_rel, g))
        for agg in AGGS:
            ref = _run(model, queries, 6, agg, weights, known)
            check_combo_burden(model, queries, 6, agg, ref, _lim(), weights, known, what='%s routes R%d %s' % (kind, n_rel, agg))
            for no_prefix in (0, 1):
                for run in (1, 3, 16, 64):
                    with _route(no_prefix, run):
                        assert _same(ref, _run(model, queries, 6, agg, weights, known)), (n_rel, agg, no_prefix, run)


# ------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_repeatable_and_capturable(kind):
    g = torch.Generator().manual_seed(15)
    n_rel, k = 300, 10
    model = _model(kind, n_rel, g)
    queries = cases.mixed_queries(60, g)
    known = _known(cases.known_for(queries[:20], n_rel, g))
    weights = cases.weights_for(n_rel, g).to(DEV)
    plan = ops.combo_plan(*query_lists(queries), DEV)
    fn = ops.distmult_combo_burden if kind == 'distmult' else ops.pair_table_combo_burden
    pick = lambda r: (r[0], r[2], r[3])
    for agg in AGGS:
        a = pick(fn(model[1], model[2], plan, k, agg, weights, known))
        b = pick(fn(model[1], model[2], plan, k, agg, weights, known))
        assert _same(a, b), agg
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                     # the entry alone: three sequential launches
            c = pick(fn(model[1], model[2], plan, k, agg, weights, known))
        for x in c:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a, c), agg


# ------------------------------------------------------------------ what already ships
def test_two_fixed_drugs_under_max_are_the_pair_topk_logit():
    """S = 0, two fixed drugs, 'max', one-hot weights: B = sigma(the logit section 4d returns for that relation), within
    tau / 4 (the slope of sigma is at most 1/4)."""
    g = torch.Generator().manual_seed(16)
    n_rel, k = 65, 4
    for dim in (16, 64):
        model = _dev(cases.ac.mixed_dm(n_rel, dim, g))
        pairs = torch.stack([torch.randperm(N, generator=g)[:2] for _ in range(6)], 1)
        top_s, top_r = ops.distmult_pair_topk(model[1], model[2], pairs.to(DEV), k)
        queries = [(pairs[:, p].tolist(), []) for p in range(pairs.shape[1])]
        _, tau = logits64(model, pairs[0].to(DEV), pairs[1].to(DEV))
        for j in range(k):
            for p in range(pairs.shape[1]):
                r = int(top_r[p, j])
                onehot = torch.zeros(n_rel, device=DEV)
                onehot[r] = 1.0
                b = _run(model, [queries[p]], 0, 'max', onehot)[0]
                want = torch.sigmoid(top_s[p, j].double())
                assert abs(float(b[0].double() - want)) <= float(tau[p, r]) / 4, (dim, p, j)


def _model_of(model, sub=None):
    z = model.embeddings.detach()
    dec = model.decoder
    if model.decoder_kind == 'distmult':
        w = dec.weight.detach()
        return ('distmult', z, w if sub is None else w[sub])
    with torch.no_grad():                                                 # the tables as NNDecoder.forward forms them
        w1, w2 = (dec.w1_l2, dec.w2_l2) if sub is None else (dec.w1_l2[sub], dec.w2_l2[sub])
        s1 = ops.matmul(torch.relu(ops.matmul(z, dec.w1_l1)), w1.t())
        s2 = ops.matmul(torch.relu(ops.matmul(z, dec.w2_l1)), w2.t())
    return ('table', s1, s2)


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_combination_risk(decoder):
    from tip_amd.layers import TIP, CombinationRisk, Setting
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None, decoder=decoder)    # the bundled graph
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    lim = _lim()
    m = _model_of(model)
    g = torch.Generator().manual_seed(17)
    p = torch.randperm(n, generator=g).tolist()
    u, v = int(d.dd_train_idx[0, 0]), int(d.dd_train_idx[1, 0])          # a recorded pair
    others = [x for x in p if x not in (u, v)]
    slots = [[[others[0], others[1], u], [others[2], v, -1]], [[others[3]], [others[4], others[5]], [others[6], -1]], []]
    fixed = [[others[7]], [others[8], others[9]], [u, v, others[10]]]
    queries = [(f, s) for f, s in zip(fixed, slots)]
    weights = (3 * torch.rand(R, generator=g)).tolist()
    lists = {None: None, 'train': ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n),
             'all': ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n, extra=(d.dd_test_idx, d.dd_test_range))}
    k = 4
    for agg in AGGS:
        for exclude in (None, 'all'):
            for w in (None, weights):
                res = model.combination_risk(slots, fixed=fixed, k=k, aggregate=agg, weights=w, exclude=exclude)
                assert isinstance(res, CombinationRisk) and res.burden.dtype == torch.float32
                assert res.ptr.dtype == torch.int64 and res.ptr.tolist() == [0, 9, 13, 14]
                assert res.best_combination.dtype == torch.int64 and res.best_drugs.shape == (3, k, 3)
                vals, pos = expected_selection(res.burden, res.ptr, k)
                assert torch.equal(res.best_combination, pos)
                wt = None if w is None else torch.tensor(w, dtype=torch.float32)
                check_combo_burden(m, queries, k, agg, (res.burden, res.best_burden, pos), lim, wt, lists[exclude],
                                   what='TIP %s %s %s' % (decoder, agg, exclude))
                # best_drugs decodes best_combination: the chosen drug per slot, -1 for an empty or missing slot and padding
                for q, (f, s) in enumerate(queries):
                    combos = list(itertools.product(*s))
                    for j in range(k):
                        c = int(res.best_combination[q, j])
                        want = [-1] * 3 if c < 0 else list(combos[c]) + [-1] * (3 - len(s))
                        assert res.best_drugs[q, j].tolist() == want, (q, j)
    # exclude='all' removes the recorded triples: the combination that takes the recorded pair (u, v) loses burden
    kept = model.combination_risk(slots, fixed=fixed, k=0).burden
    less = model.combination_risk(slots, fixed=fixed, k=0, exclude='all').burden
    at = list(itertools.product(*slots[0])).index((u, v))
    assert float(less[at]) < float(kept[at]) and float(less[13]) < float(kept[13])
    res0 = model.combination_risk(slots, fixed=fixed, k=0)
    assert res0.best_burden.shape == (3, 0) and res0.best_combination.shape == (3, 0) and res0.best_drugs.shape == (3, 0, 3)
    # relations=[...]: the burden counts the subset only, weights follow the subset
    sub = [4, 1, 5]
    res = model.combination_risk(slots, fixed=fixed, k=k, weights=[0.5, 2.0, 1.0], relations=sub)
    check_combo_burden(_model_of(model, torch.tensor(sub, device=DEV)), queries, k, 'noisy_or',
                       (res.burden, res.best_burden, res.best_combination), lim, torch.tensor([0.5, 2.0, 1.0]), None)
    # one combination with one-hot weights is the probability `regimen_side_effects` lists for that regimen, within the
    # two rules' tolerances: both are exp(-max(A64 - T_A, 0)) * T_A on the same A64 (the regimen rule's T_A is the smaller
    # by (S + 1) U A64), and torch evaluates the regimen's expm1 / sigmoid in fp32 (4 U P)
    reg = sorted([others[11], others[12], others[13], u])
    for agg in AGGS:
        listed = model.regimen_side_effects([reg], k=3, aggregate=agg, probability=True)
        for j in range(3):
            r = int(listed.relation[0, j])
            onehot = [0.0] * R
            onehot[r] = 1.0
            b = model.combination_risk([], fixed=reg, k=0, aggregate=agg, weights=onehot).burden
            t = spec_combo_burden(m, [(reg, [])], agg, lim, torch.tensor(onehot))
            tol = float(t['T_B'][0] + t['TP_w'][0] + 4 * U * t['B64'][0])
            assert abs(float(b[0]) - float(listed.score[0, j])) <= tol, (agg, j, float(b[0]), float(listed.score[0, j]), tol)
