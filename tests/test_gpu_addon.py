"""-m gpu: `tipk_distmult_addon_burden` / `tipk_pair_table_addon_burden` (include/tipk.h section 4i) and `TIP.add_on_risk`
against the fp64 acceptance rule of tests/addon_spec.py -- small shapes around the 64-relation lane groups and the relation
window with saturating and unsaturated inputs (tests/addon_cases.py), both rel_w routes, every context length class and bad
id, the persistent loop's second round, both candidate forms, k from 0 to 128, the known filter's corner cases, the logit
pinned to the pair top-k of section 4d, NaN and infinities, repeat runs and graph capture, and both decoder kinds of the
model face."""
import ctypes
import os

import pytest
import torch

import addon_cases as cases
from addon_cases import AGGS, N
from addon_spec import C_BURDEN, M_MAX, check_addon_burden, expected_selection
from pair_topk_spec import U, known_from_dict
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(model):
    return (model[0], model[1].to(DEV), model[2].to(DEV))


def _csr(lists):
    return tuple(t.to(DEV) for t in cases.csr(lists))


def _known(d, n=N):
    return tuple(t.to(DEV) for t in known_from_dict(d, n))


def _run(model, drugs, ptr, cand, cptr, k, agg, weights=None, known=None):
    fn = ops.distmult_addon_burden if model[0] == 'distmult' else ops.pair_table_addon_burden
    return fn(model[1], model[2], drugs, ptr, cand, cptr, k, agg, weights, known)


def _same(a, b):
    """Bit-equal results (NaN included)."""
    return all((x is None and y is None) or torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(a, b))


def _hold(model, ctx, cands, weights, kd, ks, what):
    model, weights = _dev(model), weights.to(DEV)
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr(cands)
    known = _known(kd)
    for agg in AGGS:
        for k in ks:
            for kn in (None, known):
                for w in (None, weights):
                    got = _run(model, drugs, ptr, cand, cptr, k, agg, w, kn)
                    check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, got, w, kn, what='%s %s k=%d' % (what, agg, k))


def _n_cu():
    n_cu = ctypes.c_int(0)
    assert _lib.lib().tipk_device_info(0, ctypes.byref(n_cu), None, None, None, 0) == 0
    return n_cu.value


# ------------------------------------------------------------------ lane and window edges
@pytest.mark.parametrize('recipe', ['mixed', 'unsat'])
@pytest.mark.parametrize('dim,n_rel', cases.DM_EDGES)
def test_distmult_lane_and_window_edges(dim, n_rel, recipe):
    _hold(*cases.edge_case('distmult', n_rel, dim, recipe), ks=[5], what='dm %s dim%d R%d' % (recipe, dim, n_rel))


@pytest.mark.parametrize('recipe', ['mixed', 'unsat'])
@pytest.mark.parametrize('n_rel', cases.TABLE_EDGES)
def test_table_lane_and_window_edges(n_rel, recipe):
    _hold(*cases.edge_case('table', n_rel, 0, recipe), ks=[5], what='table %s R%d' % (recipe, n_rel))


# ------------------------------------------------------------------ routes
def test_routes_identical():
    L = _lib.lib()
    route = L.tipk_distmult_addon_burden_lds_route
    assert _lib.get_option('addon_global') == 0
    # rel_w cannot fit LDS: the global route on its own, held to the rule on unsaturated inputs
    n_rel, dim, m = cases.DM_WIDE[0]
    assert (n_rel, dim) == (640, 64) and route(dim, n_rel) == 0
    g = torch.Generator().manual_seed(n_rel + dim)
    model = cases.unsat_dm(n_rel, dim, g)
    ctx, cands = cases.random_queries(12, g, lo=m, hi=m)
    _hold(model, ctx, cands, cases.weights_for(n_rel, g), cases.known_for(ctx, cands, n_rel, g), [5], 'dm global R640')
    # shapes that fit: both routes, all three outputs the same bits (dim 16 has a kernel of its own)
    for dim in (16, 32):
        n_rel = 300
        model, ctx, cands, weights, kd = cases.edge_case('distmult', n_rel, dim, 'mixed')
        model, weights, known = _dev(model), weights.to(DEV), _known(kd)
        drugs, ptr = _csr(ctx)
        cand, cptr = _csr(cands)
        assert route(dim, n_rel) == 1
        for agg in AGGS:
            a = _run(model, drugs, ptr, cand, cptr, 10, agg, weights, known)
            _lib.set_option('addon_global', 1)
            try:
                assert route(dim, n_rel) == 0
                b = _run(model, drugs, ptr, cand, cptr, 10, agg, weights, known)
            finally:
                _lib.set_option('addon_global', 0)
            assert _same(a, b), (dim, agg)
            check_addon_burden(model, drugs, ptr, cand, cptr, 10, agg, a, weights, known, what='dm routes dim%d' % dim)


# ------------------------------------------------------------------ contexts and bad ids
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_context_lengths_and_bad_ids_in_one_call(kind):
    """Contexts of 0, 1, 2, 3, 8, M_MAX and M_MAX + 1 drugs, a context with an id = n and one with -1, candidates inside
    their context, = n and = -1: NaN, never selected; every legal query's row is what the query gives alone."""
    g = torch.Generator().manual_seed(64)
    n_rel, k = 65, 6
    assert _lib.lib().tipk_addon_max_context() == M_MAX
    model = _dev(cases.mixed_dm(n_rel, 16, g) if kind == 'distmult' else cases.mixed_table(n_rel, g))
    perm = lambda m: torch.randperm(N, generator=g)[:m].tolist()
    bad = perm(5)
    bad[2] = N
    neg = perm(4)
    neg[1] = -1
    ctx = [[], perm(1), perm(2), perm(3), bad, perm(8), perm(M_MAX), neg, perm(M_MAX) + [0], perm(2)]
    legal = (1, 2, 3, 5, 6, 9)
    cands = []
    for q, c in enumerate(ctx):
        free = [x for x in perm(N) if x not in c][:9]                     # the M_MAX context leaves 6 drugs
        cands.append(free[:1] + [c[0] if c else 0] + free[1:3] + [N] + free[3:] + [-1])    # a member, n and -1 among them
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr(cands)
    known = _known(cases.known_for([ctx[q] for q in legal], [cands[q] for q in legal], n_rel, g))
    weights = cases.weights_for(n_rel, g).to(DEV)
    for agg in AGGS:
        for kn in (None, known):
            got = _run(model, drugs, ptr, cand, cptr, k, agg, weights, kn)
            check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, got, weights, kn, what='%s lengths' % kind)
            for q in range(len(ctx)):
                row = got[0][cptr[q]:cptr[q + 1]]
                if q not in legal:
                    assert bool(torch.isnan(row).all()) and bool((got[2][q] == -1).all()) and bool(torch.isposinf(got[1][q]).all())
                    continue
                off = [i for i, c in enumerate(cands[q]) if c in ctx[q] or c < 0 or c >= N]
                assert len(off) == 3 and torch.isnan(row).tolist() == [i in off for i in range(len(cands[q]))]
                assert not bool(torch.isin(got[2][q], torch.tensor(off, device=DEV)).any())
                alone = _run(model, *_csr([ctx[q]]), *_csr([cands[q]]), k, agg, weights, kn)
                assert _same((row, got[1][q], got[2][q]), (alone[0], alone[1][0], alone[2][0])), q


# ------------------------------------------------------------------ task counts, candidate forms
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_task_counts_and_second_round(kind):
    """0, 1, 16, 17 tasks (a workgroup takes 16), and one more than the wavefronts of the largest grid the entries launch
    (two workgroups of 16 per CU), so the persistent loop takes another round; one-drug contexts, R = 65."""
    g = torch.Generator().manual_seed(17)
    n_rel, k = 65, 3
    model = _dev(cases.unsat_dm(n_rel, 16, g) if kind == 'distmult' else cases.unsat_table(n_rel, g))
    drugs, ptr = _csr([[3]])
    for count in (0, 1, 16, 17, 16 * 2 * _n_cu() + 1):
        cand = torch.randint(0, N, (count,), generator=g).to(torch.int32).to(DEV)
        for agg in AGGS:
            got = _run(model, drugs, ptr, cand, None, k, agg)
            assert got[0].shape == (1, count) and got[1].shape == (1, k)
            check_addon_burden(model, drugs, ptr, cand, None, k, agg, got, what='%s count %d' % (kind, count))
            if count == 0:
                assert bool(torch.isinf(got[1]).all()) and bool((got[2] == -1).all())


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_shared_list_is_the_repeated_csr_list(kind):
    g = torch.Generator().manual_seed(5)
    n_rel, k = 130, 4
    model = _dev(cases.mixed_dm(n_rel, 16, g) if kind == 'distmult' else cases.mixed_table(n_rel, g))
    ctx, _ = cases.random_queries(21, g)
    shared = torch.randint(0, N, (37,), generator=g).tolist()
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr([shared] * len(ctx))
    weights = cases.weights_for(n_rel, g).to(DEV)
    known = _known(cases.known_for(ctx, [shared] * len(ctx), n_rel, g))
    for agg in AGGS:
        a = _run(model, drugs, ptr, cand[:37].contiguous(), None, k, agg, weights, known)
        b = _run(model, drugs, ptr, cand, cptr, k, agg, weights, known)
        assert a[0].shape == (len(ctx), 37) and b[0].shape == (len(ctx) * 37,)
        assert _same((a[0].reshape(-1), a[1], a[2]), b), agg
        check_addon_burden(model, drugs, ptr, cand[:37], None, k, agg, a, weights, known, what='%s shared' % kind)


# ------------------------------------------------------------------ k
def test_k_values():
    """k = 0 (best outputs None), 1, C, C + 3 (padding) and 128; k = 129 is refused; repeated candidate ids come back in
    position order; a query whose tasks are all NaN has a fully padded row."""
    g = torch.Generator().manual_seed(200)
    n_rel, C = 65, 60
    for model in (cases.mixed_dm(n_rel, 16, g), cases.mixed_table(n_rel, g)):
        ctx, cands = cases.random_queries(30, g, n_cand=C)
        _hold(model, ctx, cands, cases.weights_for(n_rel, g), {}, [0, 1, C, C + 3, 128], '%s k' % model[0])
        big = [torch.randint(0, N, (300,), generator=g).tolist() for _ in ctx[:6]]     # more candidates than k = 128
        _hold(model, ctx[:6], big, cases.weights_for(n_rel, g), {}, [128], '%s k 128' % model[0])
        model = _dev(model)
        drugs, ptr = _csr(ctx)
        cand, cptr = _csr(cands)
        got = _run(model, drugs, ptr, cand, cptr, 0, 'max')
        assert got[1] is None and got[2] is None
        with pytest.raises(_lib.TipkError, match='unsupported'):
            _run(model, drugs, ptr, cand, cptr, 129, 'max')
        # repeated ids: equal burdens, returned in position order; the all-NaN query (every candidate a member): padding
        rep = [[7, 9, 7, 7, 9, 11, 7], [20, 21, 20]]
        drugs, ptr = _csr([[1, 2, 3], [20, 21]])
        cand, cptr = _csr(rep)
        for agg in AGGS:
            b, bb, bp = _run(model, drugs, ptr, cand, cptr, 7, agg)
            check_addon_burden(model, drugs, ptr, cand, cptr, 7, agg, (b, bb, bp), what='repeats')
            assert b[0] == b[2] == b[3] == b[6] and b[1] == b[4]
            order = bp[0].tolist()
            assert [p for p in order if p in (0, 2, 3, 6)] == [0, 2, 3, 6] and [p for p in order if p in (1, 4)] == [1, 4]
            assert bool(torch.isnan(b[7:]).all()) and bp[1].tolist() == [-1] * 7 and bool(torch.isposinf(bb[1]).all())


# ------------------------------------------------------------------ known filter
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_known_filter_cases(kind):
    g = torch.Generator().manual_seed(300)
    n_rel, k = 700, 5
    model = _dev(cases.unsat_dm(n_rel, 16, g) if kind == 'distmult' else cases.unsat_table(n_rel, g))
    ctx = [[4, 9, 20, 31], [40, 41], [50, 51, 52]]
    cands = [[1, 2, 60], [3, 42], [5, 6]]
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr(cands)
    gone = 300                                                            # a relation of the second window
    d = {}
    for i, s in enumerate(ctx[0]):                                        # candidate 1: `gone` known for every context drug,
        d[(1, s) if i % 2 else (s, 1)] = [gone]                           # listed in either pair direction
        d[(s, 2) if i % 2 else (2, s)] = list(range(100, n_rel))          # candidate 2: long blocks over three windows
    d[(3, 40)] = list(range(n_rel))                                       # every triple of one context drug known
    d[(41, 3)] = [0, n_rel - 1]
    d[(60, 61)] = [0, 5]                                                  # keys of pairs that occur nowhere
    d[(0, 0)] = [1]
    d[(N - 1, N - 1)] = [2]
    known = _known(d)
    weights = cases.weights_for(n_rel, g).to(DEV)
    w0 = weights.clone()
    w0[gone] = 0.0
    for agg in AGGS:
        for w in (None, weights):
            got = _run(model, drugs, ptr, cand, cptr, k, agg, w, known)
            check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, got, w, known, what='%s known' % kind)
            plain = _run(model, drugs, ptr, cand, cptr, k, agg, w)
            assert bool((got[0][[0, 1, 3]] < plain[0][[0, 1, 3]]).all())
            assert _same((got[0][[2, 4, 5, 6]],), (plain[0][[2, 4, 5, 6]],))       # tasks without a known pair
        # a relation known for every context drug of the task = that relation's weight set to 0: adding +0.0 is exact
        a = _run(model, drugs, ptr, cand, cptr, k, agg, weights, known)
        b = _run(model, drugs, ptr, cand, cptr, k, agg, w0, known)
        c = _run(model, drugs, ptr, cand, cptr, k, agg, w0)
        assert _same((a[0][:1],), (b[0][:1],)) and _same((a[0][:1],), (c[0][:1],)), agg
        assert not bool(torch.isnan(a[0]).any())


# ------------------------------------------------------------------ the logit is that of section 4d
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_logit_pinned_to_the_pair_topk(kind):
    """One-hot weights e_r, one-drug contexts, max: B = sigma(the 4d logit of (c, s, r)) within C_BURDEN roundings."""
    g = torch.Generator().manual_seed(41)
    n_rel, Q, C = 6, 12, 9
    model = _dev(cases.mixed_dm(n_rel, 16, g) if kind == 'distmult' else cases.mixed_table(n_rel, g))
    s = torch.randint(0, N, (Q,), generator=g)
    cand = torch.randint(0, N, (Q, C), generator=g)
    cand[cand == s[:, None]] = N - 1 - s[:, None].expand(-1, C)[cand == s[:, None]]     # no member among the candidates
    assert bool((cand != s[:, None]).all())
    cs = s[:, None].expand(-1, C)
    pairs = torch.stack([torch.minimum(cand, cs).reshape(-1), torch.maximum(cand, cs).reshape(-1)]).to(DEV)
    topk = ops.distmult_pair_topk if kind == 'distmult' else ops.pair_table_pair_topk
    logit, rel = topk(model[1], model[2], pairs, n_rel)
    by_rel = torch.empty_like(logit).scatter_(1, rel.long(), logit)      # [Q * C, R] fp32 logits of section 4d
    drugs, ptr = s.to(torch.int32).to(DEV), torch.arange(Q + 1, device=DEV)
    flat, cptr = cand.reshape(-1).to(torch.int32).to(DEV), C * torch.arange(Q + 1, device=DEV)
    for r in range(n_rel):
        e = torch.zeros(n_rel, device=DEV)
        e[r] = 1.0
        b = _run(model, drugs, ptr, flat, cptr, 0, 'max', e)[0]
        p64 = torch.sigmoid(by_rel[:, r].double())
        assert bool(((b.double() - p64).abs() <= C_BURDEN * U * p64).all()), (kind, r)
    # (c, s) and (s, c) are one pair: the same bits with the roles swapped (the table logit takes u = min either way)
    first = flat[::C].contiguous()
    b1 = _run(model, drugs, ptr, first, ptr, 0, 'noisy_or')[0]
    b2 = _run(model, first, ptr, drugs, ptr, 0, 'noisy_or')[0]
    assert _same((b1,), (b2,)) and not bool(torch.isnan(b1).any())


# ------------------------------------------------------------------ specials
def test_nan_and_infinities():
    g = torch.Generator().manual_seed(13)
    n_rel, k = 130, 8
    kind, z, w = cases.mixed_dm(n_rel, 16, g)
    z[7, 3] = float('nan')                                                # every triple through drug 7 is NaN
    model = _dev((kind, z, w))
    ctx = [[7, 2], [2, 12], [12], [7]]
    cands = [[1, 3, 5], [7, 1, 3, 5, 7], [7, 4], [1, 2]]
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr(cands)
    weights = torch.zeros(n_rel, device=DEV)                              # the NaN rule holds under a weight of 0 too
    for agg in AGGS:
        for wts in (None, weights):
            b, bb, bp = _run(model, drugs, ptr, cand, cptr, k, agg, wts)
            check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, (b, bb, bp), wts, what='nan')
            assert torch.isnan(b).tolist() == [True] * 3 + [True, False, False, False, True] + [True, False] + [True] * 2
            assert bp[0].tolist() == [-1] * k and bp[3].tolist() == [-1] * k and sorted(bp[1, :3].tolist()) == [1, 2, 3]
            assert not bool(torch.isnan(bb).any())
        # known for the pair: the NaN triples contribute nothing and the task is applicable again
        known = _known({(7, 12): range(n_rel)})
        b, bb, bp = _run(model, drugs, ptr, cand, cptr, k, agg, None, known)
        check_addon_burden(model, drugs, ptr, cand, cptr, k, agg, (b, bb, bp), None, known, what='nan known')
        assert float(b[8]) == 0.0 and bp[2, 0] == 0
    # infinities in the tables: +inf gives P = 1, -inf gives 0, inf - inf is a NaN
    s1, s2 = torch.randn(N, 40, generator=g), torch.randn(N, 40, generator=g)
    s1[3, 10], s1[3, 11], s2[4, 11] = float('inf'), float('-inf'), 0.5
    s1[5, 12], s2[6, 12] = float('inf'), float('-inf')
    model = _dev(('table', s1, s2))
    drugs, ptr = _csr([[3], [3, 8], [5], [6, 9]])
    cand, cptr = _csr([[4, 9], [4], [6, 9], [5, 3]])
    for agg in AGGS:
        got = _run(model, drugs, ptr, cand, cptr, 2, agg)
        check_addon_burden(model, drugs, ptr, cand, cptr, 2, agg, got, what='inf')
        assert torch.isnan(got[0]).tolist() == [False, False, False, True, False, True, False]
        for r, want in ((10, 1.0), (11, 0.0)):
            e = torch.zeros(40, device=DEV)
            e[r] = 1.0
            b = _run(model, drugs, ptr, cand, cptr, 0, agg, e)[0]
            assert float(b[0]) == want and float(b[1]) == want           # (3, 4) and (3, 9): 3 is the first argument
        e = torch.zeros(40, device=DEV)
        e[11] = 1.0
        b = _run(model, drugs, ptr, cand, cptr, 0, agg, e)[0]             # -inf beside a finite logit of (4, 8)
        p = torch.sigmoid(model[1][4, 11].double() + model[2][8, 11].double())
        assert abs(float(b[2]) - float(p)) <= 64 * U * float(p)


# ------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_repeatable_and_capturable(kind):
    g = torch.Generator().manual_seed(77)
    n_rel, k = 300, 10
    model = _dev(cases.mixed_dm(n_rel, 16, g) if kind == 'distmult' else cases.mixed_table(n_rel, g))
    ctx, cands = cases.random_queries(100, g, hi=12)
    drugs, ptr = _csr(ctx)
    cand, cptr = _csr(cands)
    known = _known(cases.known_for(ctx[:20], cands[:20], n_rel, g))
    weights = cases.weights_for(n_rel, g).to(DEV)
    for agg in AGGS:
        a = _run(model, drugs, ptr, cand, cptr, k, agg, weights, known)
        b = _run(model, drugs, ptr, cand, cptr, k, agg, weights, known)
        assert _same(a, b), agg
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                     # the single entry alone: two sequential launches
            c = _run(model, drugs, ptr, cand, cptr, k, agg, weights, known)
        for x in c:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a, c), agg


# ------------------------------------------------------------------ TIP.add_on_risk
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


def _pair_dict(idx, rng, d=None):
    d = {} if d is None else d
    idx = idx.cpu().tolist()
    for r, (a, b) in enumerate(torch.as_tensor(rng).long().tolist()):
        for u, v in zip(idx[0][a:b], idx[1][a:b]):
            d.setdefault((min(u, v), max(u, v)), set()).add(r)
    return d


def _check_risk(res, m, regs, candidates, replace, n, k, agg, weights, known, what):
    from tip_amd.layers import normalize_add_on_queries
    nd, nptr, cand, cptr = normalize_add_on_queries(regs, candidates, replace, n, M_MAX)
    G = nptr.numel() - 1
    assert res.burden.dtype == torch.float32 and res.candidate.dtype == torch.int64 and res.best_drug.dtype == torch.int64
    assert res.best_burden.shape == (G, k) and res.best_drug.shape == (G, k) and res.ptr.shape == (G + 1,)
    if cptr is None:
        assert res.burden.numel() == G * cand.numel() and torch.equal(res.candidate.cpu(), cand.long().repeat(G))
        assert res.ptr.tolist() == [g * cand.numel() for g in range(G + 1)]
    else:
        assert torch.equal(res.candidate.cpu(), cand.long()) and torch.equal(res.ptr.cpu(), cptr)
    vals, pos = expected_selection(res.burden, res.ptr, k)
    lookup = res.candidate if res.candidate.numel() else torch.zeros(1, dtype=torch.int64, device=DEV)
    want = torch.where(pos >= 0, lookup[(res.ptr[:-1, None] + pos).clamp(min=0, max=lookup.numel() - 1)], pos)
    assert torch.equal(res.best_drug, want), 'best_drug is not candidate[ptr + position]'
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32)
    check_addon_burden(m, nd, nptr, cand, cptr, k, agg, (res.burden, res.best_burden if k else None, pos if k else None), w,
                       known, what=what)
    return nd, nptr


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_add_on_risk(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    train_d = _pair_dict(d.dd_train_idx, d.dd_train_range)
    both_d = _pair_dict(d.dd_test_idx, d.dd_test_range, _pair_dict(d.dd_train_idx, d.dd_train_range))
    lists = {None: None, 'train': _known(train_d, n), 'all': _known(both_d, n)}
    g = torch.Generator().manual_seed(4)
    regs = [list(p) for p in sorted(train_d)[:6]]
    regs += [torch.randperm(n, generator=g)[:int(torch.randint(1, min(9, n) + 1, (1,), generator=g))].tolist()
             for _ in range(20)] + [[], [3], [5, 2, 5, 2]]
    G = len(regs)
    m = _model_of(model)
    k = 5
    weights = (3 * torch.rand(R, generator=g)).tolist()
    shared = torch.randperm(n, generator=g)[:min(n, 12)].tolist()
    per_reg = [torch.randint(0, n, (int(torch.randint(0, 8, (1,), generator=g)),), generator=g).tolist() for _ in regs]
    for agg in AGGS:
        for exclude in (None, 'train', 'all'):
            for candidates, w in ((None, None), (shared, weights), (per_reg, weights)):
                res = model.add_on_risk(regs, candidates=candidates, k=k, aggregate=agg, weights=w, exclude=exclude)
                _check_risk(res, m, regs, candidates, None, n, k, agg, w, lists[exclude],
                            'TIP %s %s %s' % (decoder, agg, exclude))
    # candidates None: every drug; the members of a regimen come back NaN and are never chosen
    rows = model.add_on_risk(regs, k=k).burden.view(G, n)
    member = torch.zeros((G, n), dtype=torch.bool, device=DEV)
    for q, reg in enumerate(regs):
        member[q, reg] = True
    empty = torch.tensor([len(r) == 0 for r in regs], device=DEV)
    assert torch.equal(torch.isnan(rows), member | empty[:, None])
    res0 = model.add_on_risk(regs, candidates=shared, k=0)
    assert res0.best_burden.shape == (G, 0) and res0.best_drug.shape == (G, 0)
    _check_risk(res0, m, regs, shared, None, n, 0, 'noisy_or', None, None, 'TIP k=0')
    # replace: the context loses the drug, and the drug is scorable as a candidate (the baseline)
    replace = [reg[0] if len(set(reg)) > 1 else -1 for reg in regs]
    res = model.add_on_risk(regs, candidates=None, k=k, replace=replace, exclude='train', weights=weights)
    nd, nptr = _check_risk(res, m, regs, None, replace, n, k, 'noisy_or', weights, lists['train'], 'TIP replace')
    rows = res.burden.view(G, n)
    for q, rep in enumerate(replace):
        if rep >= 0:
            assert rep not in nd[nptr[q]:nptr[q + 1]].tolist() and not bool(torch.isnan(rows[q, rep]))
    kept = model.add_on_risk(regs, candidates=None, k=k, exclude='train', weights=weights).burden.view(G, n)
    assert all(bool(torch.isnan(kept[q, rep])) for q, rep in enumerate(replace) if rep >= 0)
    # relations=[...]: the burden counts the subset only, weights follow the subset, the filter follows
    sub = [4, 1, 5]
    sub_t = torch.tensor(sub, device=DEV)
    res = model.add_on_risk(regs, candidates=shared, k=k, weights=[0.5, 2.0, 1.0], relations=sub, exclude='train')
    sub_known = known_from_dict({p: [sub.index(r) for r in rs if r in sub] for p, rs in train_d.items()}, n)
    _check_risk(res, _model_of(model, sub_t), regs, shared, None, n, k, 'noisy_or', [0.5, 2.0, 1.0],
                tuple(t.to(DEV) for t in sub_known), 'TIP %s subset' % decoder)
