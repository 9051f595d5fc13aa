"""-m gpu: `tipk_distmult_regimen_topk` / `tipk_pair_table_regimen_topk` (include/tipk.h section 4e) and
`TIP.regimen_side_effects` against the fp64 acceptance rule of tests/regimen_spec.py -- small shapes around the 64-relation
lane groups and the relation window, both rel_w routes, every regimen length class, the persistent loop's second round, the
bit-for-bit cross-check with the pair top-k of section 4d, the known filter's corner cases, ties, zeros, NaN and infinities,
repeat runs and graph capture, and both decoder kinds of the model face."""
import os

import pytest
import torch

from pair_topk_spec import check_pair_topk, known_from_dict, logits64
from regimen_spec import M_MAX, check_regimen_topk
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 70
WINDOW = 256                                   # relations per window of the kernel (64 lanes x 4)
AGGS = ('max', 'noisy_or')


def _csr(lists):
    ptr = [0]
    for g in lists:
        ptr.append(ptr[-1] + len(g))
    return (torch.tensor([x for g in lists for x in g], dtype=torch.int32, device=DEV),
            torch.tensor(ptr, dtype=torch.int64, device=DEV))


def _random_lists(count, g, lo=2, hi=9, n=N):
    """`count` regimens of distinct drugs in random (unsorted) order, lengths uniform in [lo, hi]."""
    return [torch.randperm(n, generator=g)[:int(torch.randint(lo, hi + 1, (1,), generator=g))].tolist() for _ in range(count)]


def _known_for(lists, n_rel, g, n=N, share=0.3):
    """Random known relations for about half the pairs of `lists` (listed in either direction), plus keys of pairs that
    occur in no regimen."""
    d = {}
    for lst in lists:
        for a in range(len(lst)):
            for b in range(a + 1, len(lst)):
                if float(torch.rand(1, generator=g)) < 0.5:
                    rels = torch.nonzero(torch.rand(n_rel, generator=g) < share).reshape(-1).tolist()
                    d[(lst[b], lst[a]) if a % 2 else (lst[a], lst[b])] = rels
    for u, v in torch.randint(0, n, (30, 2), generator=g).tolist():
        d.setdefault((u, v), [0, n_rel - 1])
    return tuple(t.to(DEV) for t in known_from_dict(d, n))


def _run(model, drugs, ptr, k, agg, known=None):
    if model[0] == 'distmult':
        return ops.distmult_regimen_topk(model[1], model[2], drugs, ptr, k, agg, known)
    return ops.pair_table_regimen_topk(model[1], model[2], drugs, ptr, k, agg, known)


def _dm(n_rel, dim, g, n=N):
    return ('distmult', (torch.randn(n, dim, generator=g) / dim ** 0.25).to(DEV),
            (torch.randn(n_rel, dim, generator=g) / dim ** 0.25).to(DEV))


def _tb(n_rel, g, n=N):
    wide = torch.randn(2, n, n_rel + 5, generator=g).to(DEV)            # row stride n_rel + 5
    return ('table', wide[0, :, :n_rel], wide[1, :, :n_rel])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _hold(model, lists, n_rel, g, ks, what):
    drugs, ptr = _csr(lists)
    known = _known_for(lists, n_rel, g)
    for agg in AGGS:
        for k in ks:
            for kn in (None, known):
                got = _run(model, drugs, ptr, k, agg, kn)
                check_regimen_topk(model, drugs, ptr, k, agg, got, kn, what='%s %s k=%d' % (what, agg, k))


# ------------------------------------------------------------------ lane and window edges
@pytest.mark.parametrize('dim,n_rel', [(16, 1), (16, 63), (16, 64), (16, 65), (16, 130), (8, 65), (20, 65), (4, WINDOW + 1),
                                       (16, WINDOW + 1)])
def test_distmult_lane_and_window_edges(dim, n_rel):
    g = torch.Generator().manual_seed(100 * n_rel + dim)
    _hold(_dm(n_rel, dim, g), _random_lists(40, g), n_rel, g, sorted({1, min(n_rel, 10)}), 'dm dim%d R%d' % (dim, n_rel))


@pytest.mark.parametrize('n_rel', [1, 64, 65, WINDOW + 1])
def test_table_lane_and_window_edges(n_rel):
    g = torch.Generator().manual_seed(7 * n_rel)
    _hold(_tb(n_rel, g), _random_lists(40, g), n_rel, g, sorted({1, min(n_rel, 10)}), 'table R%d' % n_rel)


# ------------------------------------------------------------------ routes
def test_routes_identical():
    g = torch.Generator().manual_seed(2500)
    L = _lib.lib()
    assert _lib.get_option('regimen_global') == 0
    lists = _random_lists(50, g)
    # rel_w cannot fit LDS: the global route on its own
    assert L.tipk_distmult_regimen_topk_lds_route(64, 2500) == 0
    _hold(_dm(2500, 64, g), lists, 2500, g, [10], 'dm global R2500')
    # shapes that fit: both routes, all three outputs the same bits (dim 16 has a kernel of its own)
    for dim in (16, 32):
        n_rel = 300
        model = _dm(n_rel, dim, g)
        drugs, ptr = _csr(lists)
        known = _known_for(lists, n_rel, g)
        assert L.tipk_distmult_regimen_topk_lds_route(dim, n_rel) == 1
        for agg in AGGS:
            a = _run(model, drugs, ptr, 10, agg, known)
            _lib.set_option('regimen_global', 1)
            try:
                assert L.tipk_distmult_regimen_topk_lds_route(dim, n_rel) == 0
                b = _run(model, drugs, ptr, 10, agg, known)
            finally:
                _lib.set_option('regimen_global', 0)
            assert _same(a, b), (dim, agg)
            check_regimen_topk(model, drugs, ptr, 10, agg, a, known, what='dm routes dim%d' % dim)


# ------------------------------------------------------------------ regimen sizes
def _n_cu():
    import ctypes
    n_cu = ctypes.c_int(0)
    assert _lib.lib().tipk_device_info(0, ctypes.byref(n_cu), None, None, None, 0) == 0
    return n_cu.value


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_regimen_lengths_in_one_call(kind):
    """Lengths 0, 1, 2, 3, 8, M_MAX and M_MAX + 1 in one call, and a regimen with an out-of-range id in the middle of its
    list: the illegal ones get padded rows, their neighbours' rows are what they are alone."""
    g = torch.Generator().manual_seed(64)
    n_rel, k = 65, 6
    assert _lib.lib().tipk_regimen_max_drugs() == M_MAX
    model = _dm(n_rel, 16, g) if kind == 'distmult' else _tb(n_rel, g)
    perm = lambda m: torch.randperm(N, generator=g)[:m].tolist()
    bad = perm(5)
    bad[2] = N
    neg = perm(4)
    neg[1] = -1
    lists = [[], perm(1), perm(2), perm(3), bad, perm(8), perm(M_MAX), neg, perm(M_MAX) + [0], perm(2)]
    drugs, ptr = _csr(lists)
    known = _known_for([l for l in lists if l and max(l) < N and min(l) >= 0], n_rel, g)
    for agg in AGGS:
        for kn in (None, known):
            got = _run(model, drugs, ptr, k, agg, kn)
            check_regimen_topk(model, drugs, ptr, k, agg, got, kn, what='%s lengths' % kind)
            for row in (0, 1, 4, 7, 8):
                assert bool((got[1][row] == -1).all()) and bool(torch.isneginf(got[0][row]).all())
                assert bool((got[2][row] == -1).all()) and bool((got[3][row] == -1).all())
            for row in (2, 3, 5, 6, 9):
                alone = _run(model, *_csr([lists[row]]), k, agg, kn)
                assert all(torch.equal(x[row], y[0]) for x, y in zip(got, alone)), row


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_regimen_counts_and_second_round(kind):
    """n_regimens in {0, 1, 16, 17} (a workgroup takes 16), and one more than 16 x the largest grid the entries launch (two
    workgroups per CU), so the persistent loop takes another round; length-2 regimens, R = 65."""
    g = torch.Generator().manual_seed(17)
    n_rel, k = 65, 3
    model = _dm(n_rel, 16, g) if kind == 'distmult' else _tb(n_rel, g)
    for count in (0, 1, 16, 17, 16 * 2 * _n_cu() + 1):
        pairs = torch.randint(0, N, (count, 2), generator=g)
        drugs = pairs.reshape(-1).to(torch.int32).to(DEV)
        ptr = (2 * torch.arange(count + 1)).to(DEV)
        for agg in AGGS:
            got = _run(model, drugs, ptr, k, agg)
            assert got[0].shape == (count, k)
            check_regimen_topk(model, drugs, ptr, k, agg, got, what='%s count %d' % (kind, count))


# ------------------------------------------------------------------ cross-check with the pair top-k
@pytest.mark.parametrize('dim', [16, 8])
def test_length_two_max_is_the_pair_topk(dim):
    g = torch.Generator().manual_seed(2)
    n_rel, k = 130, 20
    pairs = torch.cat([torch.tensor([[3, 7], [7, 3], [5, 5]]), torch.randint(0, N, (300, 2), generator=g)])
    drugs = pairs.reshape(-1).to(torch.int32).to(DEV)
    ptr = (2 * torch.arange(pairs.shape[0] + 1)).to(DEV)
    known = _known_for(pairs.tolist(), n_rel, g)
    pt = pairs.t().contiguous().to(DEV)
    dm, tb = _dm(n_rel, dim, g), _tb(n_rel, g)
    for kn in (None, known):
        s, r, pi, pj = ops.distmult_regimen_topk(dm[1], dm[2], drugs, ptr, k, 'max', kn)
        ws, wr = ops.distmult_pair_topk(dm[1], dm[2], pt, k, kn)
        assert torch.equal(s, ws) and torch.equal(r, wr)
        assert bool(((pi == 0) & (pj == 1))[r >= 0].all())
        s, r, pi, pj = ops.pair_table_regimen_topk(tb[1], tb[2], drugs, ptr, k, 'max', kn)
        ws, wr = ops.pair_table_pair_topk(tb[1], tb[2], pt, k, kn)
        assert torch.equal(s, ws) and torch.equal(r, wr)


# ------------------------------------------------------------------ k
def test_k_values():
    """k in {1, 128} at R = 200; k = R and k = R + 3 (padding) at R = 100, the entry ranking at most 128 relations: k = 200
    is refused."""
    g = torch.Generator().manual_seed(200)
    lists = _random_lists(30, g)
    for n_rel, ks in ((200, (1, 128)), (100, (100, 103))):
        _hold(_dm(n_rel, 16, g), lists, n_rel, g, ks, 'dm k R%d' % n_rel)
        _hold(_tb(n_rel, g), lists, n_rel, g, ks, 'table k R%d' % n_rel)
    model = _dm(200, 16, g)
    for k in (200, 203):
        with pytest.raises(_lib.TipkError, match='unsupported'):
            _run(model, *_csr(lists), k, 'max')
    got = _run(model, *_csr(lists), 103, 'noisy_or')
    assert bool((got[1] >= 0).all())


# ------------------------------------------------------------------ known filter
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_known_filter_cases(kind):
    g = torch.Generator().manual_seed(300)
    n_rel, k = 700, 128
    model = _dm(n_rel, 16, g) if kind == 'distmult' else _tb(n_rel, g)
    reg = [4, 9, 20, 31]
    pairs = [(reg[a], reg[b]) for a in range(4) for b in range(a + 1, 4)]
    drugs, ptr = _csr([reg, [40, 41], [50, 51, 52]])
    # relations 100 .. 699 are known for every pair of regimen 0 (blocks of 600: a long cursor over three windows), so its
    # 100 candidates all fit into k = 128 rows and none can drop out of the result below
    base = {p: range(100, n_rel) for p in pairs}
    free = _run(model, drugs, ptr, k, 'max', tuple(t.to(DEV) for t in known_from_dict(base, N)))
    assert int((free[1][0] >= 0).sum()) == 100
    top_r, top_i, top_j = int(free[1][0, 0]), int(free[2][0, 0]), int(free[3][0, 0])
    second_r = int(free[1][0, 1])
    best_pair = (reg[top_i], reg[top_j])
    d = {p: [second_r] + list(range(100, n_rel)) for p in pairs}          # known for every pair of the regimen: absent
    d[(best_pair[1], best_pair[0])] = sorted({second_r, top_r} | set(range(100, n_rel)))   # listed in the other direction
    d[(40, 41)] = range(n_rel)                                            # every triple of regimen 1 known: a padded row
    d[(60, 61)] = [0, 5]                                                  # keys of pairs in no regimen
    d[(0, 0)] = [1]
    d[(N - 1, N - 1)] = [2]
    known = tuple(t.to(DEV) for t in known_from_dict(d, N))
    for agg in AGGS:
        got = _run(model, drugs, ptr, k, agg, known)
        check_regimen_topk(model, drugs, ptr, k, agg, got, known, what='%s known' % kind)
        assert second_r not in got[1][0].tolist()
        assert bool((got[1][1] == -1).all()) and bool(torch.isneginf(got[0][1]).all())
        plain = _run(model, drugs, ptr, k, agg)
        assert all(torch.equal(x[2], y[2]) for x, y in zip(got, plain))   # regimen 2 has no known pair
    got = _run(model, drugs, ptr, k, 'max', known)
    at = got[1][0].tolist().index(top_r)                                  # known for the best pair only: still there,
    assert (int(got[2][0, at]), int(got[3][0, at])) != (top_i, top_j)     # with another driver and a lower score
    assert float(got[0][0, at]) < float(free[0][0, 0])


# ------------------------------------------------------------------ ties and specials
def test_ties_zeros_nan_and_infinities():
    g = torch.Generator().manual_seed(13)
    n_rel, dim, k = 130, 16, 128
    z = torch.randn(N, dim, generator=g)
    w = torch.randn(13, dim, generator=g)[torch.arange(n_rel) % 13].contiguous()    # every row occurs 10 times
    lists = _random_lists(30, g)
    drugs, ptr = _csr(lists)
    model = ('distmult', z.to(DEV), w.to(DEV))
    for agg in AGGS:
        s, r, pi, pj = _run(model, drugs, ptr, k, agg)
        check_regimen_topk(model, drugs, ptr, k, agg, (s, r, pi, pj), what='ties')
        run = (r[:, 1:] % 13) == (r[:, :-1] % 13)                         # neighbours from one group of equal rows
        assert bool((s[:, 1:][run] == s[:, :-1][run]).all()) and bool((r[:, 1:][run] > r[:, :-1][run]).all())
        assert int(run.sum()) >= len(lists) * (k - 14) * 0.9
    # an all-zero z row: +-0 logits for every pair through drug 5; the order stays total (zeros tie by relation id)
    z0 = z.clone()
    z0[5] = 0.0
    zero_lists = [[5, 9], [9, 5, 11], [5, 5]] + lists[:5]
    model = ('distmult', z0.to(DEV), torch.randn(n_rel, dim, generator=g).to(DEV))
    for agg in AGGS:
        got = _run(model, *_csr(zero_lists), k, agg)
        check_regimen_topk(model, *_csr(zero_lists), k, agg, got, what='zeros')
        assert got[1][0].tolist() == list(range(k)) and bool((got[0][0] == (0.0 if agg == 'max' else got[0][0, 0])).all())
    # one NaN in z: triples through drug 7 are skipped, no NaN comes back, and a regimen of 7 plus one other is padded
    zn = z.clone()
    zn[7, 3] = float('nan')
    nan_lists = [[7, 2], [2, 7, 12], [12, 2], [7, 7]] + lists[:5]
    model = ('distmult', zn.to(DEV), model[2])
    for agg in AGGS:
        got = _run(model, *_csr(nan_lists), k, agg)
        check_regimen_topk(model, *_csr(nan_lists), k, agg, got, what='nan')
        assert not bool(torch.isnan(got[0]).any())
        assert bool((got[1][0] == -1).all()) and bool((got[1][3] == -1).all())
        assert _same([x[1] for x in got[:2]], [x[2] for x in got[:2]])    # (2, 7, 12) ranks as (12, 2) alone does ...
        assert bool(((got[2][1] == 0) & (got[3][1] == 2)).all())          # ... through its positions 0 and 2
    # infinities in the tables: softplus(-inf) contributes 0, +inf ranks first, inf - inf is a NaN and is skipped
    s1, s2 = torch.randn(N, 40, generator=g), torch.randn(N, 40, generator=g)
    s1[3, 10], s1[3, 11], s2[4, 11], s1[3, 12], s2[4, 12] = float('inf'), float('-inf'), 0.5, float('inf'), float('-inf')
    model = ('table', s1.to(DEV), s2.to(DEV))
    inf_lists = [[3, 4], [3, 4, 6], [6, 3]]
    for agg in AGGS:
        got = _run(model, *_csr(inf_lists), 40, agg)
        check_regimen_topk(model, *_csr(inf_lists), 40, agg, got, what='inf')
        assert got[1][0, 0] == 10 and got[0][0, 0] == float('inf') and got[1][1, 0] == 10
        assert 12 not in got[1][0].tolist() and 12 in got[1][1].tolist()  # (3, 4) alone has no triple for 12; (3, 6) has
        assert got[1][0, 38] == 11 and got[1][0, 39] == -1                 # -inf: last candidate (0 under noisy-or is too)
        if agg == 'max':
            assert got[0][0, 38] == float('-inf')
        else:
            assert got[0][0, 38] == 0.0


# ------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_repeatable_and_capturable(kind):
    g = torch.Generator().manual_seed(77)
    n_rel, k = 300, 10
    model = _dm(n_rel, 16, g) if kind == 'distmult' else _tb(n_rel, g)
    lists = _random_lists(200, g, hi=12)
    drugs, ptr = _csr(lists)
    known = _known_for(lists[:40], n_rel, g)
    for agg in AGGS:
        a = _run(model, drugs, ptr, k, agg, known)
        b = _run(model, drugs, ptr, k, agg, known)
        assert _same(a, b), agg
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                     # the single entry alone: no parallel branches
            c = _run(model, drugs, ptr, k, agg, known)
        for x in c:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a, c), agg


# ------------------------------------------------------------------ TIP.regimen_side_effects
def _model_of(model):
    z = model.embeddings.detach()
    if model.decoder_kind == 'distmult':
        return ('distmult', z, model.decoder.weight.detach())
    dec = model.decoder
    with torch.no_grad():                                                 # the tables as NNDecoder.forward forms them
        s1 = ops.matmul(torch.relu(ops.matmul(z, dec.w1_l1)), dec.w1_l2.t())
        s2 = ops.matmul(torch.relu(ops.matmul(z, dec.w2_l1)), dec.w2_l2.t())
    return ('table', s1, s2)


def _pair_dict(idx, rng, d=None):
    d = {} if d is None else d
    idx = idx.cpu().tolist()
    for r, (a, b) in enumerate(torch.as_tensor(rng).long().tolist()):
        for u, v in zip(idx[0][a:b], idx[1][a:b]):
            d.setdefault((min(u, v), max(u, v)), set()).add(r)
    return d


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_regimen_side_effects(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting, normalize_regimens
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    train_d = _pair_dict(d.dd_train_idx, d.dd_train_range)
    both_d = _pair_dict(d.dd_test_idx, d.dd_test_range, _pair_dict(d.dd_train_idx, d.dd_train_range))
    lists = {None: None, 'train': tuple(t.to(DEV) for t in known_from_dict(train_d, n)),
             'all': tuple(t.to(DEV) for t in known_from_dict(both_d, n))}
    g = torch.Generator().manual_seed(4)
    regs = [p for p in sorted(train_d)[:6]] and [list(p) for p in sorted(train_d)[:6]]
    regs += _random_lists(40, g, hi=min(9, n), n=n) + [[], [3], [5, 2, 5, 2]]
    nd, nptr = (t.to(DEV) for t in normalize_regimens(regs, n, M_MAX))
    m = _model_of(model)
    k = min(R, 12)
    for agg in AGGS:
        for exclude in (None, 'train', 'all'):
            res = model.regimen_side_effects(regs, k=k, aggregate=agg, exclude=exclude, probability=False)
            assert res.relation.dtype == torch.int64 and res.u.dtype == torch.int64 and res.score.shape == (len(regs), k)
            have = res.relation >= 0
            assert bool((res.u < res.v)[have].all()) and bool(((res.u == -1) & (res.v == -1))[~have].all())
            # back to list positions of the normalised (sorted, de-duplicated) regimens
            pos = torch.full((len(regs), n), -1, dtype=torch.int64, device=DEV)
            owner = torch.repeat_interleave(torch.arange(len(regs), device=DEV), nptr[1:] - nptr[:-1])
            pos[owner, nd.long()] = torch.arange(nd.numel(), device=DEV) - nptr[owner]
            pi = torch.where(have, pos.gather(1, res.u.clamp(min=0)), res.u)
            pj = torch.where(have, pos.gather(1, res.v.clamp(min=0)), res.v)
            check_regimen_topk(m, nd, nptr, k, agg, (res.score, res.relation, pi, pj), lists[exclude],
                               what='TIP %s %s' % (decoder, exclude))
            prob = model.regimen_side_effects(regs, k=k, aggregate=agg, exclude=exclude)
            want = torch.sigmoid(res.score) if agg == 'max' \
                else torch.where(have, -torch.expm1(-res.score), torch.zeros_like(res.score))
            assert torch.equal(prob.score, want) and torch.equal(prob.relation, res.relation)
            assert torch.equal(prob.u, res.u) and torch.equal(prob.v, res.v)
            assert bool((prob.score[~have] == 0).all())
            same = model.regimen_side_effects((nd.cpu(), nptr.cpu()), k=k, aggregate=agg, exclude=exclude, probability=False)
            assert _same(tuple(res), tuple(same))
    assert bool((res.relation[-3:-1] == -1).all())                        # the empty and the singleton regimen
    # relations=[...]: candidates restricted, global ids returned, the filter follows
    sub = [4, 1, 5]
    sub_t = torch.tensor(sub, device=DEV)
    res = model.regimen_side_effects(regs, k=3, aggregate='noisy_or', exclude='train', relations=sub, probability=False)
    if decoder == 'distmult':
        m_sub = ('distmult', m[1], m[2][sub_t])
    else:
        dec, e = model.decoder, model.embeddings.detach()
        with torch.no_grad():
            m_sub = ('table', ops.matmul(torch.relu(ops.matmul(e, dec.w1_l1)), dec.w1_l2[sub_t].t()),
                     ops.matmul(torch.relu(ops.matmul(e, dec.w2_l1)), dec.w2_l2[sub_t].t()))
    assert bool(((res.relation < 0) | torch.isin(res.relation, sub_t)).all())
    local = torch.full((R,), -1, dtype=torch.int64, device=DEV)
    local[sub_t] = torch.arange(3, device=DEV)
    have = res.relation >= 0
    got_local = torch.where(have, local[res.relation.clamp(min=0)], res.relation)
    pi = torch.where(have, pos.gather(1, res.u.clamp(min=0)), res.u)
    pj = torch.where(have, pos.gather(1, res.v.clamp(min=0)), res.v)
    sub_known = known_from_dict({p: [sub.index(r) for r in rs if r in sub] for p, rs in train_d.items()}, n)
    check_regimen_topk(m_sub, nd, nptr, 3, 'noisy_or', (res.score, got_local, pi, pj), tuple(t.to(DEV) for t in sub_known),
                       what='TIP %s subset' % decoder)

    # `TIP.side_effects` after the renumbering moved into ops.restrict_known_relations: held to its own rule as before
    pairs = torch.randint(0, n, (2, 200), generator=g).to(DEV)
    both_sub = known_from_dict({p: [sub.index(r) for r in rs if r in sub] for p, rs in both_d.items()}, n)
    se = model.side_effects(pairs, k=3, exclude='all', relations=sub, sigmoid=False)
    se_local = torch.where(se.relation >= 0, local[se.relation.clamp(min=0)], se.relation)
    check_pair_topk(m_sub, pairs, 3, (se.score, se_local), tuple(t.to(DEV) for t in both_sub))
