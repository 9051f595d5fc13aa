"""-m gpu: `tipk_distmult_pair_topk` / `tipk_pair_table_pair_topk` (include/tipk.h section 4d) and `TIP.side_effects`
against the fp64 acceptance rule of tests/pair_topk_spec.py -- small shapes around the 64-relation lane groups for both
decoders, ties, the known filter's corner pairs, both DistMult routes and repeat runs, an out-of-range pair through the C
entries, the exclude modes of `TIP.side_effects` for both decoder kinds, and every pair of a BioSNAP-sized graph."""
import os

import pytest
import torch

from pair_topk_spec import check_pair_topk, known_from_dict, logits64
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 97
K_MAX = 128


def _pairs(p, g):
    """[2, p]: a pair, its reverse, a self pair, the first pair again, the last node with itself, the first node with
    itself, then random pairs (p = 1: the first pair alone)."""
    head = [(3, 7), (7, 3), (5, 5), (3, 7), (N - 1, N - 1), (0, 0)]
    if p <= len(head):
        return torch.tensor(head[:p]).t().contiguous().to(DEV)
    rest = torch.randint(0, N, (p - len(head), 2), generator=g)
    return torch.cat([torch.tensor(head), rest]).t().contiguous().to(DEV)


def _known(n_rel, g):
    """(7, 3) listed in that direction only: every third relation; (5, 5): every relation; the first key (0, 0) and the last
    key (96, 96): one relation each; 300 random pairs with random relations."""
    d = {(7, 3): range(0, n_rel, 3), (5, 5): range(n_rel), (0, 0): [n_rel - 1], (N - 1, N - 1): [0]}
    for u, v in torch.randint(0, N, (300, 2), generator=g).tolist():
        if (min(u, v), max(u, v)) in ((3, 7), (5, 5), (0, 0), (N - 1, N - 1)):
            continue
        d[(u, v)] = torch.nonzero(torch.rand(n_rel, generator=g) < 0.3).reshape(-1).tolist()
    return tuple(t.to(DEV) for t in known_from_dict(d, N))


def _ks(n_rel):
    """k in {1, R, R + 3, 128}, as far as the entry supports them (k <= 128)."""
    return sorted({k for k in (1, n_rel, n_rel + 3, K_MAX) if k <= K_MAX})


def _small_cases(model, run, n_rel, seed, symmetric):
    g = torch.Generator().manual_seed(seed)
    known = _known(n_rel, g)
    for p in (1, 5, 20003):                                 # 20 003: more pairs than resident waves (loop and tail)
        pairs = _pairs(p, g)
        for k in _ks(n_rel):
            for kn in (None, known):
                got = run(pairs, k, kn)
                check_pair_topk(model, pairs, k, got, kn)
                if symmetric and p > 1:                    # the reversed pair: identical bits
                    assert torch.equal(got[0][0], got[0][1]) and torch.equal(got[1][0], got[1][1])
                if p > 3:                                   # the repeated pair
                    assert torch.equal(got[0][0], got[0][3]) and torch.equal(got[1][0], got[1][3])
                if kn is not None and p > 2:                # (5, 5): every relation known
                    assert bool((got[1][2] == -1).all()) and bool(torch.isneginf(got[0][2]).all())


@pytest.mark.parametrize('dim', [4, 16, 128])
@pytest.mark.parametrize('n_rel', [1, 63, 64, 65, 130])
def test_distmult_small_shapes(n_rel, dim):
    g = torch.Generator().manual_seed(100 * n_rel + dim)
    z = (torch.randn(N, dim, generator=g) / dim ** 0.25).to(DEV)
    w = (torch.randn(n_rel, dim, generator=g) / dim ** 0.25).to(DEV)
    _small_cases(('distmult', z, w), lambda pairs, k, kn: ops.distmult_pair_topk(z, w, pairs, k, kn), n_rel,
                 seed=n_rel + dim, symmetric=True)


@pytest.mark.parametrize('n_rel', [1, 63, 64, 65, 130])
def test_table_small_shapes(n_rel):
    g = torch.Generator().manual_seed(7 * n_rel)
    wide = torch.randn(2, N, n_rel + 5, generator=g).to(DEV)            # row stride n_rel + 5
    s1, s2 = wide[0, :, :n_rel], wide[1, :, :n_rel]
    _small_cases(('table', s1, s2), lambda pairs, k, kn: ops.pair_table_pair_topk(s1, s2, pairs, k, kn), n_rel,
                 seed=n_rel, symmetric=False)


def test_column_sliced_tables_equal_contiguous_copies():
    """Tables with column stride 2 (`big[:, ::2]`; the row stride 140 >= 70 looks fine) must be read as their contiguous
    copies are, bit for bit, by all four table faces: the entries know a row stride only.  70 relations: lane windows of
    64 + 6.  The partner rank takes relation-major tables, so its views are [70, 9]."""
    def bits(out):
        return [t.view(torch.int32) if t.is_floating_point() else t for t in out]

    def same(face, t1, t2, *lists):
        assert t1.stride(1) == 2 and t2.stride(1) == 2
        got, want = face(t1, t2, *lists), face(t1.contiguous(), t2.contiguous(), *lists)
        assert all(torch.equal(a, b) for a, b in zip(bits(got), bits(want))), face.__name__

    g = torch.Generator().manual_seed(970)
    n, n_rel, k = 9, 70, 3
    s1, s2 = (torch.randn(n, 2 * n_rel, generator=g).to(DEV)[:, ::2] for _ in range(2))
    s1t, s2t = (torch.randn(n_rel, 2 * n, generator=g).to(DEV)[:, ::2] for _ in range(2))
    assert tuple(s1.shape) == (n, n_rel) and tuple(s1t.shape) == (n_rel, n)
    pairs = torch.tensor([[0, 1, 8, 3, 4], [5, 0, 2, 7, 6]], device=DEV)
    one_each = torch.arange(6, device=DEV)                                # a target per pair / query
    tgt_rel = torch.tensor([0, 63, 64, 69, 17], device=DEV)
    same(ops.pair_table_pair_topk, s1, s2, pairs, k)
    same(ops.pair_table_pair_rank, s1, s2, pairs, one_each, tgt_rel)
    reg_drugs = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8, 1, 3, 2, 8], device=DEV)
    reg_ptr = torch.tensor([0, 3, 5, 9, 11, 13], device=DEV)
    same(ops.pair_table_regimen_topk, s1, s2, reg_drugs, reg_ptr, k)
    same(ops.pair_table_partner_rank, s1t, s2t, tgt_rel, pairs[0], one_each, pairs[1])


def test_ties_resolve_by_relation_id():
    """rel_w has 13 distinct rows repeated 10 times (table: 13 distinct columns): every logit occurs 10 times, and equal
    logits must come out in ascending relation id -- rule 3 of the acceptance rule is exact about that."""
    g = torch.Generator().manual_seed(13)
    n_rel, dim = 130, 16
    z = torch.randn(N, dim, generator=g).to(DEV)
    w = torch.randn(13, dim, generator=g).to(DEV)[torch.arange(n_rel) % 13].contiguous()
    pairs = _pairs(200, g)
    for k in (10, 128):
        s, r = ops.distmult_pair_topk(z, w, pairs, k)
        check_pair_topk(('distmult', z, w), pairs, k, (s, r))
        run = (r[:, 1:] % 13) == (r[:, :-1] % 13)                         # neighbours from one group of equal rows
        assert bool((s[:, 1:][run] == s[:, :-1][run]).all()) and bool((r[:, 1:][run] > r[:, :-1][run]).all())
        assert int(run.sum()) >= pairs.shape[1] * (k - (k + 9) // 10 - 1) * 0.9
    s1 = torch.randn(N, 13, generator=g).to(DEV)[:, torch.arange(n_rel) % 13].contiguous()
    s2 = torch.randn(N, 13, generator=g).to(DEV)[:, torch.arange(n_rel) % 13].contiguous()
    s, r = ops.pair_table_pair_topk(s1, s2, pairs, 128)
    check_pair_topk(('table', s1, s2), pairs, 128, (s, r))
    run = (r[:, 1:] % 13) == (r[:, :-1] % 13)
    assert bool((s[:, 1:][run] == s[:, :-1][run]).all()) and bool((r[:, 1:][run] > r[:, :-1][run]).all())


@pytest.mark.parametrize('n_rel', [70, 4500])
def test_known_filter_corner_pairs(n_rel):
    """n_rel = 4 500 spans three bitmap windows of 2 048 relations: the cursor into a pair's block moves across them."""
    g = torch.Generator().manual_seed(n_rel)
    dim = 8
    z = torch.randn(N, dim, generator=g).to(DEV)
    w = torch.randn(n_rel, dim, generator=g).to(DEV)
    s1, s2 = torch.randn(N, n_rel, generator=g).to(DEV), torch.randn(N, n_rel, generator=g).to(DEV)
    some = sorted(set(torch.randint(0, n_rel, (n_rel // 2,), generator=g).tolist()) | {0, 2047, 2048, n_rel - 1} & set(range(n_rel)))
    d = {(0, 0): some,                      # the first key of the list
         (9, 4): some,                      # listed as (9, 4), asked as (4, 9)
         (20, 30): range(n_rel),            # every relation known
         (40, 41): [],                      # an empty entry: no key at all
         (N - 1, N - 1): some}              # the last key of the list
    known = tuple(t.to(DEV) for t in known_from_dict(d, N))
    assert known[0].tolist() == [0, 4 * N + 9, 20 * N + 30, (N - 1) * N + N - 1]
    pairs = torch.tensor([[0, 4, 9, 20, 30, 40, 50, N - 1, 0, 1],
                          [0, 9, 4, 30, 20, 41, 60, N - 1, 1, 0]], device=DEV)
    k = 64
    for model, run in ((('distmult', z, w), lambda: ops.distmult_pair_topk(z, w, pairs, k, known)),
                       (('table', s1, s2), lambda: ops.pair_table_pair_topk(s1, s2, pairs, k, known))):
        s, r = run()
        check_pair_topk(model, pairs, k, (s, r), known)
        listed = torch.tensor(some, device=DEV)
        for row in (0, 1, 2, 7):
            assert not bool(torch.isin(r[row].long(), listed).any()), row
        assert bool((r[3] == -1).all()) and bool((r[4] == -1).all())
        L, _ = logits64(model, pairs[0], pairs[1])
        for row in (5, 6, 8, 9):                                          # absent from the lists: the plain top k
            assert bool(torch.isin(L[row].argmax(), r[row].long()).all()), row
    # an empty list (no key at all) filters nothing
    none = tuple(t.to(DEV) for t in known_from_dict({}, N))
    a = ops.distmult_pair_topk(z, w, pairs, k, none)
    b = ops.distmult_pair_topk(z, w, pairs, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_routes_identical_and_repeatable():
    g = torch.Generator().manual_seed(700)
    n_rel, k = 700, 10
    pairs = _pairs(3000, g)
    known = _known(n_rel, g)
    L = _lib.lib()
    assert _lib.get_option('pair_topk_stream') == 0
    # rel_w cannot fit LDS: the streamed route on its own
    z = (torch.randn(N, 256, generator=g) / 4).to(DEV)
    w = (torch.randn(n_rel, 256, generator=g) / 4).to(DEV)
    assert L.tipk_distmult_pair_topk_lds_route(256, n_rel) == 0
    a = ops.distmult_pair_topk(z, w, pairs[:, :400], k, known)
    b = ops.distmult_pair_topk(z, w, pairs[:, :400], k, known)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'streamed route, run to run'
    check_pair_topk(('distmult', z, w), pairs[:, :400], k, a, known)
    # a shape that fits: both routes
    z = (torch.randn(N, 16, generator=g) / 2).to(DEV)
    w = (torch.randn(n_rel, 16, generator=g) / 2).to(DEV)
    assert L.tipk_distmult_pair_topk_lds_route(16, n_rel) == 1
    a = ops.distmult_pair_topk(z, w, pairs, k, known)
    b = ops.distmult_pair_topk(z, w, pairs, k, known)
    _lib.set_option('pair_topk_stream', 1)
    try:
        assert L.tipk_distmult_pair_topk_lds_route(16, n_rel) == 0
        c = ops.distmult_pair_topk(z, w, pairs, k, known)
        d = ops.distmult_pair_topk(z, w, pairs, k, known)
    finally:
        _lib.set_option('pair_topk_stream', 0)
    for x, y, what in ((a, b, 'LDS route, run to run'), (c, d, 'streamed route, run to run'), (a, c, 'LDS vs streamed')):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), what
    check_pair_topk(('distmult', z, w), pairs, k, a, known)
    # the generic-width kernel on both routes too (dim 16 has a kernel of its own)
    z = (torch.randn(N, 32, generator=g) / 2).to(DEV)
    w = (torch.randn(n_rel, 32, generator=g) / 2).to(DEV)
    a = ops.distmult_pair_topk(z, w, pairs, k, known)
    _lib.set_option('pair_topk_stream', 1)
    try:
        c = ops.distmult_pair_topk(z, w, pairs, k, known)
    finally:
        _lib.set_option('pair_topk_stream', 0)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), 'LDS vs streamed, dim 32'
    check_pair_topk(('distmult', z, w), pairs, k, a, known)
    s1, s2 = torch.randn(N, n_rel, generator=g).to(DEV), torch.randn(N, n_rel, generator=g).to(DEV)
    a = ops.pair_table_pair_topk(s1, s2, pairs, k, known)
    b = ops.pair_table_pair_topk(s1, s2, pairs, k, known)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'table variant, run to run'


def test_out_of_range_pair_is_padded():
    """Through the C entries (the Python faces of `TIP` refuse such a pair): the row is fully padded, its neighbours'
    rows are what they are without it."""
    g = torch.Generator().manual_seed(5)
    n_rel, dim, k = 70, 16, 7
    z = torch.randn(N, dim, generator=g).to(DEV)
    w = torch.randn(n_rel, dim, generator=g).to(DEV)
    s1, s2 = torch.randn(N, n_rel, generator=g).to(DEV), torch.randn(N, n_rel, generator=g).to(DEV)
    pu = torch.tensor([1, N, 2, -1, 3, 2 ** 31 - 1, 4], dtype=torch.int32, device=DEV)
    pv = torch.tensor([2, 0, 500, 0, 3, 5, -7], dtype=torch.int32, device=DEV)
    good = torch.tensor([0, 4], device=DEV)
    bad = torch.tensor([1, 2, 3, 5, 6], device=DEV)
    valid = torch.stack([pu[good], pv[good]])
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(torch.device(DEV))
    for kind in ('distmult', 'table'):
        out_s = torch.full((7, k), 123.0, device=DEV)
        out_r = torch.full((7, k), 123, dtype=torch.int32, device=DEV)
        if kind == 'distmult':
            status = L.tipk_distmult_pair_topk(p(z), N, dim, p(w), n_rel, p(pu), p(pv), 7, None, None, None, 0, k, p(out_s),
                                               p(out_r), None, st)
            want = ops.distmult_pair_topk(z, w, valid, k)
        else:
            status = L.tipk_pair_table_pair_topk(p(s1), p(s2), n_rel, N, n_rel, p(pu), p(pv), 7, None, None, None, 0, k,
                                                 p(out_s), p(out_r), st)
            want = ops.pair_table_pair_topk(s1, s2, valid, k)
        assert status == 0
        torch.cuda.synchronize()
        assert bool((out_r[bad] == -1).all()) and bool(torch.isneginf(out_s[bad]).all()), kind
        assert torch.equal(out_s[good], want[0]) and torch.equal(out_r[good], want[1]), kind


# ------------------------------------------------------------------ TIP.side_effects
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
def test_tip_side_effects_exclude_modes(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    train_d = _pair_dict(d.dd_train_idx, d.dd_train_range)
    test_d = _pair_dict(d.dd_test_idx, d.dd_test_range)
    both_d = _pair_dict(d.dd_test_idx, d.dd_test_range, _pair_dict(d.dd_train_idx, d.dd_train_range))
    train = tuple(t.to(DEV) for t in known_from_dict(train_d, n))
    both = tuple(t.to(DEV) for t in known_from_dict(both_d, n))
    # pairs with a held-out relation that is not a training relation of the pair, in both directions; plus plain ones
    held = [(p, r) for p, rs in sorted(test_d.items()) for r in sorted(rs) if r not in train_d.get(p, ())][:40]
    assert len(held) >= 10
    g = torch.Generator().manual_seed(4)
    rand = torch.randint(0, n, (2, 200), generator=g)
    pairs = torch.cat([torch.tensor([[p[0] for p, _ in held], [p[1] for p, _ in held]]),
                       torch.tensor([[p[1] for p, _ in held], [p[0] for p, _ in held]]), rand], 1).to(DEV)
    m = _model_of(model)
    k = R

    res = model.side_effects(pairs, k=k, exclude=None, sigmoid=False)
    assert res.relation.dtype == torch.int64 and res.score.shape == (pairs.shape[1], k)
    check_pair_topk(m, pairs, k, res, None)
    L, T = logits64(m, pairs[0], pairs[1])                               # the dense fp64 ranking of all relations
    top = torch.sort(L, dim=1, descending=True, stable=True)
    gap = (top.values[:, :-1] - top.values[:, 1:]) > 2 * T.amax(1, keepdim=True)
    clear = torch.cat([gap, gap[:, -1:]], 1) & torch.cat([gap[:, :1], gap], 1)   # both neighbours further than rounding
    assert bool(((res.relation == top.indices) | ~clear).all())
    assert bool(clear.any())
    sig = model.side_effects(pairs, k=k, exclude=None)
    assert torch.equal(sig.score, torch.sigmoid(res.score)) and torch.equal(sig.relation, res.relation)
    # the returned logits are the decoder's logits of the same triples
    ok = res.relation >= 0
    idx = pairs[:, :, None].expand(2, pairs.shape[1], k)[:, ok]
    if decoder == 'distmult':
        ref = model.decoder(model.embeddings, idx, res.relation[ok], sigmoid=False)
    else:
        ref = ops.pair_table_score(m[1], m[2], idx, res.relation[ok], sigmoid=False)
    both_tau = 2 * T.gather(1, res.relation.clamp(min=0))[ok]            # each kernel is within tau of fp64
    assert bool(((res.score[ok].double() - ref.double()).abs() <= both_tau).all())

    res_t = model.side_effects(pairs, k=k, exclude='train', sigmoid=False)
    check_pair_topk(m, pairs, k, res_t, train)
    res_a = model.side_effects(pairs, k=k, exclude='all', sigmoid=False)
    check_pair_topk(m, pairs, k, res_a, both)
    for i, (p, r) in enumerate(held):
        for row in (i, len(held) + i):
            rt, ra = res_t.relation[row].tolist(), res_a.relation[row].tolist()
            assert r in rt and r not in ra, (p, r)
            assert not (set(rt) & train_d.get(p, set())) and not (set(ra) & both_d[p])
    pad = model.side_effects(pairs[:, :3], k=k + 2, exclude='all')
    assert bool((pad.relation[:, k:] == -1).all()) and bool((pad.score[:, k:] == 0).all())

    # relations=[...]: candidates restricted, ids mapped back, the filter follows
    sub = [4, 1, 5]
    res_s = model.side_effects(pairs, k=3, exclude='train', relations=sub, sigmoid=False)
    sub_t = torch.tensor(sub, device=DEV)
    if decoder == 'distmult':
        m_sub = ('distmult', m[1], m[2][sub_t])
    else:                                                                 # the tables of the gathered rows, as formed
        dec, e = model.decoder, model.embeddings.detach()
        with torch.no_grad():
            m_sub = ('table', ops.matmul(torch.relu(ops.matmul(e, dec.w1_l1)), dec.w1_l2[sub_t].t()),
                     ops.matmul(torch.relu(ops.matmul(e, dec.w2_l1)), dec.w2_l2[sub_t].t()))
    local = torch.full((R,), -1, dtype=torch.int64, device=DEV)
    local[sub_t] = torch.arange(3, device=DEV)
    sub_known = known_from_dict({p: [sub.index(r) for r in rs if r in sub] for p, rs in train_d.items()}, n)
    got_local = torch.where(res_s.relation >= 0, local[res_s.relation.clamp(min=0)], res_s.relation)
    assert bool(((res_s.relation < 0) | torch.isin(res_s.relation, sub_t)).all())
    check_pair_topk(m_sub, pairs, 3, (res_s.score, got_local), tuple(t.to(DEV) for t in sub_known))

    with pytest.raises(ValueError, match='out of range'):
        model.side_effects(torch.tensor([[0, n], [1, 2]]), k=3)
    with pytest.raises(ValueError, match='out of range'):
        model.side_effects(torch.tensor([[0, 1], [-1, 2]]), k=3)


def test_biosnap_size_all_pairs():
    """Every unordered pair of 645 drugs (207 690), 1 097 relations, dim 16, k = 10, a BioSNAP-like training list excluded
    (about 70 known relations per known pair), random z / w: the whole result against fp64, chunked on the device."""
    g = torch.Generator().manual_seed(645)
    n, R, dim, k = 645, 1097, 16, 10
    z = (torch.randn(n, dim, generator=g) / 2).to(DEV)
    w = (torch.randn(R, dim, generator=g) / 2).to(DEV)
    iu = torch.triu_indices(n, n, 1).to(DEV)
    assert iu.shape[1] == 207690
    # a training list: 63 000 known pairs with ~70 relations each, grouped by relation, each block mirrored
    kp = iu[:, torch.randperm(iu.shape[1], generator=g)[:63000].to(DEV)]
    rel = torch.randint(0, R, (63000 * 70,), generator=g).to(DEV)
    owner = torch.arange(63000, device=DEV).repeat_interleave(70)
    order = torch.sort(rel, stable=True).indices
    half = kp[:, owner[order]]
    counts = torch.bincount(rel, minlength=R)
    ends = torch.cumsum(counts, 0)
    # edges of relation r: [half_r | mirrored half_r], as the data contract has them
    pos = torch.arange(half.shape[1], device=DEV) - (ends - counts)[rel[order]]
    start = 2 * (ends - counts)[rel[order]]
    edge = torch.empty((2, 2 * half.shape[1]), dtype=torch.int64, device=DEV)
    edge[:, start + pos] = half
    edge[:, start + counts[rel[order]] + pos] = half.flip(0)
    rng = torch.stack([2 * (ends - counts), 2 * ends], 1)
    known = ops.known_relations_by_pair(edge, rng, n)
    assert known[0].numel() == 63000 and 60 < known[2].numel() / 63000 < 70
    assert _lib.lib().tipk_distmult_pair_topk_lds_route(dim, R) == 1
    got = ops.distmult_pair_topk(z, w, iu, k, known)
    check_pair_topk(('distmult', z, w), iu, k, got, known, chunk=16384)
    assert bool((got[1] >= 0).all())
