"""CPU tests of the pair rank (include/tipk.h section 4f): the `_supported` predicates, the route query and its option,
argument validation of both C entries (every refusal happens before anything touches a device, so bogus device pointers are
safe here), the Python surface's refusals, `ops.targets_by_pair` against a dict built by hand, `utils.rank_report` against
numbers worked by hand, self-tests of the fp64 spec and the acceptance rule (tests/pair_rank_spec.py), and the degeneracy
cap of that rule for the seeds and shapes tests/test_gpu_pair_rank.py runs on the device."""
import ctypes
import math
import types

import pytest
import torch

import pair_rank_cases as cases
from pair_rank_spec import CAP, check_pair_rank, spec_pair_rank
from pair_topk_spec import known_from_dict
from tip_amd import _lib, ops, utils

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _dm(n=10, dim=16, n_rel=3, n_pairs=4, n_tgt=6, keys=None, kptr=None, krel=None, n_known=0, z=FAKE, w=FAKE, pu=FAKE,
        tptr=FAKE, trel=FAKE, out=FAKE, logit=FAKE):
    return _lib.lib().tipk_distmult_pair_rank(z, n, dim, w, n_rel, pu, FAKE, n_pairs, tptr, trel, n_tgt, keys, kptr, krel,
                                              n_known, out, logit, None)


def _tb(n=10, n_rel=3, ld=None, n_pairs=4, n_tgt=6, keys=None, kptr=None, krel=None, n_known=0, s1=FAKE, pv=FAKE, tptr=FAKE,
        trel=FAKE, out=FAKE):
    return _lib.lib().tipk_pair_table_pair_rank(s1, FAKE, n_rel if ld is None else ld, n, n_rel, FAKE, pv, n_pairs, tptr, trel,
                                                n_tgt, keys, kptr, krel, n_known, out, FAKE, None)


def test_abi_and_supported_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() >= 28
    dm, tb = L.tipk_distmult_pair_rank_supported, L.tipk_pair_table_pair_rank_supported
    for dim in (4, 8, 16, 32, 64, 128, 256):
        assert dm(645, dim, 1097) == 1
    for dim in (0, 2, 6, 130, 260):
        assert dm(645, dim, 1097) == 0
    assert dm(1, 4, 1) == 1 and dm(46340, 256, 65536) == 1
    assert dm(0, 16, 4) == 0 and dm(46341, 16, 4) == 0 and dm(645, 16, 0) == 0 and dm(645, 16, 65537) == 0
    assert tb(1, 1) == 1 and tb(46340, 65536) == 1
    assert tb(0, 4) == 0 and tb(46341, 4) == 0 and tb(645, 0) == 0 and tb(645, 65537) == 0


def test_route_query_and_option():
    L = _lib.lib()
    assert _lib.get_option('pair_rank_stream') == 0
    assert L.tipk_distmult_pair_rank_lds_route(16, 1097) == 1            # BioSNAP: 1 097 rows of 80 B
    assert L.tipk_distmult_pair_rank_lds_route(16, 700) == 1
    assert L.tipk_distmult_pair_rank_lds_route(16, 4500) == 0            # 4 500 rows of 80 B: 360 KB
    assert L.tipk_distmult_pair_rank_lds_route(256, 700) == 0
    assert L.tipk_distmult_pair_rank_lds_route(6, 10) == 0
    _lib.set_option('pair_rank_stream', 1)
    try:
        assert _lib.get_option('pair_rank_stream') == 1
        assert L.tipk_distmult_pair_rank_lds_route(16, 1097) == 0
        assert L.tipk_distmult_pair_topk_lds_route(16, 1097) == 1        # the option of 4f does not touch 4d
    finally:
        _lib.set_option('pair_rank_stream', 0)
    assert L.tipk_distmult_pair_rank_lds_route(16, 1097) == 1


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(n_pairs=-1) == EINVAL
        assert call(n_tgt=-1) == EINVAL
        assert call(n=0) == EINVAL
        assert call(n_rel=0) == EINVAL
        assert call(n_known=-1) == EINVAL
        assert call(keys=FAKE, n_known=2) == EINVAL                       # known arrays given only in part
        assert call(keys=FAKE, kptr=FAKE, n_known=2) == EINVAL
        assert call(kptr=FAKE, krel=FAKE, n_known=2) == EINVAL
        assert call(krel=FAKE) == EINVAL
        assert call(tptr=None) == EINVAL and call(trel=None) == EINVAL and call(out=None) == EINVAL
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL and _dm(pu=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(pv=None) == EINVAL
    assert _dm(dim=0) == EINVAL and _dm(dim=-4) == EINVAL
    assert _tb(ld=2) == EINVAL                                           # row stride below n_rel
    assert _dm(n_tgt=-1, dim=6) == EINVAL                                # argument errors come before shape limits
    assert _tb(n_pairs=-1, n=46341) == EINVAL


def test_unsupported_shapes_and_empty_lists():
    assert _dm(dim=6) == EUNSUPPORTED
    assert _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED
    assert _dm(w=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # rel_w must be 16-byte aligned
    assert _tb(n=46341) == EUNSUPPORTED
    assert _tb(n_rel=65537) == EUNSUPPORTED
    assert _dm(n_pairs=0) == 0 and _tb(n_pairs=0) == 0                   # nothing to rank: nothing launched
    assert _dm(n_tgt=0) == 0 and _tb(n_tgt=0) == 0
    assert _dm(n_tgt=0, z=None, pu=None, trel=None, out=None) == 0
    assert _dm(n_pairs=0, keys=FAKE, kptr=FAKE, krel=FAKE, n_known=3) == 0
    assert _dm(logit=None, n_tgt=0) == 0                                 # out_logit is optional


def test_ops_refuse_cpu_tensors():
    pairs, tptr, trel = torch.tensor([[0, 1], [2, 3]]), torch.tensor([0, 1, 2]), torch.tensor([0, 1])
    with pytest.raises(_lib.TipkError):
        ops.distmult_pair_rank(torch.ones(5, 4), torch.ones(2, 4), pairs, tptr, trel)
    with pytest.raises(_lib.TipkError):
        ops.pair_table_pair_rank(torch.ones(5, 3), torch.ones(5, 3), pairs, tptr, trel)


def test_tip_rank_side_effects_refusals():
    from tip_amd.layers import TIP
    triples = (torch.tensor([[0], [1]]), torch.tensor([2]))
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.rank_side_effects(types.SimpleNamespace(decoder_kind='distmult', shard=object()), triples)
    for bad in ('test', 'none', 0):
        with pytest.raises(ValueError, match='filter'):
            TIP.rank_side_effects(types.SimpleNamespace(decoder_kind='nn', shard=None), triples, filter=bad)
    me = types.SimpleNamespace(decoder_kind='distmult', shard=None, embeddings=torch.zeros(5, 4),
                               data=types.SimpleNamespace(n_drug=5, n_dd_et=3))
    for idx in ([[0], [5]], [[-1], [1]]):
        with pytest.raises(ValueError, match='drug id out of range'):
            TIP.rank_side_effects(me, (torch.tensor(idx), torch.tensor([2])), filter=None)
    for et in (3, -1):
        with pytest.raises(ValueError, match='side-effect id out of range'):
            TIP.rank_side_effects(me, (torch.tensor([[0], [1]]), torch.tensor([et])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_side_effects(me, (torch.tensor([[0.0], [1.0]]), torch.tensor([2])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_side_effects(me, (torch.tensor([[0], [1]]), torch.tensor([2.0])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_side_effects(me, (torch.tensor([0, 1]), torch.tensor([2])), filter=None)


# ------------------------------------------------------------------ targets_by_pair
def test_targets_by_pair_vs_dict():
    n = 7
    # (0, 1) and (1, 0) are two groups; (0, 1, 4) is given twice; (6, 6) is a self pair; the relations keep the given order
    ei = torch.tensor([[0, 1, 0, 6, 0, 3, 1, 0],
                       [1, 0, 1, 6, 1, 2, 0, 1]])
    et = torch.tensor([4, 4, 2, 0, 4, 1, 3, 0])
    pairs, ptr, rel, order = ops.targets_by_pair(ei, et, n)
    want = {}
    for i, (u, v, r) in enumerate(zip(ei[0].tolist(), ei[1].tolist(), et.tolist())):
        want.setdefault((u, v), []).append((r, i))
    keys = sorted(want)
    assert pairs.t().tolist() == [list(k) for k in keys] == [[0, 1], [1, 0], [3, 2], [6, 6]]
    assert ptr.tolist() == [0, 4, 6, 7, 8]
    assert rel.tolist() == [r for k in keys for r, _ in want[k]] == [4, 2, 4, 0, 4, 3, 1, 0]
    assert order.tolist() == [i for k in keys for _, i in want[k]]
    assert pairs.dtype == torch.int64 and ptr.dtype == torch.int64 and rel.dtype == torch.int32
    back = torch.empty(8, dtype=torch.int64)                              # the round trip: grouped results to the given order
    back[order] = rel.long()
    assert back.tolist() == et.tolist()
    u = torch.empty(8, dtype=torch.int64)
    u[order] = torch.repeat_interleave(pairs[0], ptr[1:] - ptr[:-1])
    assert u.tolist() == ei[0].tolist()
    e = ops.targets_by_pair(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n)
    assert e[0].shape == (2, 0) and e[1].tolist() == [0] and e[2].numel() == 0 and e[3].numel() == 0
    with pytest.raises(_lib.TipkError):
        ops.targets_by_pair(ei.float(), et, n)


def test_targets_by_pair_random():
    g = torch.Generator().manual_seed(5)
    n, T = 11, 400
    ei, et = torch.randint(0, n, (2, T), generator=g), torch.randint(0, 9, (T,), generator=g)
    pairs, ptr, rel, order = ops.targets_by_pair(ei, et, n)
    key = pairs[0] * n + pairs[1]
    assert bool((key[1:] > key[:-1]).all()) and int(ptr[-1]) == T and sorted(order.tolist()) == list(range(T))
    owner = torch.repeat_interleave(torch.arange(pairs.shape[1]), ptr[1:] - ptr[:-1])
    assert torch.equal(ei[:, order], pairs[:, owner]) and torch.equal(et[order].int(), rel)
    same = owner[1:] == owner[:-1]
    assert bool((order[1:] > order[:-1])[same].all())                     # stable inside a pair


# ------------------------------------------------------------------ the spec and the rule, by hand
def _three():
    # pair (0, 1): h = (2, -1): logits 3, 3, -1: a tie between relations 0 and 1
    z = torch.tensor([[1.0, 1.0], [2.0, -1.0], [1.0, 0.0]])
    w = torch.tensor([[2.0, 1.0], [1.0, -1.0], [0.0, 1.0]])
    return ('distmult', z, w)


def test_spec_by_hand():
    m = _three()
    pairs = torch.tensor([[0, 1], [1, 0]])
    ptr, rel = torch.tensor([0, 3, 6]), torch.tensor([0, 1, 2, 2, 1, 0])
    r, s = spec_pair_rank(m, pairs, ptr, rel)
    assert r.tolist() == [1, 2, 3, 3, 2, 1] and s.tolist() == [3.0, 3.0, -1.0, -1.0, 3.0, 3.0]   # the tie: 0 before 1
    # relation 0 listed for (1, 0): gone as a competitor in both directions, still ranked as a target
    known = known_from_dict({(1, 0): [0]}, 3)
    r, _ = spec_pair_rank(m, pairs, ptr, rel, known)
    assert r.tolist() == [1, 1, 2, 2, 1, 1]
    # every relation listed: every target ranks 1; a pair without a block is untouched
    every = known_from_dict({(0, 1): range(3)}, 3)
    r, _ = spec_pair_rank(m, torch.tensor([[0, 0], [1, 2]]), ptr, rel, every)
    assert r[:3].tolist() == [1, 1, 1] and r[3:].tolist() == spec_pair_rank(m, [[0], [2]], [0, 3], rel[3:])[0].tolist()
    # not ranked: a pair index outside [0, n), a target outside [0, R), a NaN logit; a NaN competitor beats nothing
    r, s = spec_pair_rank(m, torch.tensor([[0, 3, -1], [1, 0, 0]]), torch.tensor([0, 2, 3, 4]), torch.tensor([3, -1, 0, 0]))
    assert r.tolist() == [0, 0, 0, 0] and bool(torch.isnan(s).all())
    s1 = torch.tensor([[float('nan'), 1.0, 2.0]])                        # a table pair whose relation 0 alone is NaN
    r, s = spec_pair_rank(('table', s1, torch.zeros(1, 3)), [[0], [0]], [0, 3], [0, 1, 2])
    assert r.tolist() == [0, 2, 1] and math.isnan(s[0]) and s[1:].tolist() == [1.0, 2.0]


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_check_pair_rank_catches_mistakes(kind):
    g = torch.Generator().manual_seed(2)
    n, n_rel = 12, 9
    m = cases.model_of(kind, n, n_rel, 8, g)
    pairs = torch.tensor([[0, 3, 5, 7, 2], [1, 3, 2, 0, 5]])
    known = known_from_dict({(1, 0): [0, 4], (5, 2): range(n_rel - 2), (7, 0): range(n_rel)}, n)
    ptr, rel = cases.csr([[0, 4, 7], [1, 1], list(range(n_rel)), [2, 8], [3]])
    r, s = spec_pair_rank(m, pairs, ptr, rel, known)
    assert r[14:16].tolist() == [1, 1] and r[3] == r[4]                   # (7, 0): all listed; the repeated target
    good = (r.int(), s.float())
    assert check_pair_rank(m, pairs, ptr, rel, good, known) == 0.0
    check_pair_rank(m, pairs, ptr, rel, (r.int(), None), known)

    def planted(fn):
        br, bs = good[0].clone(), good[1].clone()
        fn(br, bs)
        with pytest.raises(AssertionError):
            check_pair_rank(m, pairs, ptr, rel, (br, bs), known)

    def up(br, bs):                                                      # a rank off by one, either way
        br[5] += 1

    def down(br, bs):
        br[6] -= 1 if br[6] > 1 else -1

    raw = spec_pair_rank(m, pairs, ptr, rel)[0]
    assert raw[0] > r[0] or raw[1] > r[1] or raw[2] > r[2]               # the filter of (1, 0) changes a rank of pair 0
    j = int(torch.nonzero(raw != r)[0])

    def filtered_counted(br, bs):                                        # a listed relation counted as a competitor
        br[j] = raw[j]

    def dropped_target(br, bs):                                          # target 4 of (0, 1) is listed: it still has a rank
        br[1] = 0
        bs[1] = float('nan')

    def unranked(br, bs):
        br[16] = 0

    def off_logit(br, bs):
        bs[0] = bs[0] * 1.001 + 0.001

    for fn in (up, down, filtered_counted, dropped_target, unranked, off_logit):
        planted(fn)
    # a rank where none is due: a target outside [0, R)
    ptr2, rel2 = cases.csr([[0, n_rel], [], [], [], []])
    r2, s2 = spec_pair_rank(m, pairs, ptr2, rel2, known)
    assert r2.tolist()[1] == 0
    check_pair_rank(m, pairs, ptr2, rel2, (r2, s2), known)
    with pytest.raises(AssertionError):
        check_pair_rank(m, pairs, ptr2, rel2, (torch.tensor([int(r2[0]), 1]), s2), known)
    # ties resolve by ascending id: two equal rows of w (equal table columns) ranked the wrong way round are caught, and
    # the cap refuses a case made of such ties
    if kind == 'distmult':
        w = m[2].clone()
        w[6] = w[2]
        mt = ('distmult', m[1], w)
    else:
        a, b = m[1].clone(), m[2].clone()
        a[:, 6], b[:, 6] = a[:, 2], b[:, 2]
        mt = ('table', a, b)
    ptr3, rel3 = cases.csr([[2, 6], [], [], [], []])
    r3, s3 = spec_pair_rank(mt, pairs, ptr3, rel3)
    assert r3[1] == r3[0] + 1 and s3[0] == s3[1]
    assert check_pair_rank(mt, pairs, ptr3, rel3, (r3, s3), cap=None) == 1.0
    with pytest.raises(AssertionError, match='proves nothing'):
        check_pair_rank(mt, pairs, ptr3, rel3, (r3, s3))


# ------------------------------------------------------------------ utils.rank_report
def test_rank_report_by_hand():
    # relation 0: ranks 1, 2, 4; relation 2: rank 10 and one unranked triple; relations 1 and 3: no triple
    rank = torch.tensor([1, 10, 2, 0, 4])
    rel = torch.tensor([0, 2, 0, 2, 0])
    rep = utils.rank_report(rank, rel, 4, ks=(1, 3, 10))
    assert rep['unranked'] == 1
    assert abs(rep['mrr'] - (1 + 0.1 + 0.5 + 0.25) / 4) < 1e-15                        # micro: over the 4 ranked triples
    assert rep['hits'] == {1: 0.25, 3: 0.5, 10: 1.0}
    per = rep['per_relation']
    assert per['count'].tolist() == [3, 0, 1, 0] and per['count'].dtype == torch.int64
    assert per['mrr'].dtype == torch.float64 and per['hits'].shape == (3, 4)
    assert abs(float(per['mrr'][0]) - (1 + 0.5 + 0.25) / 3) < 1e-15 and abs(float(per['mrr'][2]) - 0.1) < 1e-15
    assert math.isnan(per['mrr'][1]) and math.isnan(per['mrr'][3]) and bool(torch.isnan(per['hits'][:, [1, 3]]).all())
    assert [round(float(x), 12) for x in per['hits'][:, 0]] == [round(1 / 3, 12), round(2 / 3, 12), 1.0]
    assert per['hits'][:, 2].tolist() == [0.0, 0.0, 1.0]
    assert abs(rep['macro_mrr'] - ((1 + 0.5 + 0.25) / 3 + 0.1) / 2) < 1e-15             # macro differs from micro
    assert abs(rep['macro_mrr'] - rep['mrr']) > 0.05
    none = utils.rank_report(torch.tensor([0, 0]), torch.tensor([1, 1]), 2, ks=(5,))
    assert none['unranked'] == 2 and math.isnan(none['mrr']) and math.isnan(none['hits'][5]) and math.isnan(none['macro_mrr'])
    assert none['per_relation']['count'].tolist() == [0, 0]
    empty = utils.rank_report(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), 3)
    assert empty['unranked'] == 0 and math.isnan(empty['mrr']) and sorted(empty['hits']) == [1, 3, 10]


# ------------------------------------------------------------------ the cap, for the device cases' seeds
def _share(case):
    return check_pair_rank(case[0], case[1], case[2], case[3], None, case[4])


def test_cap_small_and_counts_cases():
    worst = 0.0
    for n_rel in cases.SMALL_R:
        for kind, dims in (('distmult', cases.SMALL_DIM), ('table', (0,))):
            for dim in dims:
                worst = max(worst, _share(cases.small_case(kind, n_rel, dim)))
    for kind in ('distmult', 'table'):
        worst = max(worst, _share(cases.counts_case(kind)))
    assert worst <= CAP, worst


def test_cap_corner_and_routes_cases():
    for n_rel in (70, 4500):
        for kind in ('distmult', 'table'):
            assert _share(cases.corner_case(kind, n_rel)[0]) <= CAP
    for n_rel, dim, n_pairs in cases.ROUTES:
        assert _share(cases.routes_case(n_rel, dim, n_pairs)) <= CAP


def test_cap_biosnap_case():
    """The held-out triples of the bundled graph under filter='all', with the device test's seeded weights: the cap on every
    16th ordered pair (about 58 000 of the 924 708 triples; the device test holds all of them to the cap as well)."""
    from tip_amd.data import build_data_dict
    d = build_data_dict()
    n, R = d['n_drug'], d['n_dd_et']
    pairs, ptr, rel, _ = ops.targets_by_pair(d['dd_test_idx'], d['dd_test_et'], n)
    known = ops.known_relations_by_pair(d['dd_train_idx'], d['dd_train_range'], n, extra=(d['dd_test_idx'], d['dd_test_range']))
    pick = torch.arange(0, pairs.shape[1], 16)
    lists = [rel[int(ptr[p]):int(ptr[p + 1])].tolist() for p in pick.tolist()]
    sub_ptr, sub_rel = cases.csr(lists)
    share = check_pair_rank(cases.biosnap_weights(n, R), pairs[:, pick], sub_ptr, sub_rel, None, known)
    assert sub_rel.numel() > 40000 and share <= CAP, share
