"""CPU tests of the partner rank (include/tipk.h section 4g): the `_supported` predicates, the route query and its option,
argument validation of both C entries (every refusal happens before anything touches a device, so bogus device pointers are
safe here), the Python surface's refusals, `ops.targets_by_query` against a dict built by hand, self-tests of the fp64 spec
and the acceptance rule (tests/partner_rank_spec.py), and the degeneracy cap of that rule for the seeds and shapes
tests/test_gpu_partner_rank.py runs on the device."""
import ctypes
import math
import types

import pytest
import torch

import partner_rank_cases as cases
from partner_rank_spec import CAP, check_partner_rank, spec_partner_rank
from tip_amd import _lib, ops

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _dm(n=10, dim=16, n_rel=3, n_q=4, n_tgt=6, keys=None, kptr=None, z=FAKE, w=FAKE, qr=FAKE, qd=FAKE, tptr=FAKE, tnode=FAKE,
        out=FAKE, logit=FAKE):
    return _lib.lib().tipk_distmult_partner_rank(z, n, dim, w, n_rel, qr, qd, n_q, tptr, tnode, n_tgt, keys, kptr, out, logit,
                                                 None)


def _tb(n=10, n_rel=3, ld=None, n_q=4, n_tgt=6, keys=None, kptr=None, s1=FAKE, s2=FAKE, qr=FAKE, qd=FAKE, tptr=FAKE, tnode=FAKE,
        out=FAKE, logit=FAKE):
    return _lib.lib().tipk_pair_table_partner_rank(s1, s2, n if ld is None else ld, n, n_rel, qr, qd, n_q, tptr, tnode, n_tgt,
                                                   keys, kptr, out, logit, None)


def test_abi_and_supported_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() >= 29
    dm, tb = L.tipk_distmult_partner_rank_supported, L.tipk_pair_table_partner_rank_supported
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
    route = L.tipk_distmult_partner_rank_lds_route
    assert _lib.get_option('partner_rank_global') == 0
    assert route(645, 16) == 1                                           # BioSNAP: 645 rows of 80 B
    assert route(700, 16) == 1 and route(700, 32) == 1                   # 700 rows of 144 B: 101 KB
    assert route(2600, 16) == 0                                          # 2 600 rows of 80 B: 208 KB
    assert route(700, 256) == 0
    assert route(645, 6) == 0 and route(0, 16) == 0
    # the budget: n * stride * 4 + 16 * dim * 4 + 16 * 256 <= 152 KB; dim 16 has stride 20
    most = (152 * 1024 - 16 * 16 * 4 - 16 * 256) // 80
    assert route(most, 16) == 1 and route(most + 1, 16) == 0
    _lib.set_option('partner_rank_global', 1)
    try:
        assert _lib.get_option('partner_rank_global') == 1
        assert route(645, 16) == 0
        assert L.tipk_distmult_pair_rank_lds_route(16, 1097) == 1        # the option of 4g does not touch 4f
    finally:
        _lib.set_option('partner_rank_global', 0)
    assert route(645, 16) == 1


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(n_q=-1) == EINVAL
        assert call(n_tgt=-1) == EINVAL
        assert call(n=0) == EINVAL
        assert call(n_rel=0) == EINVAL
        assert call(keys=FAKE) == EINVAL                                  # keys without offsets, and the reverse
        assert call(kptr=FAKE) == EINVAL
        for name in ('qr', 'qd', 'tptr', 'tnode', 'out'):
            assert call(**{name: None}) == EINVAL, name
        assert call(n_tgt=-1, n=46341) == EINVAL                          # argument errors come before shape limits
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(s2=None) == EINVAL
    assert _dm(dim=0) == EINVAL and _dm(dim=-4) == EINVAL
    assert _tb(ld=9) == EINVAL                                           # row stride below n_nodes
    assert _dm(n_q=-1, dim=6) == EINVAL


def test_unsupported_shapes_and_empty_lists():
    assert _dm(dim=6) == EUNSUPPORTED
    assert _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED
    assert _dm(z=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # z must be 16-byte aligned
    assert _tb(n=46341, ld=46341) == EUNSUPPORTED
    assert _tb(n_rel=65537) == EUNSUPPORTED
    assert _dm(n_q=0) == 0 and _tb(n_q=0) == 0                           # nothing to rank: nothing launched
    assert _dm(n_tgt=0) == 0 and _tb(n_tgt=0) == 0
    assert _dm(n_tgt=0, z=None, qr=None, tnode=None, out=None) == 0
    assert _tb(n_q=0, s1=None, qd=None, tptr=None, out=None) == 0
    assert _dm(n_q=0, keys=FAKE, kptr=FAKE) == 0
    assert _dm(logit=None, n_tgt=0) == 0 and _tb(logit=None, n_q=0) == 0  # out_logit is optional


def test_ops_refuse_cpu_tensors():
    qr, qd, tptr, tnode = torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([0, 1, 2]), torch.tensor([0, 1])
    with pytest.raises(_lib.TipkError, match='device'):
        ops.distmult_partner_rank(torch.ones(5, 4), torch.ones(2, 4), qr, qd, tptr, tnode)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.pair_table_partner_rank(torch.ones(3, 5), torch.ones(3, 5), qr, qd, tptr, tnode)


def test_tip_rank_partners_refusals():
    from tip_amd.layers import TIP
    triples = (torch.tensor([[0], [1]]), torch.tensor([2]))
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.rank_partners(types.SimpleNamespace(decoder_kind='distmult', shard=object()), triples)
    for bad in ('test', 'none', 0):
        with pytest.raises(ValueError, match='filter'):
            TIP.rank_partners(types.SimpleNamespace(decoder_kind='nn', shard=None), triples, filter=bad)
    me = types.SimpleNamespace(decoder_kind='distmult', shard=None, embeddings=torch.zeros(5, 4),
                               data=types.SimpleNamespace(n_drug=5, n_dd_et=3))
    for idx in ([[0], [5]], [[-1], [1]]):
        with pytest.raises(ValueError, match='drug id out of range'):
            TIP.rank_partners(me, (torch.tensor(idx), torch.tensor([2])), filter=None)
    for et in (3, -1):
        with pytest.raises(ValueError, match='side-effect id out of range'):
            TIP.rank_partners(me, (torch.tensor([[0], [1]]), torch.tensor([et])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_partners(me, (torch.tensor([[0.0], [1.0]]), torch.tensor([2])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_partners(me, (torch.tensor([[0], [1]]), torch.tensor([2.0])), filter=None)
    with pytest.raises(ValueError, match='int tensors'):
        TIP.rank_partners(me, (torch.tensor([0, 1]), torch.tensor([2])), filter=None)


# ------------------------------------------------------------------ targets_by_query
def test_targets_by_query_vs_dict():
    n = 7
    # (r 4, u 0) is asked for partner 1 three times; (4, 1) is another query; (0, 6) ranks itself; partners keep the given order
    ei = torch.tensor([[0, 1, 0, 6, 0, 3, 1, 0],
                       [1, 0, 2, 6, 1, 2, 0, 1]])
    et = torch.tensor([4, 4, 2, 0, 4, 1, 3, 4])
    q_rel, q_drug, ptr, node, order = ops.targets_by_query(ei, et, n)
    want = {}
    for i, (u, v, r) in enumerate(zip(ei[0].tolist(), ei[1].tolist(), et.tolist())):
        want.setdefault((r, u), []).append((v, i))
    keys = sorted(want)
    assert list(zip(q_rel.tolist(), q_drug.tolist())) == keys == [(0, 6), (1, 3), (2, 0), (3, 1), (4, 0), (4, 1)]
    assert ptr.tolist() == [0, 1, 2, 3, 4, 7, 8]
    assert node.tolist() == [v for k in keys for v, _ in want[k]] == [6, 2, 2, 0, 1, 1, 1, 0]
    assert order.tolist() == [i for k in keys for _, i in want[k]]
    assert q_rel.dtype == torch.int32 and q_drug.dtype == torch.int32 and ptr.dtype == torch.int64 and node.dtype == torch.int32
    back = torch.empty(8, dtype=torch.int64)                              # the round trip: grouped results to the given order
    back[order] = node.long()
    assert back.tolist() == ei[1].tolist()
    u = torch.empty(8, dtype=torch.int64)
    u[order] = torch.repeat_interleave(q_drug.long(), ptr[1:] - ptr[:-1])
    assert u.tolist() == ei[0].tolist()
    e = ops.targets_by_query(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n)
    assert e[0].numel() == 0 and e[1].numel() == 0 and e[2].tolist() == [0] and e[3].numel() == 0 and e[4].numel() == 0
    with pytest.raises(_lib.TipkError):
        ops.targets_by_query(ei.float(), et, n)
    with pytest.raises(_lib.TipkError):
        ops.targets_by_query(ei, et[:-1], n)


def test_targets_by_query_random():
    g = torch.Generator().manual_seed(5)
    n, T = 11, 400
    ei, et = torch.randint(0, n, (2, T), generator=g), torch.randint(0, 9, (T,), generator=g)
    q_rel, q_drug, ptr, node, order = ops.targets_by_query(ei, et, n)
    key = q_rel.long() * n + q_drug.long()
    assert bool((key[1:] > key[:-1]).all()) and int(ptr[-1]) == T and sorted(order.tolist()) == list(range(T))
    owner = torch.repeat_interleave(torch.arange(q_rel.numel()), ptr[1:] - ptr[:-1])
    assert torch.equal(ei[0][order].int(), q_drug[owner]) and torch.equal(et[order].int(), q_rel[owner])
    assert torch.equal(ei[1][order].int(), node)
    same = owner[1:] == owner[:-1]
    assert bool((order[1:] > order[:-1])[same].all())                     # stable inside a query


# ------------------------------------------------------------------ the spec and the rule, by hand
def _three():
    # relation 0, drug 0: a = z0 * w0 = (2, 1); logits of drugs 0, 1, 2: 3, 3, 2.  drug 1: a = (4, -1): 3, 9, 4
    z = torch.tensor([[1.0, 1.0], [2.0, -1.0], [1.0, 0.0]])
    w = torch.tensor([[2.0, 1.0], [1.0, -1.0]])
    return ('distmult', z, w)


def test_spec_by_hand():
    m = _three()
    q_rel, q_drug = torch.tensor([0, 0, 0]), torch.tensor([0, 1, 2])
    ptr, node = cases.csr([[1, 2], [0, 2], [0, 1]])
    r, s = spec_partner_rank(m, q_rel, q_drug, ptr, node)
    # drug 0 ranks 1 (logit 3) over 2 (logit 2); drug 1 ranks 2 (4) over 0 (3); drug 2: a = (2, 0): logits 2, 4, 2
    assert r.tolist() == [1, 2, 2, 1, 2, 1] and s.tolist() == [3.0, 2.0, 3.0, 4.0, 2.0, 4.0]
    # the self candidate is never counted: for drug 0 its own logit 3 ties with drug 1's and would beat drug 2
    assert r[1] == 2
    # (0, 1) listed forward only: for query (0, 0) drug 1 is no competitor but still a target; for query (0, 1) -- the key
    # in reverse -- drug 0 is no competitor either
    known = cases.known_from_dict({0: [(0, 1)]}, 3, 2)
    r, _ = spec_partner_rank(m, q_rel, q_drug, ptr, node, known)
    assert r.tolist() == [1, 1, 2, 1, 2, 1]
    # the list of another relation filters nothing
    r, _ = spec_partner_rank(m, q_rel, q_drug, ptr, node, cases.known_from_dict({1: [(0, 1), (1, 0), (2, 1)]}, 3, 2))
    assert r.tolist() == [1, 2, 2, 1, 2, 1]
    # a tie resolves by ascending id: z3 = z1 gives drug 3 drug 1's logit
    m4 = ('distmult', torch.cat([m[1], m[1][1:2]]), m[2])
    r, s = spec_partner_rank(m4, [0], [0], [0, 2], [3, 1])
    assert r.tolist() == [2, 1] and s[0] == s[1]
    # not ranked: r, u, t out of range on either side, t == u, a NaN logit; a NaN competitor beats nothing
    r, s = spec_partner_rank(m, torch.tensor([2, -1, 0, 0, 0]), torch.tensor([0, 0, 3, -1, 1]), torch.tensor([0, 1, 2, 3, 4, 7]),
                             torch.tensor([1, 1, 1, 1, 3, -1, 1]))
    assert r.tolist() == [0] * 7 and bool(torch.isnan(s).all())
    s2t = torch.tensor([[float('nan'), 1.0, 2.0, 0.5]])                  # a table query whose drug 0 alone is NaN
    r, s = spec_partner_rank(('table', torch.zeros(1, 4), s2t), [0], [3], [0, 3], [0, 1, 2])
    assert r.tolist() == [0, 2, 1] and math.isnan(s[0]) and s[1:].tolist() == [1.0, 2.0]
    # the table logit is s1t[r, u] + s2t[r, c]: the queried drug reads the FIRST table
    s1t, s2t = torch.tensor([[10.0, 20.0, 30.0]]), torch.tensor([[1.0, 3.0, 2.0]])
    r, s = spec_partner_rank(('table', s1t, s2t), [0, 0], [0, 2], [0, 2, 4], [1, 2, 0, 1])
    assert s.tolist() == [13.0, 12.0, 31.0, 33.0] and r.tolist() == [1, 2, 2, 1]


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_check_partner_rank_catches_mistakes(kind):
    g = torch.Generator().manual_seed(2)
    n, n_rel = 12, 3
    m = cases.model_of(kind, n, n_rel, 8, g)
    q_rel, q_drug = torch.tensor([0, 0, 1, 2, 1]), torch.tensor([1, 3, 5, 7, 2])
    known = cases.known_from_dict({0: [(1, 0), (1, 4), (6, 1), (8, 3)], 1: [(5, c) for c in range(n - 2) if c != 5],
                                   2: [(c, 7) for c in range(n) if c != 7]}, n, n_rel)
    ptr, node = cases.csr([[0, 4, 7], [1, 1], [c for c in range(n) if c != 5], [2, 8], [3]])
    r, s = spec_partner_rank(m, q_rel, q_drug, ptr, node, known)
    assert r[16:18].tolist() == [1, 1] and r[3] == r[4]                   # (2, 7): all listed in reverse; the repeated target
    good = (r.int(), s.float())
    assert check_partner_rank(m, q_rel, q_drug, ptr, node, good, known) == 0.0
    check_partner_rank(m, q_rel, q_drug, ptr, node, (r.int(), None), known)

    def planted(fn, lists=(ptr, node), base=good):
        br, bs = base[0].clone(), base[1].clone()
        fn(br, bs)
        with pytest.raises(AssertionError):
            check_partner_rank(m, q_rel, q_drug, lists[0], lists[1], (br, bs), known)

    def up(br, bs):                                                      # a rank off by one, either way
        br[5] += 1

    def down(br, bs):
        br[6] -= 1 if br[6] > 1 else -1

    raw = spec_partner_rank(m, q_rel, q_drug, ptr, node)[0]
    assert bool((raw[:3] >= r[:3]).all()) and bool((raw != r).any())
    j = int(torch.nonzero(raw != r)[0])

    def dropped_filter(br, bs):                                          # a listed drug counted as a competitor
        br[j] = raw[j]

    def dropped_target(br, bs):                                          # target 4 of (0, 1) is listed: it still has a rank
        br[1] = 0
        bs[1] = float('nan')

    def unranked(br, bs):
        br[18] = 0

    def off_logit(br, bs):
        bs[0] = bs[0] * 1.001 + 0.001

    for fn in (up, down, dropped_filter, dropped_target, unranked, off_logit):
        planted(fn)
    # a counted self candidate: the ranks of a spec that lets u compete are caught wherever u beats the target
    selfish = r.clone()
    owner = torch.repeat_interleave(torch.arange(5), ptr[1:] - ptr[:-1])
    from partner_rank_spec import query_logits64
    L = query_logits64(m, q_rel, q_drug)[0]
    beats = L[owner, q_drug[owner]] > L[owner, node.long()]
    assert bool(beats.any())
    selfish[beats] += 1
    with pytest.raises(AssertionError, match='outside its interval'):
        check_partner_rank(m, q_rel, q_drug, ptr, node, (selfish, s), known)
    # a rank where none is due: a target outside [0, n), a target that is the queried drug
    ptr2, node2 = cases.csr([[0, n, 1], [], [], [], []])
    r2, s2 = spec_partner_rank(m, q_rel, q_drug, ptr2, node2, known)
    assert r2.tolist()[1:] == [0, 0] and r2[0] > 0
    check_partner_rank(m, q_rel, q_drug, ptr2, node2, (r2, s2), known)
    for at in (1, 2):
        bad = r2.clone()
        bad[at] = 1
        with pytest.raises(AssertionError, match='not ranked'):
            check_partner_rank(m, q_rel, q_drug, ptr2, node2, (bad, s2), known)
    # ties resolve by ascending id: two equal rows of z (equal table columns) ranked the wrong way round are caught, and
    # the cap refuses a case made of such ties
    if kind == 'distmult':
        z = m[1].clone()
        z[6] = z[2]
        mt = ('distmult', z, m[2])
    else:
        a, b = m[1].clone(), m[2].clone()
        a[:, 6], b[:, 6] = a[:, 2], b[:, 2]
        mt = ('table', a, b)
    ptr3, node3 = cases.csr([[2, 6], [], [], [], []])
    r3, s3 = spec_partner_rank(mt, q_rel, q_drug, ptr3, node3)
    assert r3[1] == r3[0] + 1 and s3[0] == s3[1]
    assert check_partner_rank(mt, q_rel, q_drug, ptr3, node3, (r3, s3), cap=None) == 1.0
    with pytest.raises(AssertionError, match='proves nothing'):
        check_partner_rank(mt, q_rel, q_drug, ptr3, node3, (r3, s3))


# ------------------------------------------------------------------ the cap, for the device cases' seeds
def _share(case):
    return check_partner_rank(case[0], case[1], case[2], case[3], case[4], None, case[5])


def test_cap_small_and_counts_cases():
    worst = 0.0
    for n in cases.SMALL_N:
        for kind, dims in (('distmult', cases.SMALL_DIM), ('table', (0,))):
            for dim in dims:
                case = cases.small_case(kind, n, dim)
                worst = max(worst, _share(case), _share(case[:5] + (None,)))
    for kind in ('distmult', 'table'):
        case = cases.counts_case(kind)
        worst = max(worst, _share(case), _share(case[:5] + (None,)))
    assert worst <= CAP, worst


def test_cap_corner_routes_and_screen_cases():
    for n in (70, 4500):
        for kind in ('distmult', 'table'):
            case = cases.corner_case(kind, n)[0]
            assert _share(case) <= CAP and _share(case[:5] + (None,)) <= CAP
    for n, dim, n_q in cases.ROUTES:
        assert _share(cases.routes_case(n, dim, n_q)) <= CAP
    for n in (130, 700):
        assert _share(cases.screen_case(n)) <= CAP
    assert _share(cases.screen_case(130, one_direction=True)) <= CAP


def test_cap_biosnap_case():
    """The held-out triples of relations 0..199 of the bundled graph under filter='all', with the device test's seeded
    weights: the cap on every 16th query (the device test holds all of them to the cap as well)."""
    from tip_amd.data import build_data_dict
    d = build_data_dict()
    n, R = d['n_drug'], d['n_dd_et']
    keep = d['dd_test_et'] < 200
    q_rel, q_drug, ptr, node, _ = ops.targets_by_query(d['dd_test_idx'][:, keep], d['dd_test_et'][keep], n)
    known = biosnap_known(d)
    pick = torch.arange(0, q_rel.numel(), 16)
    lists = [node[int(ptr[q]):int(ptr[q + 1])].tolist() for q in pick.tolist()]
    sub_ptr, sub_node = cases.csr(lists)
    share = check_partner_rank(cases.biosnap_weights(n, R), q_rel[pick], q_drug[pick], sub_ptr, sub_node, None, known)
    assert sub_node.numel() > 5000 and share <= CAP, share


def biosnap_known(d, dev='cpu'):
    """The relation-major keys of train + test, as `TIP.rank_partners(filter='all')` filters, built with torch ops."""
    n, R = d['n_drug'], d['n_dd_et']
    rel, key = [], []
    for idx, rng in ((d['dd_train_idx'], d['dd_train_range']), (d['dd_test_idx'], d['dd_test_range'])):
        ends = torch.as_tensor(rng).reshape(-1, 2)[:, 1].contiguous().long()
        rel.append(torch.bucketize(torch.arange(idx.shape[1]), ends, right=True))
        key.append(idx[0].long() * n + idx[1].long())
    comb = torch.unique(torch.cat(rel) * (n * n) + torch.cat(key))
    ptr = torch.zeros(R + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(torch.div(comb, n * n, rounding_mode='floor'), minlength=R), 0)
    return (comb % (n * n)).to(dev), ptr.to(dev)
