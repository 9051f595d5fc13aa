"""CPU tests of the pair top-k (include/tipk.h section 4d): the `_supported` predicates, the route query and its option,
argument validation of both C entries (every refusal happens before anything touches a device, so bogus device pointers are
safe here), the Python surface's refusals, `ops.known_relations_by_pair` on CPU tensors against a Python dict, and
self-tests of the fp64 spec and the acceptance rule (tests/pair_topk_spec.py) on hand-worked cases."""
import ctypes
import types

import pytest
import torch

from pair_topk_spec import check_pair_topk, known_from_dict, spec_pair_topk
from tip_amd import _lib, ops

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _dm(n=10, dim=16, n_rel=3, n_pairs=4, k=5, keys=None, kptr=None, krel=None, n_known=0, z=FAKE, w=FAKE, pu=FAKE,
        out=FAKE):
    return _lib.lib().tipk_distmult_pair_topk(z, n, dim, w, n_rel, pu, FAKE, n_pairs, keys, kptr, krel, n_known, k, out,
                                              FAKE, None, None)


def _tb(n=10, n_rel=3, ld=None, n_pairs=4, k=5, keys=None, kptr=None, krel=None, n_known=0, s1=FAKE, pv=FAKE):
    return _lib.lib().tipk_pair_table_pair_topk(s1, FAKE, n_rel if ld is None else ld, n, n_rel, FAKE, pv, n_pairs, keys,
                                                kptr, krel, n_known, k, FAKE, FAKE, None)


def test_supported_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() >= 26
    dm, tb = L.tipk_distmult_pair_topk_supported, L.tipk_pair_table_pair_topk_supported
    for dim in (4, 8, 16, 32, 64, 128, 256):
        assert dm(645, dim, 1097, 10) == 1
    for dim in (0, 2, 6, 130, 260):
        assert dm(645, dim, 1097, 10) == 0
    assert dm(645, 16, 1097, 1) == 1 and dm(645, 16, 1097, 128) == 1
    assert dm(645, 16, 1097, 0) == 0 and dm(645, 16, 1097, 129) == 0
    assert dm(1, 16, 1, 4) == 1 and dm(46340, 256, 65536, 128) == 1
    assert dm(0, 16, 4, 4) == 0 and dm(46341, 16, 4, 4) == 0
    assert dm(645, 16, 0, 4) == 0 and dm(645, 16, 65537, 4) == 0
    assert dm(10000, 128, 2000, 10) == 1                                 # config 5
    assert tb(1, 1, 1) == 1 and tb(46340, 65536, 128) == 1
    assert tb(0, 4, 4) == 0 and tb(46341, 4, 4) == 0 and tb(645, 0, 4) == 0 and tb(645, 65537, 4) == 0
    assert tb(645, 1097, 0) == 0 and tb(645, 1097, 129) == 0
    ws = L.tipk_distmult_pair_topk_workspace_bytes
    assert ws(645, 16, 1097, 207690, 10) >= 0
    assert ws(46341, 16, 4, 1, 4) == -1 and ws(645, 6, 4, 1, 4) == -1 and ws(645, 16, 4, 1, 129) == -1
    assert ws(645, 16, 4, -1, 4) == -1


def test_route_query_and_option():
    L = _lib.lib()
    assert _lib.get_option('pair_topk_stream') == 0
    assert L.tipk_distmult_pair_topk_lds_route(16, 1097) == 1            # BioSNAP: 1 097 rows of 80 B beside the lists
    assert L.tipk_distmult_pair_topk_lds_route(16, 700) == 1
    assert L.tipk_distmult_pair_topk_lds_route(256, 700) == 0            # 700 rows of 1 040 B
    assert L.tipk_distmult_pair_topk_lds_route(128, 2000) == 0           # config 5
    assert L.tipk_distmult_pair_topk_lds_route(6, 10) == 0
    _lib.set_option('pair_topk_stream', 1)
    try:
        assert _lib.get_option('pair_topk_stream') == 1
        assert L.tipk_distmult_pair_topk_lds_route(16, 1097) == 0
    finally:
        _lib.set_option('pair_topk_stream', 0)
    assert L.tipk_distmult_pair_topk_lds_route(16, 1097) == 1


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(k=0) == EINVAL
        assert call(k=-3) == EINVAL
        assert call(n_pairs=-1) == EINVAL
        assert call(n=0) == EINVAL
        assert call(n_rel=0) == EINVAL
        assert call(n_known=-1) == EINVAL
        assert call(keys=FAKE, n_known=2) == EINVAL                       # known arrays given only in part
        assert call(keys=FAKE, kptr=FAKE, n_known=2) == EINVAL
        assert call(kptr=FAKE, krel=FAKE, n_known=2) == EINVAL
        assert call(krel=FAKE) == EINVAL
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL and _dm(pu=None) == EINVAL and _dm(out=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(pv=None) == EINVAL
    assert _dm(dim=0) == EINVAL
    assert _tb(ld=2) == EINVAL                                           # row stride below n_rel
    assert _dm(k=0, dim=6) == EINVAL                                     # argument errors come before shape limits
    assert _tb(k=0, n=46341) == EINVAL


def test_unsupported_shapes_and_empty_list():
    assert _dm(k=129) == EUNSUPPORTED
    assert _dm(dim=6) == EUNSUPPORTED
    assert _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED
    assert _dm(w=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # rel_w must be 16-byte aligned
    assert _tb(k=129) == EUNSUPPORTED
    assert _tb(n=46341) == EUNSUPPORTED
    assert _tb(n_rel=65537) == EUNSUPPORTED
    assert _dm(n_pairs=0) == 0 and _tb(n_pairs=0) == 0                   # no pair: nothing to do, nothing launched
    assert _dm(n_pairs=0, z=None, pu=None, out=None) == 0
    assert _dm(n_pairs=0, keys=FAKE, kptr=FAKE, krel=FAKE, n_known=3) == 0


def test_ops_refuse_cpu_tensors():
    pairs = torch.tensor([[0, 1], [2, 3]])
    with pytest.raises(_lib.TipkError):
        ops.distmult_pair_topk(torch.ones(5, 4), torch.ones(2, 4), pairs, 2)
    with pytest.raises(_lib.TipkError):
        ops.pair_table_pair_topk(torch.ones(5, 3), torch.ones(5, 3), pairs, 2)


def test_tip_side_effects_refusals():
    from tip_amd.layers import TIP
    pairs = torch.tensor([[0], [1]])
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.side_effects(types.SimpleNamespace(decoder_kind='distmult', shard=object()), pairs, k=5)
    for bad in ('test', 'none', 0):
        with pytest.raises(ValueError, match='exclude'):
            TIP.side_effects(types.SimpleNamespace(decoder_kind='nn', shard=None), pairs, k=5, exclude=bad)
    assert 'side_effects' in TIP.pred_topk.__doc__


# ------------------------------------------------------------------ known_relations_by_pair
def _dict_of(ei, rl, n, d=None):
    d = {} if d is None else d
    for r, (a, b) in enumerate(rl):
        for e in range(a, b):
            u, v = int(ei[0][e]), int(ei[1][e])
            d.setdefault((min(u, v), max(u, v)), set()).add(r)
    return d


def _as_lists(known):
    keys, ptr, rel = (t.tolist() for t in known)
    return keys, ptr, rel


def test_known_relations_by_pair_vs_dict():
    n = 7
    # relation 0: (0,1) with its mirror and a duplicate, a self pair; relation 1: empty; relation 2: (0,1) again, (5,2);
    # relation 3: (6,6), (2,5) -- the mirror of relation 2's edge under another relation
    ei = torch.tensor([[0, 1, 0, 3, 0, 5, 6, 2],
                       [1, 0, 1, 3, 1, 2, 6, 5]])
    rl = [[0, 4], [4, 4], [4, 6], [6, 8]]
    rt = torch.tensor(rl)
    got = ops.known_relations_by_pair(ei, rt, n)
    want = known_from_dict(_dict_of(ei.tolist(), rl, n), n)
    assert _as_lists(got) == _as_lists(want)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
    keys, ptr, rel = _as_lists(got)
    assert keys == [0 * n + 1, 2 * n + 5, 3 * n + 3, 6 * n + 6] and ptr == [0, 2, 4, 5, 6] and rel == [0, 2, 2, 3, 0, 3]
    assert ops.known_relations_by_pair(ei, rt, n) is got                    # cached per (edge tensor, range tensor)
    assert _as_lists(ops.known_relations_by_pair(ei, torch.tensor(rl), n)) == _as_lists(got)

    # a second list merged in: a new pair, a new relation of an old pair, a repeat of an old entry
    ei2 = torch.tensor([[4, 1, 5], [2, 0, 2]])
    rl2 = [[0, 1], [1, 2], [2, 3], [3, 3]]
    both = ops.known_relations_by_pair(ei, torch.tensor(rl), n, extra=(ei2, torch.tensor(rl2)))
    want = known_from_dict(_dict_of(ei2.tolist(), rl2, n, _dict_of(ei.tolist(), rl, n)), n)
    assert _as_lists(both) == _as_lists(want)
    assert _as_lists(both)[0] == [0 * n + 1, 2 * n + 4, 2 * n + 5, 3 * n + 3, 6 * n + 6]

    empty = ops.known_relations_by_pair(torch.zeros((2, 0), dtype=torch.int64), torch.tensor([[0, 0], [0, 0]]), n)
    assert _as_lists(empty) == ([], [0], [])


def test_known_relations_by_pair_random():
    g = torch.Generator().manual_seed(3)
    n, n_rel = 23, 9
    sizes = torch.randint(0, 40, (n_rel,), generator=g)
    sizes[4] = 0
    ends = torch.cumsum(sizes, 0)
    rl = torch.stack([ends - sizes, ends], 1)
    half = torch.randint(0, n, (2, int(ends[-1])), generator=g)
    got = ops.known_relations_by_pair(half, rl, n)
    want = known_from_dict(_dict_of(half.tolist(), rl.tolist(), n), n)
    assert _as_lists(got) == _as_lists(want)
    assert bool((got[0][1:] > got[0][:-1]).all())


# ------------------------------------------------------------------ the spec and the rule, by hand
def _dm_model():
    z = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.5, 0.5], [2.0, 2.0]])
    w = torch.tensor([[1.0, 1.0], [-1.0, 2.0], [0.0, -3.0], [1.0, 1.0], [2.0, 0.0]])
    return ('distmult', z, w)


def test_spec_by_hand():
    m = _dm_model()
    # pair (0, 1): h = (3, -2); logits 1, -7, 6, 1, 6: ties 2 < 4 and 0 < 3; a negative weight row ranks last
    s, r = spec_pair_topk(m, [[0], [1]], 5)
    assert r.tolist() == [[2, 4, 0, 3, 1]] and s.tolist() == [[6.0, 6.0, 1.0, 1.0, -7.0]]
    s2, r2 = spec_pair_topk(m, [[1], [0]], 5)                             # DistMult is symmetric
    assert r2.tolist() == r.tolist() and s2.tolist() == s.tolist()
    s, r = spec_pair_topk(m, [[0], [1]], 2)
    assert r.tolist() == [[2, 4]]
    # k > R: padding; a self pair is scored like any other: h = (1, 4): 5, 7, -12, 5, 2
    s, r = spec_pair_topk(m, [[0], [0]], 7)
    assert r.tolist() == [[1, 0, 3, 4, 2, -1, -1]] and s[0, :5].tolist() == [7.0, 5.0, 5.0, 2.0, -12.0]
    assert bool(torch.isneginf(s[0, 5:]).all())
    # known, listed for (1, 0): dropped for (0, 1) too; another pair is untouched
    known = known_from_dict({(1, 0): [2, 0]}, 4)
    s, r = spec_pair_topk(m, [[0, 1, 0], [1, 0, 2]], 3, known)
    assert r[0].tolist() == [4, 3, 1] and r[1].tolist() == [4, 3, 1]
    assert r[2].tolist() == spec_pair_topk(m, [[0], [2]], 3)[1][0].tolist()
    # all relations known: a fully padded row
    every = known_from_dict({(0, 1): range(5)}, 4)
    s, r = spec_pair_topk(m, [[1], [0]], 3, every)
    assert r.tolist() == [[-1, -1, -1]] and bool(torch.isneginf(s).all())


def test_spec_table_is_not_symmetric():
    s1 = torch.tensor([[1.0, 0.0, 2.0], [0.0, 5.0, 0.0]])
    s2 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    m = ('table', s1, s2)
    s, r = spec_pair_topk(m, [[0, 1], [1, 0]], 3)
    assert r.tolist() == [[2, 0, 1], [1, 0, 2]] and s.tolist() == [[3.0, 2.0, 1.0], [5.0, 0.0, 0.0]]
    known = known_from_dict({(1, 0): [0]}, 2)
    s, r = spec_pair_topk(m, [[0, 1], [1, 0]], 3, known)                  # dropped in both directions
    assert r.tolist() == [[2, 1, -1], [1, 2, -1]]


@pytest.mark.parametrize('kind', ['distmult', 'table'])
def test_check_pair_topk_catches_mistakes(kind):
    g = torch.Generator().manual_seed(1)
    n, n_rel, k = 12, 9, 4
    if kind == 'distmult':
        m = ('distmult', torch.randn(n, 8, generator=g), torch.randn(n_rel, 8, generator=g))
    else:
        m = ('table', torch.randn(n, n_rel, generator=g), torch.randn(n, n_rel, generator=g))
    pairs = torch.tensor([[0, 3, 5, 7, 2], [1, 3, 2, 0, 5]])
    known = known_from_dict({(1, 0): [0, 4], (5, 2): range(n_rel - 2), (7, 0): range(n_rel)}, n)
    s, r = spec_pair_topk(m, pairs, k, known)
    good = (s.float(), r.int())
    check_pair_topk(m, pairs, k, good, known)
    assert r[3].tolist() == [-1] * k and r[2, 2:].tolist() == [-1, -1] and sorted(r[4].tolist()) == sorted(r[2].tolist())

    def planted(fn):
        bs, br = good[0].clone(), good[1].clone()
        fn(bs, br)
        with pytest.raises(AssertionError):
            check_pair_topk(m, pairs, k, (bs, br), known)

    def swap(bs, br):                                                    # order
        bs[0, [0, 1]] = bs[0, [1, 0]]
        br[0, [0, 1]] = br[0, [1, 0]]

    def known_returned(bs, br):
        br[0, 3] = 4

    def duplicate(bs, br):
        br[1, 3] = br[1, 2]
        bs[1, 3] = bs[1, 2]

    def off_logit(bs, br):
        bs[1, 0] = bs[1, 0] * 1.001 + 0.001

    def out_of_range(bs, br):
        br[1, 3] = n_rel

    def short_row(bs, br):                                               # padding where a candidate exists
        bs[1, 3] = float('-inf')
        br[1, 3] = -1

    def overfull_row(bs, br):                                            # an entry where padding belongs
        bs[3, 0] = 0.0
        br[3, 0] = 1

    def pad_score(bs, br):
        bs[2, 3] = 0.0

    for fn in (swap, known_returned, duplicate, off_logit, out_of_range, short_row, overfull_row, pad_score):
        planted(fn)
    s5, r5 = spec_pair_topk(m, pairs, k + 1, known)                       # the 5th best in place of the 4th

    def fifth(bs, br):
        bs[1, 3] = s5[1, 4]
        br[1, 3] = r5[1, 4]
    planted(fifth)
    # ties resolve by ascending id: two equal rows of w (or equal table columns) in the wrong order are caught
    if kind == 'distmult':
        w = m[2].clone()
        w[6] = w[2]
        mt = ('distmult', m[1], w)
    else:
        a, b = m[1].clone(), m[2].clone()
        a[:, 6], b[:, 6] = a[:, 2], b[:, 2]
        mt = ('table', a, b)
    s, r = spec_pair_topk(mt, pairs[:, 1:2], n_rel)
    i2 = r[0].tolist().index(2)
    assert r[0, i2 + 1] == 6 and s[0, i2] == s[0, i2 + 1]
    check_pair_topk(mt, pairs[:, 1:2], n_rel, (s.float(), r.int()))
    r[0, i2], r[0, i2 + 1] = 6, 2
    with pytest.raises(AssertionError):
        check_pair_topk(mt, pairs[:, 1:2], n_rel, (s.float(), r.int()))
