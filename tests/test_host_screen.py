"""CPU tests of the DistMult screen (include/tipk.h section 4c): argument validation of the C entry (every refusal happens
before anything touches a device, so bogus device pointers are safe here), the `_supported` predicate and the route
option, the Python surface's refusals, and self-tests of the fp64 spec (tests/screen_spec.py) on hand-worked graphs."""
import ctypes
import types

import pytest
import torch

from screen_spec import assert_screen_exact, check_screen, exact_screen, keys_from_pairs, spec_screen
from tip_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _call(n=10, dim=16, n_rel=3, queries=((0, -1),), k=5, keys=None, kptr=None, z=FAKE, ws=FAKE):
    q = (ctypes.c_int32 * (2 * len(queries)))(*[x for p in queries for x in p]) if queries else None
    return _lib.lib().tipk_distmult_screen(z, n, dim, FAKE, n_rel, q, len(queries), keys, kptr, k, FAKE, FAKE, FAKE, ws,
                                           None)


def test_supported_predicate():
    L = _lib.lib()
    for dim in (4, 8, 16, 32, 64, 128, 256):
        assert L.tipk_distmult_screen_supported(645, dim, 10) == 1
    for dim in (0, 2, 6, 130, 260):
        assert L.tipk_distmult_screen_supported(645, dim, 10) == 0
    assert L.tipk_distmult_screen_supported(645, 16, 1) == 1 and L.tipk_distmult_screen_supported(645, 16, 1024) == 1
    assert L.tipk_distmult_screen_supported(645, 16, 0) == 0 and L.tipk_distmult_screen_supported(645, 16, 1025) == 0
    assert L.tipk_distmult_screen_supported(1, 16, 4) == 1 and L.tipk_distmult_screen_supported(46340, 128, 4) == 1
    assert L.tipk_distmult_screen_supported(0, 16, 4) == 0 and L.tipk_distmult_screen_supported(46341, 16, 4) == 0
    assert L.tipk_distmult_screen_workspace_bytes(46341, 16, 1, 4) == -1
    assert L.tipk_distmult_screen_workspace_bytes(645, 16, -1, 4) == -1
    small, big = L.tipk_distmult_screen_workspace_bytes(645, 16, 1097, 10), L.tipk_distmult_screen_workspace_bytes(645, 16, 1097, 100)
    assert 0 < small < big


def test_bitmap_route_and_option():
    L = _lib.lib()
    assert _lib.get_option('screen_search') == 0
    assert L.tipk_distmult_screen_bitmap_route(645) == 1
    assert L.tipk_distmult_screen_bitmap_route(724) == 1                # 724^2 bits = 65 524 bytes
    assert L.tipk_distmult_screen_bitmap_route(725) == 0
    assert L.tipk_distmult_screen_bitmap_route(10000) == 0
    _lib.set_option('screen_search', 1)
    try:
        assert L.tipk_distmult_screen_bitmap_route(645) == 0
    finally:
        _lib.set_option('screen_search', 0)
    assert L.tipk_distmult_screen_bitmap_route(645) == 1


@pytest.mark.parametrize('queries', [((3, -1),), ((-1, -1),), ((0, 10),), ((0, -2),), ((0, -1), (1, 3), (2, 11))])
def test_bad_queries_einval(queries):
    assert _call(queries=queries) == EINVAL


def test_bad_arguments_einval():
    assert _call(k=0) == EINVAL
    assert _call(k=-3) == EINVAL
    assert _call(keys=FAKE, kptr=None) == EINVAL                         # keys without their relation offsets
    assert _call(keys=None, kptr=FAKE) == EINVAL
    assert _call(z=None) == EINVAL
    assert _call(ws=None) == EINVAL
    assert _call(n_rel=0) == EINVAL
    assert _call(k=0, dim=6) == EINVAL                                   # argument errors come before shape limits


def test_unsupported_shapes():
    assert _call(k=1025) == EUNSUPPORTED
    assert _call(dim=6) == EUNSUPPORTED
    assert _call(dim=260) == EUNSUPPORTED
    assert _call(n=46341) == EUNSUPPORTED
    assert _call(z=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED      # z must be 16-byte aligned
    assert _call(queries=()) == 0                                         # no query: nothing to do, nothing launched


def test_ops_refuse_cpu_tensors():
    from tip_amd import ops
    with pytest.raises(_lib.TipkError):
        ops.distmult_screen(torch.ones(5, 4), torch.ones(2, 4), torch.tensor([[0, -1]]), 3)


class _ClaimsDevice(torch.Tensor):
    """A host tensor that says it is on the device (and so do the tensors derived from it): it takes a call past the
    operand checks, so that the refusal of another argument can be seen without a device."""
    is_cuda = property(lambda self: True)


def test_ops_refuse_cpu_known_lists():
    """The relation-major known lists of the screen and of the partner rank are refused on the host like every other
    operand -- here they are the ONLY host tensors the call can see, and the refusal comes before any launch."""
    from tip_amd import ops

    def on(*shape, **kw):
        return torch.ones(*shape, **kw).as_subclass(_ClaimsDevice)

    z, w = on(5, 4), on(2, 4)
    keys, kptr = torch.tensor([7]), torch.tensor([0, 0, 1])
    for known in ((keys, kptr), (keys.as_subclass(_ClaimsDevice), kptr), (keys, kptr.as_subclass(_ClaimsDevice))):
        with pytest.raises(_lib.TipkError, match='device'):
            ops.distmult_screen(z, w, torch.tensor([[0, -1]]), 3, known=known)
        ints = [on(n, dtype=torch.int64) for n in (2, 2, 3, 2)]             # q_rel, q_drug, tgt_ptr, tgt_node
        with pytest.raises(_lib.TipkError, match='device'):
            ops.distmult_partner_rank(z, w, *ints, known=known)


def test_tip_screen_refusals():
    from tip_amd.layers import TIP
    with pytest.raises(NotImplementedError, match='NN decoder'):
        TIP.screen(types.SimpleNamespace(decoder_kind='nn', shard=None), k=5)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.screen(types.SimpleNamespace(decoder_kind='distmult', shard=object()), k=5)
    with pytest.raises(ValueError):
        TIP.screen(types.SimpleNamespace(decoder_kind='distmult', shard=None), k=5, exclude='test')


def test_screen_queries_order():
    from tip_amd.layers import screen_queries
    assert screen_queries(3).tolist() == [[0, -1], [1, -1], [2, -1]]
    assert screen_queries(9, relations=[4, 2], drugs=[7, 0, 5]).tolist() == \
        [[4, 7], [2, 7], [4, 0], [2, 0], [4, 5], [2, 5]]                   # drug-major


# ------------------------------------------------------------------ the fp64 spec on hand-worked graphs
def _line_graph():
    """n = 3, dim = 1, z = (1, 2, 3), w = 1: logits (0,1) = 2, (0,2) = 3, (1,2) = 6."""
    return torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[1.0]])


def test_spec_relation_query():
    z, w = _line_graph()
    s, u, v = spec_screen(z, w, [[0, -1]], 2)
    assert s.tolist() == [[6.0, 3.0]] and u.tolist() == [[1, 0]] and v.tolist() == [[2, 2]]
    s, u, v = spec_screen(z, w, [[0, -1]], 5)                            # 3 candidates: 2 padded slots
    assert s[0, :3].tolist() == [6.0, 3.0, 2.0] and u.tolist() == [[1, 0, 0, -1, -1]] and v.tolist() == [[2, 2, 1, -1, -1]]
    assert s[0, 3:].isneginf().all()


def test_spec_known_pairs_either_direction():
    z, w = _line_graph()
    known = keys_from_pairs([[(2, 1)]], 3)                               # listed as (2, 1): drops the candidate (1, 2)
    s, u, v = spec_screen(z, w, [[0, -1]], 2, known)
    assert s.tolist() == [[3.0, 2.0]] and u.tolist() == [[0, 0]] and v.tolist() == [[2, 1]]
    s, u, v = spec_screen(z, w, [[0, 1]], 3, known)                      # drug 1: partner 2 known, 0 left
    assert s[0, 0].item() == 2.0 and u.tolist() == [[1, -1, -1]] and v.tolist() == [[0, -1, -1]]


def test_spec_drug_query_and_ties():
    z, w = _line_graph()
    s, u, v = spec_screen(z, w, [[0, 1]], 2)
    assert s.tolist() == [[6.0, 2.0]] and u.tolist() == [[1, 1]] and v.tolist() == [[2, 0]]
    ones = torch.ones(3, 2)
    s, u, v = spec_screen(ones, torch.ones(1, 2), [[0, -1], [0, 2]], 3)  # every logit 2: ascending key
    assert u.tolist() == [[0, 0, 1], [2, 2, -1]] and v.tolist() == [[1, 2, 2], [0, 1, -1]]


def test_spec_negative_weights_and_all_known():
    z = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, -1.0]])
    w = torch.tensor([[1.0, -1.0], [0.5, 0.5]])
    # relation 0: (0,1)=0 (0,2)=1 (0,3)=2 (1,2)=-1 (1,3)=1 (2,3)=3
    s, u, v = spec_screen(z, w, [[0, -1]], 3)
    assert s.tolist() == [[3.0, 2.0, 1.0]] and u.tolist() == [[2, 0, 0]] and v.tolist() == [[3, 3, 2]]
    every = keys_from_pairs([[], [(a, b) for a in range(4) for b in range(a + 1, 4)]], 4)
    s, u, v = spec_screen(z, w, [[1, -1], [1, 3]], 2, every)
    assert s.isneginf().all() and (u == -1).all() and (v == -1).all()


def test_exact_screen_equals_spec_on_hand_graphs():
    """The vectorised exact reference gives the Python-loop spec's answer on every hand-worked graph above, and
    `assert_screen_exact` names the first differing (query, slot)."""
    z, w = _line_graph()
    ones = torch.ones(3, 2)
    z4 = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, -1.0]])
    w4 = torch.tensor([[1.0, -1.0], [0.5, 0.5]])
    every = keys_from_pairs([[], [(a, b) for a in range(4) for b in range(a + 1, 4)]], 4)
    for zz, ww, q, k, known in [(z, w, [[0, -1]], 2, None), (z, w, [[0, -1]], 5, None),
                                (z, w, [[0, -1], [0, 1]], 3, keys_from_pairs([[(2, 1)]], 3)), (z, w, [[0, 1]], 2, None),
                                (ones, torch.ones(1, 2), [[0, -1], [0, 2]], 3, None), (z4, w4, [[0, -1], [1, -1]], 3, None),
                                (z4, w4, [[1, -1], [1, 3], [0, 3], [0, -1]], 2, every)]:
        s, u, v = spec_screen(zz, ww, q, k, known)
        got = exact_screen(zz, ww, q, k, known)
        assert_screen_exact(got, (s.float(), u.int(), v.int()))
    got = exact_screen(ones, torch.ones(1, 2), [[0, -1], [0, 2]], 3)
    bad = [t.clone() for t in got]
    bad[2][1, [0, 1]] = bad[2][1, [1, 0]]                                  # two tied partners in the wrong order
    with pytest.raises(AssertionError, match='query 1 slot 0'):
        assert_screen_exact(bad, got)
    zn = z.clone()
    zn[0] = float('nan')                                                   # NaN logits are never returned
    s, u, v = exact_screen(zn, w, [[0, -1], [0, 0]], 2)
    assert s.tolist() == [[6.0, float('-inf')], [float('-inf')] * 2] and u.tolist() == [[1, -1], [-1, -1]]


def test_check_screen_catches_mistakes():
    """The acceptance check passes the spec's own answer and refuses a wrong order, a known pair and a missing better
    pair."""
    g = torch.Generator().manual_seed(3)
    z, w = torch.randn(9, 4, generator=g), torch.randn(2, 4, generator=g)
    known = keys_from_pairs([[(0, 1), (5, 2)], []], 9)
    q = [[0, -1], [1, 4]]
    s, u, v = spec_screen(z, w, q, 4, known)
    got = (s.float(), u.int(), v.int())
    check_screen(z, w, q, 4, got, known)
    bad = [t.clone() for t in got]
    for t in bad:
        t[0, [0, 1]] = t[0, [1, 0]]
    with pytest.raises(AssertionError):
        check_screen(z, w, q, 4, bad, known)
    bad = [t.clone() for t in got]
    bad[1][0, 0], bad[2][0, 0] = 0, 1                                     # a known pair
    with pytest.raises(AssertionError):
        check_screen(z, w, q, 4, bad, known)
    s5, u5, v5 = spec_screen(z, w, q, 5, known)                           # the 5th best in place of the 4th
    bad = [s5[:, [0, 1, 2, 4]].float(), u5[:, [0, 1, 2, 4]].int(), v5[:, [0, 1, 2, 4]].int()]
    with pytest.raises(AssertionError):
        check_screen(z, w, q, 4, bad, known)
    s9, u9, v9 = spec_screen(z, w, q, 9, known)                           # drug query: 8 candidates, 1 padded slot
    check_screen(z, w, q, 9, (s9.float(), u9.int(), v9.int()), known)
    assert int((u9[1] == -1).sum()) == 1
