"""CPU tests of the regimen top-k (include/tipk.h section 4e): the `_supported` predicates, the route query and its option,
argument validation of both C entries (every refusal happens before anything touches a device, so bogus device pointers are
safe here), the host normalisation and the refusals of `TIP.regimen_side_effects`, `ops.restrict_known_relations` against a
Python dict, and the fp64 spec and the acceptance rule (tests/regimen_spec.py) on a hand-worked case."""
import ctypes
import math
import types

import pytest
import torch

from pair_topk_spec import known_from_dict
from regimen_spec import check_regimen_topk, spec_regimen_topk
from tip_amd import _lib, ops
from tip_amd.layers import TIP, RegimenSideEffects, normalize_regimens

EINVAL, EUNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below is refused before a launch


def _dm(n=10, dim=16, n_rel=3, n_reg=4, k=5, agg=0, keys=None, kptr=None, krel=None, n_known=0, z=FAKE, w=FAKE, drugs=FAKE,
        rptr=FAKE, out_s=FAKE, out_r=FAKE, out_p=FAKE):
    return _lib.lib().tipk_distmult_regimen_topk(z, n, dim, w, n_rel, drugs, rptr, n_reg, keys, kptr, krel, n_known, agg, k,
                                                 out_s, out_r, out_p, None, None)


def _tb(n=10, n_rel=3, ld=None, n_reg=4, k=5, agg=0, keys=None, kptr=None, krel=None, n_known=0, s1=FAKE, s2=FAKE,
        drugs=FAKE, rptr=FAKE, out_s=FAKE, out_r=FAKE, out_p=FAKE):
    return _lib.lib().tipk_pair_table_regimen_topk(s1, s2, n_rel if ld is None else ld, n, n_rel, drugs, rptr, n_reg, keys,
                                                   kptr, krel, n_known, agg, k, out_s, out_r, out_p, None)


def test_supported_predicates():
    L = _lib.lib()
    assert L.tipk_abi_version() >= 27
    assert L.tipk_regimen_max_drugs() >= 64 and ops.regimen_max_drugs() == L.tipk_regimen_max_drugs()
    dm, tb = L.tipk_distmult_regimen_topk_supported, L.tipk_pair_table_regimen_topk_supported
    assert dm(645, 4, 1097, 10) == 1 and dm(645, 16, 1097, 10) == 1 and dm(645, 256, 1097, 10) == 1
    for dim in (0, 2, 6, 260):
        assert dm(645, dim, 1097, 10) == 0
    assert dm(645, 16, 1097, 1) == 1 and dm(645, 16, 1097, 128) == 1
    assert dm(645, 16, 1097, 0) == 0 and dm(645, 16, 1097, 129) == 0
    assert dm(645, 16, 1, 4) == 1 and dm(645, 16, 65536, 4) == 1
    assert dm(645, 16, 0, 4) == 0 and dm(645, 16, 65537, 4) == 0
    assert dm(1, 16, 4, 4) == 1 and dm(46340, 256, 65536, 128) == 1
    assert dm(0, 16, 4, 4) == 0 and dm(46341, 16, 4, 4) == 0
    assert tb(1, 1, 1) == 1 and tb(46340, 65536, 128) == 1
    assert tb(0, 4, 4) == 0 and tb(46341, 4, 4) == 0 and tb(645, 0, 4) == 0 and tb(645, 65537, 4) == 0
    assert tb(645, 1097, 0) == 0 and tb(645, 1097, 129) == 0
    ws = L.tipk_distmult_regimen_topk_workspace_bytes
    assert ws(645, 16, 1097, 10000, 10) == 0
    assert ws(46341, 16, 4, 1, 4) == -1 and ws(645, 6, 4, 1, 4) == -1 and ws(645, 16, 4, 1, 129) == -1
    assert ws(645, 16, 4, -1, 4) == -1


def test_route_query_and_option():
    L = _lib.lib()
    assert _lib.get_option('regimen_global') == 0
    assert L.tipk_distmult_regimen_topk_lds_route(16, 1097) == 1         # BioSNAP: 1 097 rows of 80 B beside the waves' state
    assert L.tipk_distmult_regimen_topk_lds_route(64, 2500) == 0         # 2 500 rows of 272 B
    assert L.tipk_distmult_regimen_topk_lds_route(256, 700) == 0
    assert L.tipk_distmult_regimen_topk_lds_route(6, 10) == 0
    _lib.set_option('regimen_global', 1)
    try:
        assert _lib.get_option('regimen_global') == 1
        assert L.tipk_distmult_regimen_topk_lds_route(16, 1097) == 0
    finally:
        _lib.set_option('regimen_global', 0)
    assert L.tipk_distmult_regimen_topk_lds_route(16, 1097) == 1


def test_bad_arguments_einval():
    for call in (_dm, _tb):
        assert call(k=0) == EINVAL
        assert call(k=-3) == EINVAL
        assert call(n_reg=-1) == EINVAL
        assert call(n=0) == EINVAL
        assert call(n_rel=0) == EINVAL
        assert call(n_known=-1) == EINVAL
        assert call(agg=2) == EINVAL and call(agg=-1) == EINVAL           # unknown aggregate
        assert call(agg=1, n_reg=0) == 0                                  # (an empty call: a full one is not refused and,
                                                                          # where a device is present, launches on FAKE)
        assert call(keys=FAKE, n_known=2) == EINVAL                       # known arrays given only in part
        assert call(keys=FAKE, kptr=FAKE, n_known=2) == EINVAL
        assert call(kptr=FAKE, krel=FAKE, n_known=2) == EINVAL
        assert call(krel=FAKE) == EINVAL
        assert call(rptr=None) == EINVAL and call(drugs=None) == EINVAL
        assert call(out_s=None) == EINVAL and call(out_r=None) == EINVAL and call(out_p=None) == EINVAL
    assert _dm(z=None) == EINVAL and _dm(w=None) == EINVAL
    assert _tb(s1=None) == EINVAL and _tb(s2=None) == EINVAL
    assert _dm(dim=0) == EINVAL
    assert _tb(ld=2) == EINVAL                                           # row stride below n_rel
    assert _dm(k=0, dim=6) == EINVAL                                     # argument errors come before shape limits
    assert _dm(agg=7, n=46341) == EINVAL
    assert _tb(k=0, n=46341) == EINVAL


def test_unsupported_shapes_and_empty_list():
    assert _dm(k=129) == EUNSUPPORTED
    assert _dm(dim=2) == EUNSUPPORTED and _dm(dim=6) == EUNSUPPORTED and _dm(dim=260) == EUNSUPPORTED
    assert _dm(n=46341) == EUNSUPPORTED
    assert _dm(n_rel=65537) == EUNSUPPORTED
    assert _dm(w=ctypes.c_void_p((1 << 20) + 4)) == EUNSUPPORTED        # rel_w must be 16-byte aligned
    assert _tb(k=129) == EUNSUPPORTED
    assert _tb(n=46341) == EUNSUPPORTED
    assert _tb(n_rel=65537) == EUNSUPPORTED
    for agg in (0, 1):
        assert _dm(n_reg=0, agg=agg) == 0 and _tb(n_reg=0, agg=agg) == 0  # no regimen: nothing to do, nothing launched
    assert _dm(n_reg=0, z=None, drugs=None, rptr=None, out_s=None, out_r=None, out_p=None) == 0
    assert _dm(n_reg=0, keys=FAKE, kptr=FAKE, krel=FAKE, n_known=3) == 0


def test_ops_refuse_cpu_tensors_and_bad_aggregate():
    drugs, ptr = torch.tensor([0, 1, 2]), torch.tensor([0, 3])
    with pytest.raises(_lib.TipkError):
        ops.distmult_regimen_topk(torch.ones(5, 4), torch.ones(2, 4), drugs, ptr, 2)
    with pytest.raises(_lib.TipkError):
        ops.pair_table_regimen_topk(torch.ones(5, 3), torch.ones(5, 3), drugs, ptr, 2)
    assert ops.REGIMEN_AGGREGATES == {'max': _lib._CONSTANTS['REGIMEN_MAX'], 'noisy_or': _lib._CONSTANTS['REGIMEN_NOISY_OR']}


# ------------------------------------------------------------------ the spec and the rule, by hand
def _hand():
    """4 drugs, 3 relations, dim 4, small integers.  h of the six pairs in pair order:
         (0,1) = (2, 0, 0, 1)   (0,2) = (1, 1, 0, 0)   (0,3) = (0, 0, 0, 2)
         (1,2) = (2, 0, 0, 0)   (1,3) = (0, 0, 1, 2)   (2,3) = (0, 0, 0, 0)
       logits under w0 = (1, 0, 0, 1), w1 = (0, 2, -1, 0), w2 = (1, 1, 1, 1):
         r0:  3, 1, 2, 2, 2, 0        r1:  0, 2, 0, 0, -1, 0        r2:  3, 2, 2, 2, 3, 0"""
    z = torch.tensor([[1.0, 1.0, 0.0, 1.0], [2.0, 0.0, 1.0, 1.0], [1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0]])
    w = torch.tensor([[1.0, 0.0, 0.0, 1.0], [0.0, 2.0, -1.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    return ('distmult', z, w), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 4])


def _sp(x):
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


def test_spec_by_hand():
    m, drugs, ptr = _hand()
    # max: r0 = 3 from pair (0,1); r2 = 3 from (0,1) too (tie with (1,3): the first in pair order); r1 = 2 from (0,2)
    s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, 4, 'max')
    assert r.tolist() == [[0, 2, 1, -1]] and s[0, :3].tolist() == [3.0, 3.0, 2.0] and s[0, 3] == float('-inf')
    assert pi.tolist() == [[0, 0, 0, -1]] and pj.tolist() == [[1, 1, 2, -1]]
    # noisy-or: sums of softplus over the six pairs
    a0 = _sp(3) + _sp(1) + 3 * _sp(2) + _sp(0)
    a1 = _sp(2) + 4 * _sp(0) + _sp(-1)
    a2 = 2 * _sp(3) + 3 * _sp(2) + _sp(0)
    s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, 3, 'noisy_or')
    assert r.tolist() == [[2, 0, 1]] and pi.tolist() == [[0, 0, 0]] and pj.tolist() == [[1, 1, 2]]
    assert s[0].tolist() == pytest.approx([a2, a0, a1], rel=1e-14)
    # r0 known for pair (1,0) only -- listed in the other direction: max falls to 2 with driver (0,3), the first of the 2s;
    # r2 known for every pair: absent
    known = known_from_dict({(1, 0): [0, 2], (0, 2): [2], (3, 0): [2], (1, 2): [2], (1, 3): [2], (2, 3): [2]}, 4)
    s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, 3, 'max', known)
    assert r.tolist() == [[0, 1, -1]] and s[0, :2].tolist() == [2.0, 2.0]
    assert pi.tolist() == [[0, 0, -1]] and pj.tolist() == [[3, 2, -1]]
    s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, 3, 'noisy_or', known)
    assert r.tolist() == [[0, 1, -1]] and pi.tolist() == [[0, 0, -1]] and pj.tolist() == [[3, 2, -1]]
    assert s[0, :2].tolist() == pytest.approx([a0 - _sp(3), a1], rel=1e-14)
    # shorter lists of the same drugs, an empty one, a singleton, one past the maximum length and one with a bad id
    drugs2 = torch.tensor([3, 1, 2, 0, 9, 1] + [0] * 65)
    ptr2 = torch.tensor([0, 2, 2, 3, 4, 6, 71])
    s, r, pi, pj = spec_regimen_topk(m, drugs2, ptr2, 2, 'max')
    assert r.tolist() == [[2, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]       # pair (3, 1): 3, 2 under r2, r0
    assert pi[0].tolist() == [0, 0] and pj[0].tolist() == [1, 1] and s[0].tolist() == [3.0, 2.0]


def test_check_regimen_topk_catches_mistakes():
    g = torch.Generator().manual_seed(2)
    n, R, k = 12, 9, 4
    m = ('distmult', torch.randn(n, 8, generator=g), torch.randn(R, 8, generator=g))
    drugs = torch.tensor([0, 3, 5, 7, 2, 1, 1, 4, 6, 8, 9])
    ptr = torch.tensor([0, 4, 6, 6, 7, 11])
    known = known_from_dict({(0, 3): [0, 4], (2, 1): range(R - 2), (4, 6): [1]}, n)
    for agg in ('max', 'noisy_or'):
        s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, k, agg, known)
        good = (s.float(), r.int(), pi.int(), pj.int())
        check_regimen_topk(m, drugs, ptr, k, agg, good, known)
        assert r[1, 2:].tolist() == [-1, -1] and r[2].tolist() == [-1] * k and r[3].tolist() == [-1] * k

        def planted(fn):
            bad = [x.clone() for x in good]
            fn(*bad)
            with pytest.raises(AssertionError):
                check_regimen_topk(m, drugs, ptr, k, agg, tuple(bad), known)

        def swap(s, r, pi, pj):
            for x in (s, r, pi, pj):
                x[0, [0, 1]] = x[0, [1, 0]]

        def not_candidate(s, r, pi, pj):
            r[1, 1] = 0

        def duplicate(s, r, pi, pj):
            r[4, 3], s[4, 3] = r[4, 2], s[4, 2]

        def off_score(s, r, pi, pj):
            s[4, 0] = s[4, 0] * 1.001 + 0.001

        def short_row(s, r, pi, pj):
            s[4, 3], r[4, 3], pi[4, 3], pj[4, 3] = float('-inf'), -1, -1, -1

        def overfull_row(s, r, pi, pj):
            s[2, 0], r[2, 0], pi[2, 0], pj[2, 0] = 0.0, 1, 0, 1

        def pad_pair(s, r, pi, pj):
            pi[1, 3] = 0

        def pair_outside(s, r, pi, pj):
            pj[1, 0] = 2

        def pair_reversed(s, r, pi, pj):
            pi[0, 0], pj[0, 0] = pj[0, 0].clone(), pi[0, 0].clone()

        for fn in (swap, not_candidate, duplicate, off_score, short_row, overfull_row, pad_pair, pair_outside, pair_reversed):
            planted(fn)
    # a driver that contributes but is far from the best pair; a driver whose triple is known
    s, r, pi, pj = spec_regimen_topk(m, drugs, ptr, R, 'noisy_or', known)
    L0 = torch.einsum('pk,rk->pr', m[1][[0, 0, 0, 3, 3, 5]].double() * m[1][[3, 5, 7, 5, 7, 7]].double(), m[2].double())
    slot = 0
    worst = int(L0[1:, int(r[0, slot])].argmin()) + 1                     # (pair 0 = (0, 3) may be known)
    ij = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)][worst]
    if (int(pi[0, slot]), int(pj[0, slot])) != ij:
        bad = (s.float(), r.int(), pi.int().clone(), pj.int().clone())
        bad[2][0, slot], bad[3][0, slot] = ij
        with pytest.raises(AssertionError, match='best pair'):
            check_regimen_topk(m, drugs, ptr, R, 'noisy_or', bad, known)
    at = r[0].tolist().index(4)                                           # relation 4 is known for (0, 3) = positions (0, 1)
    bad = (s.float(), r.int(), pi.int().clone(), pj.int().clone())
    bad[2][0, at], bad[3][0, at] = 0, 1
    with pytest.raises(AssertionError, match='contribute'):
        check_regimen_topk(m, drugs, ptr, R, 'noisy_or', bad, known)


# ------------------------------------------------------------------ host normalisation, TIP refusals
def test_normalize_regimens():
    drugs, ptr = normalize_regimens([[5, 3, 3, 1], [], [7], [9, 2], [4, 4]], 10, 64)
    assert drugs.dtype == torch.int32 and ptr.dtype == torch.int64
    assert drugs.tolist() == [1, 3, 5, 7, 2, 9, 4] and ptr.tolist() == [0, 3, 3, 4, 6, 7]
    d2, p2 = normalize_regimens((torch.tensor([5, 3, 3, 1, 7, 9, 2, 4, 4]), torch.tensor([0, 4, 4, 5, 7, 9])), 10, 64)
    assert d2.tolist() == drugs.tolist() and p2.tolist() == ptr.tolist()
    d3, p3 = normalize_regimens([], 10, 64)
    assert d3.tolist() == [] and p3.tolist() == [0]
    d4, p4 = normalize_regimens([list(range(64)) + [0, 1]], 100, 64)      # 66 entries, 64 distinct: legal
    assert d4.tolist() == list(range(64)) and p4.tolist() == [0, 64]
    with pytest.raises(ValueError, match='at most 64'):
        normalize_regimens([[1, 2], list(range(65))], 100, 64)
    for bad in ([[0, 10]], [[-1, 2]], (torch.tensor([0, 11]), torch.tensor([0, 2]))):
        with pytest.raises(ValueError, match='out of range'):
            normalize_regimens(bad, 10, 64)
    for bad in ((torch.tensor([0, 1]), torch.tensor([0, 3])), (torch.tensor([0, 1]), torch.tensor([1, 2])),
                (torch.tensor([0, 1, 2]), torch.tensor([0, 2, 1, 3])), (torch.tensor([0.0, 1.0]), torch.tensor([0, 2])),
                [1, 2, 3], [['a']]):
        with pytest.raises(ValueError, match='regimens'):
            normalize_regimens(bad, 10, 64)


def test_tip_regimen_side_effects_refusals():
    data = types.SimpleNamespace(n_drug=10)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.regimen_side_effects(types.SimpleNamespace(decoder_kind='distmult', shard=object(), data=data), [[0, 1]], k=5)
    for kind in ('distmult', 'nn'):
        self = types.SimpleNamespace(decoder_kind=kind, shard=None, data=data)
        for bad in ('test', 'none', 0):
            with pytest.raises(ValueError, match='exclude'):
                TIP.regimen_side_effects(self, [[0, 1]], k=5, exclude=bad)
        for bad in ('sum', 'noisy-or', None, 1):
            with pytest.raises(ValueError, match='aggregate'):
                TIP.regimen_side_effects(self, [[0, 1]], k=5, aggregate=bad)
        with pytest.raises(ValueError, match='out of range'):
            TIP.regimen_side_effects(self, [[0, 1], [3, 10]], k=5)
        with pytest.raises(ValueError, match='out of range'):
            TIP.regimen_side_effects(self, (torch.tensor([0, -1]), torch.tensor([0, 2])), k=5)
        big = types.SimpleNamespace(decoder_kind=kind, shard=None, data=types.SimpleNamespace(n_drug=100))
        with pytest.raises(ValueError, match='at most'):
            TIP.regimen_side_effects(big, [list(range(ops.regimen_max_drugs() + 1))], k=5)
    assert RegimenSideEffects._fields == ('score', 'relation', 'u', 'v')


# ------------------------------------------------------------------ restrict_known_relations
def test_restrict_known_relations_vs_dict():
    g = torch.Generator().manual_seed(9)
    n, R = 11, 17
    d = {}
    for u, v in torch.randint(0, n, (40, 2), generator=g).tolist():
        d[(min(u, v), max(u, v))] = torch.nonzero(torch.rand(R, generator=g) < 0.4).reshape(-1).tolist()
    d[(0, 0)] = list(range(R))
    d[(n - 1, n - 1)] = [3]                                               # loses every entry for most subsets
    known = known_from_dict(d, n)
    for sub in ([4, 1, 5], [16], [0, 2, 3, 7, 8, 15, 1], list(range(R)), list(reversed(range(R)))):
        got = ops.restrict_known_relations(known, torch.tensor(sub), R)
        keys, ptr, rel = (t.tolist() for t in got)
        assert keys == known[0].tolist() and got[2].dtype == torch.int32 and len(ptr) == len(keys) + 1
        for i, key in enumerate(keys):
            want = sorted(sub.index(r) for r in d[(key // n, key % n)] if r in sub)
            assert rel[ptr[i]:ptr[i + 1]] == want, (sub, key)
        assert ptr[0] == 0 and ptr[-1] == len(rel)
