"""No device: the fp64 statement of the protein attribution (tests/protein_attribution_spec.py) against torch.autograd on
every case of tests/protein_attribution_cases.py, the acceptance rule against the spec's own output and against results that
are wrong in one way each, the graph builders of tip_amd.ops, the C entry's statuses and `TIP.explain_proteins`'s refusals."""
import types

import pytest
import torch

import protein_attribution_cases as cases
from protein_attribution_spec import Spec, check_protein_attribution, forward64, spec_protein_attribution
from tip_amd import _lib, ops
from tip_amd.layers import TIP, ProteinExplanation

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.mark.parametrize('shape', cases.SHAPES, ids=cases.shape_id)
def test_spec_is_gradient_times_input(shape):
    op, spec, q, probe = cases.case(shape)
    n, cat = shape[0], op.cat
    roles = op.dd[1].bincount(minlength=n)
    assert int(roles[cases.ONE]) == 1 and int(roles[cases.ISOLATED]) == 0 and int(roles[cases.ZEROH]) == 0
    assert not bool((op.dd[0] == cases.ISOLATED).any()) and bool((op.dd[0] == cases.ZEROH).any())
    assert int(roles[cases.HUB]) >= n - 2 and not bool((op.dd[2] == shape[2] - 1).any())     # a relation without edges
    assert bool((op.h[cases.ZEROH] == 0).all()) and bool((op.h[cases.ISOLATED] > 0).any())
    targeted = op.pd_edges[1].bincount(minlength=n)
    assert int(targeted[cases.NOTARGET]) == 0 and int(targeted[cases.ZEROH]) == 0
    assert int(spec.entries[cases.EVERY]) == n - 2 and int(spec.entries[-1]) == 0 and int(spec.cand.sum()) == shape[1] - 1
    assert int(((op.pd_edges[0] == cases.DUP) & (op.pd_edges[1] == cases.HUB)).sum()) >= 2
    dbl = lambda ts: tuple(t.double() for t in ts)
    for i, v in enumerate(q.tolist()):
        if v < 0 or v >= n:
            continue
        hp, xe = op.hp.double().requires_grad_(), op.xe.double().requires_grad_()
        _, h64, z = forward64(hp, op.w_pd.double(), xe, dbl(op.layer1), dbl(op.layer2), op.dd, op.pd_edges, cat)
        assert torch.equal(h64 > 0, op.h > 0)                            # h recomputed in fp64: the same mask
        value = (probe[i].double() * z[v]).sum()
        g_hp, g_xe = torch.autograd.grad(value, (hp, xe))
        e = spec.values(v, probe[i])
        tol = 1e-10 * e['S'] + 1e-300
        own = (g_xe * xe.detach()).sum(1)
        c = (g_hp * hp.detach()).sum(1)
        assert float((e['own'] - own).abs().max()) <= tol and float((e['c'] - c).abs().max()) <= tol, (shape, i)
        assert abs(float(e['own'].sum() + e['c'].sum()) - float(value.detach())) <= tol, (shape, i)
        assert bool((e['c'][~e['cand']] == 0).all())


@pytest.mark.parametrize('shape', cases.SHAPES, ids=cases.shape_id)
def test_rule_accepts_the_spec(shape):
    op, spec, q, probe = cases.case(shape)
    k = shape[9]
    c, p, d, f, s = spec_protein_attribution(spec, q, probe, k)
    res = check_protein_attribution(spec, q, probe, k, (c.float(), p.int(), d.float(), f.float(), s.float()), 'spec')
    assert max(res[key] for key in ('used_value', 'used_direct', 'used_features', 'used_proteins')) <= 1.0
    n_cand = shape[1] - 1
    assert (p >= 0).sum(1).tolist() == [min(k, n_cand)] * 9 + [0, 0]
    m = min(k, n_cand)
    assert p[7, :m].tolist() == list(range(m)) and bool((c[7, :m] == 0).all())      # the zero probe: ties, by protein id
    assert bool((d[4] == 0).all()) and bool((d[5] == 0).all())                        # no target: nothing arrives directly
    assert bool(f[9:].isnan().all()) and bool(s[9:].isnan().all())


def test_rule_rejects_what_it_must():
    shape = cases.SHAPES[2]
    op, spec, q, probe = cases.case(shape)
    k = 5
    q, probe = q[:4], probe[:4]
    full = spec_protein_attribution(spec, q, probe, k + 1)
    c, p, d, f, s = spec_protein_attribution(spec, q, probe, k)
    good = (c.float(), p.int(), d.float(), f.float(), s.float())
    check_protein_attribution(spec, q, probe, k, good, 'good')
    e = spec.values(int(q[0]), probe[0])

    def broken(what, fn):
        bad = [t.clone() for t in good]
        fn(bad)
        with pytest.raises(AssertionError):
            check_protein_attribution(spec, q, probe, k, tuple(bad), what)

    def swap(b):
        for t in b[:3]:
            t[0, [0, 1]] = t[0, [1, 0]]

    def drop_best(b):                                                    # ranks 2 .. k + 1 instead of 1 .. k
        b[0][0], b[1][0], b[2][0] = full[0][0, 1:].float(), full[1][0, 1:].int(), full[2][0, 1:].float()

    assert c[0, 0] != c[0, 1] and float(e['tau'][p[0, 0]]) > 0
    broken('a swapped pair', swap)
    broken('a larger protein is missing', drop_best)
    broken('a wrong direct', lambda b: b[2].__setitem__((0, 0), b[2][0, 0] + 2 * float(e['tau_direct'][p[0, 0]]) + 1e-3))
    broken('a value off by 2 tau', lambda b: b[0].__setitem__((0, 0), b[0][0, 0] + 2 * float(e['tau'][p[0, 0]])))
    broken('an untargeted protein', lambda b: b[1].__setitem__((0, 0), shape[1] - 1))
    broken('a protein listed twice', lambda b: [t.__setitem__((0, 1), t[0, 0]) for t in b[:3]])
    broken('padding inside the list', lambda b: b[1].__setitem__((0, 2), -1))
    broken('features off', lambda b: b[3].__setitem__(0, b[3][0] + 1e-2))
    broken('proteins off', lambda b: b[4].__setitem__(0, b[4][0] + 1e-2))


def test_graph_builders_on_the_host():
    ei = torch.tensor([[0, 1, 3, 1, 0, 3, 3, 2], [1, 2, 1, 1, 1, 3, 1, 1]])
    et = torch.tensor([0, 1, 1, 0, 2, 0, 0, 0])
    n = 5
    ptr_n, src_n, rel_n = ops.in_edges_by_node(ei, et, n)
    ptr_p, src_p, rel_p = ops.in_edges_by_pair(ei, et, n)
    assert torch.equal(ptr_n, ptr_p) and ptr_p.tolist() == [0, 0, 6, 7, 8, 8]
    assert src_p[:6].tolist() == [0, 0, 1, 2, 3, 3] and rel_p[:6].tolist() == [0, 2, 0, 0, 0, 1]
    # the edges of one pair keep the order they have in the (relation, source) segment
    for s in range(n):
        assert rel_n[:6][src_n[:6] == s].tolist() == rel_p[:6][src_p[:6] == s].tolist()
    assert ops.in_edges_by_pair(ei, et, n)[1] is src_p                   # cached per edge tensors
    with pytest.raises(IndexError):
        ops.in_edges_by_pair(ei, et, 3)
    n_prot = 4
    dp = torch.tensor([[2, 0, 2, 0, 2], [n_prot + 1, n_prot + 3, n_prot + 0, n_prot + 3, n_prot + 1]])
    prot_ptr, prot_drug, inv_cnt, cnt = ops.targets_by_protein(dp, n_prot, n)
    assert prot_ptr.tolist() == [0, 2, 2, 5, 5] and prot_drug.tolist() == [3, 3, 0, 1, 1] and cnt.tolist() == [1, 2, 0, 2, 0]
    assert inv_cnt.tolist() == [1.0, 0.5, 1.0, 0.5, 1.0] and prot_drug.dtype == torch.int32 and inv_cnt.dtype == torch.float32
    with pytest.raises(IndexError, match='drug'):
        ops.targets_by_protein(dp, n_prot, 3)
    with pytest.raises(IndexError, match='protein'):
        ops.targets_by_protein(dp, 2, n + 2)


_NAMES = ('hp', 'w_pd', 'xe', 'h', 'basis1', 'att1', 'root1', 'basis2', 'att2', 'root2', 'pe_ptr', 'pe_src', 'pe_rel', 'prot_ptr',
          'prot_drug', 'inv_cnt', 'q_node', 'probe', 'oc', 'op', 'od', 'of', 'os', 'ws')


def _call(k=3, n_q=1, null=None, n=6, n_prot=4, n_rel=2, B=1, ne=3, pd=2, p=2, d1=4, d2=4, cat=1, n_edges=7, n_pd=5, ld_h=None,
          ws=4096):
    """tipk_protein_attribution with fake non-NULL addresses (nothing is launched on the paths tested here)."""
    a = {name: 4096 for name in _NAMES}
    a['ws'] = ws
    if null:
        a[null] = None
    return _lib.lib().tipk_protein_attribution(
        a['hp'], p, n_prot, p, a['w_pd'], pd, a['xe'], ne, ne, a['h'], d1 if ld_h is None else ld_h, n, d1, a['basis1'], a['att1'], B,
        a['root1'], a['basis2'], a['att2'], B, a['root2'], d2, n_rel, B, a['pe_ptr'], a['pe_src'], a['pe_rel'], n_edges,
        a['prot_ptr'], a['prot_drug'], n_pd, a['inv_cnt'], cat, a['q_node'], a['probe'], d2, n_q, k, a['oc'], a['op'], a['od'],
        a['of'], a['os'], a['ws'], None)


def test_c_entry_statuses_without_a_device():
    L = _lib.lib()
    for name in ('tipk_protein_attribution_supported', 'tipk_protein_attribution_workspace_bytes',
                 'tipk_protein_attribution_chunk', 'tipk_protein_attribution'):
        assert name in _lib.SIGNATURES, name                            # the binding read them from the header unaided
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30          # the section is purely additive
    assert L.tipk_protein_attribution_chunk() == cases.CHUNK
    sup = L.tipk_protein_attribution_supported                           # (n, P, R, B, ne, pd, p, d1, d2, cat, k)
    assert sup(645, 19081, 1097, 32, 48, 16, 16, 32, 16, 1, 10) == 1
    for shape in cases.SHAPES:
        n, P, R, B, ne, pd, p, d1, d2, k, mode = shape
        assert sup(n, P, R, B, ne, pd, p, d1, d2, int(mode == 'cat'), k) == 1, shape
    assert sup(4096, 19081, 1097, 64, 64, 64, 128, 128, 128, 1, 1024) == 1 and sup(4097, 19081, 1097, 32, 48, 16, 16, 32, 16, 1, 10) == 0
    assert sup(645, 19081, 1097, 65, 48, 16, 16, 32, 16, 1, 10) == 0 and sup(645, 19081, 1097, 32, 48, 16, 16, 32, 16, 1, 1025) == 0
    assert sup(645, 19081, 1097, 32, 48, 16, 16, 129, 16, 1, 10) == 0 and sup(645, 19081, 1097, 32, 48, 16, 16, 32, 129, 1, 10) == 0
    assert sup(645, 19081, 1097, 32, 48, 16, 129, 32, 16, 1, 10) == 0 and sup(645, 19081, 1097, 32, 100, 29, 16, 32, 16, 1, 10) == 0
    assert sup(645, 19081, 1097, 32, 128, 128, 16, 32, 16, 0, 10) == 1 and sup(645, 19081, 1097, 32, 48, 16, 16, 32, 16, 0, 10) == 0
    assert sup(645, 19081, 1097, 32, 48, 16, 16, 32, 16, 1, 0) == 0 and sup(0, 19081, 1097, 32, 48, 16, 16, 32, 16, 1, 10) == 0
    ws = L.tipk_protein_attribution_workspace_bytes                      # (n, B, d1, p, n_q)
    assert ws(645, 32, 32, 16, 1) == (2 * 645 * 645 * 32 + 645 * 49) * 4
    assert ws(645, 32, 32, 16, 4096) == ws(645, 32, 32, 16, 256) == (2 * 645 * 645 * 32 + 256 * 645 * 49) * 4
    assert ws(645, 32, 32, 16, 0) == 2 * 645 * 645 * 32 * 4
    assert ws(4097, 32, 32, 16, 1) == -1 and ws(645, 65, 32, 16, 1) == -1 and ws(645, 32, 129, 16, 1) == -1 and ws(645, 32, 32, 16, -1) == -1
    # statuses: EINVAL first, then EUNSUPPORTED, and n_q == 0 is OK with no launch
    assert _call(k=0) == EINVAL and _call(k=-1) == EINVAL and _call(n_q=-1) == EINVAL and _call(n_edges=-1) == EINVAL
    assert _call(n_pd=-1) == EINVAL and _call(ld_h=3) == EINVAL and _call(cat=0) == EINVAL and _call(n=0) == EINVAL
    for name in _NAMES:
        assert _call(null=name) == EINVAL, name
    assert _call(ws=4098) == EINVAL                                      # a workspace that is not 4-byte aligned
    assert _call(k=0, d1=129) == EINVAL                                  # EINVAL wins over EUNSUPPORTED
    assert _call(k=1025) == EUNSUPPORTED and _call(d1=129) == EUNSUPPORTED and _call(B=65) == EUNSUPPORTED
    assert _call(n=4097) == EUNSUPPORTED and _call(ne=100, pd=29) == EUNSUPPORTED
    assert _call(n_q=0) == OK and _call(n_q=0, null='ws') == OK and _call(n_q=0, k=1024, d1=128, d2=128, B=64) == OK
    assert _call(n_q=0, k=1025) == EUNSUPPORTED and _call(n_q=0, k=0) == EINVAL


def test_op_refuses_host_tensors():
    op, spec, q, probe = cases.case(cases.SHAPES[0])
    src, dst, rel = op.dd
    pair = ops.in_edges_by_pair(torch.stack([src, dst]), rel, 6)
    tg = ops.targets_by_protein(torch.stack([op.pd_edges[0], op.pd_edges[1] + 4]), 4, 6)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.protein_attribution(op.hp, op.w_pd, op.xe, op.h, op.layer1, op.layer2, pair, tg, True, q, probe, 3)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.protein_attribution(op.hp.double(), op.w_pd, op.xe, op.h, op.layer1, op.layer2, pair, tg, True, q, probe, 3)
    assert ops.protein_attribution_supported(6, 4, 2, 1, 3, 2, 2, 4, 4, True, 3)
    assert not ops.protein_attribution_supported(6, 4, 2, 1, 3, 2, 2, 4, 4, False, 3)


def test_explain_proteins_refusals():
    assert ProteinExplanation._fields == ('logit', 'offset', 'features', 'proteins', 'contribution', 'protein', 'direct', 'targets')
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.explain_proteins(types.SimpleNamespace(shard=object()))
    bare = types.SimpleNamespace(shard=None)
    with pytest.raises(ValueError, match='side'):
        TIP.explain_proteins(bare, side='w')
    with pytest.raises(ValueError, match='direction'):
        TIP.explain_proteins(bare, direction='down')
    layer = types.SimpleNamespace(bias=None, shard=None, num_bases=32, out_channels=32)
    biased = types.SimpleNamespace(bias=torch.zeros(1), shard=None, num_bases=32, out_channels=16)
    enc = types.SimpleNamespace(rgcn1=layer, rgcn2=biased)
    with pytest.raises(NotImplementedError, match='bias'):
        TIP.explain_proteins(types.SimpleNamespace(shard=None, data=None, encoder=enc))
    enc = types.SimpleNamespace(rgcn1=layer, rgcn2=types.SimpleNamespace(bias=None, shard=None, num_bases=32, out_channels=16),
                                embed=torch.zeros(3, 48), mod='cat', pp_encoder=types.SimpleNamespace(out_dim=16),
                                hgcn=types.SimpleNamespace(out_dim=16))
    data = types.SimpleNamespace(n_drug=5000, n_prot=100, n_dd_et=7)
    with pytest.raises(NotImplementedError, match='sizes'):                   # more drugs than the dense cells take
        TIP.explain_proteins(types.SimpleNamespace(shard=None, data=data, encoder=enc))
    data = types.SimpleNamespace(n_drug=645, n_prot=100, n_dd_et=7, dd_test_idx=torch.zeros(2, 3, dtype=torch.int64),
                                 dd_test_et=torch.zeros(3, dtype=torch.int64))
    model = types.SimpleNamespace(shard=None, data=data, encoder=enc, embeddings=torch.zeros(1))
    with pytest.raises(NotImplementedError, match='max_workspace_bytes'):
        TIP.explain_proteins(model, max_workspace_bytes=1 << 20)
