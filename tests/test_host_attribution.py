"""Not gpu: the host side of the R-GCN edge attribution (include/tipk.h section 4j) -- the in-edge CSR builder against a
Python loop, both decoders' probe builders against autograd in fp64, the C entry's statuses without a device, the refusals
of the op and of `TIP.explain`, and the fp64 spec (tests/attribution_spec.py) against itself and the identity it rests on."""
import types

import pytest
import torch

import attribution_cases as cases
from attribution_spec import check_attribution, rgcn_layer64, spec_attribution
from tip_amd import _lib, ops
from tip_amd.layers import TIP, Explanation, MultiInnerProductDecoder, MyRGCNConv2, NNDecoder

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _tiny_graph():
    """5 nodes, 3 relations: duplicates (0 -> 1 twice under relation 0), a self loop (2 -> 2), an isolated node (4) and an
    empty relation (1), as a range_list graph (edges grouped by relation)."""
    ei = torch.tensor([[0, 0, 3, 2, 1, 2, 0, 3],
                       [1, 1, 1, 2, 0, 1, 3, 0]])
    ranges = torch.tensor([[0, 4], [4, 4], [4, 8]])
    et = torch.tensor([0, 0, 0, 0, 2, 2, 2, 2])
    return ei, ranges, et


def _loop_csr(ei, et, n):
    ptr, src, rel = [0], [], []
    for v in range(n):
        seg = sorted((int(et[e]), int(ei[0, e])) for e in range(ei.shape[1]) if int(ei[1, e]) == v)
        src += [s for _, s in seg]
        rel += [r for r, _ in seg]
        ptr.append(len(src))
    return ptr, src, rel


def test_in_edges_by_node_against_a_loop():
    ei, ranges, et = _tiny_graph()
    ptr, src, rel = _loop_csr(ei, et, 5)
    assert ptr == [0, 2, 6, 7, 8, 8]                                     # in-degree, duplicates counted; node 4 isolated
    for second in (ranges, et, ranges.tolist()):
        in_ptr, in_src, in_rel = ops.in_edges_by_node(ei, second, 5)
        assert in_ptr.dtype == torch.int64 and in_src.dtype == torch.int32 and in_rel.dtype == torch.int32
        assert in_ptr.tolist() == ptr and in_src.tolist() == src and in_rel.tolist() == rel
    assert in_src.tolist()[2:6] == [0, 0, 3, 2] and in_rel.tolist()[2:6] == [0, 0, 0, 2]   # node 1: (relation, source) order
    a = ops.in_edges_by_node(ei, ranges, 5)
    assert ops.in_edges_by_node(ei, ranges, 5)[1] is a[1]                # cached per edge tensor
    perm = torch.tensor([7, 2, 5, 0, 3, 6, 1, 4])                        # edge order does not matter with edge_type
    in_ptr, in_src, in_rel = ops.in_edges_by_node(ei[:, perm], et[perm], 5)
    assert in_ptr.tolist() == ptr and in_src.tolist() == src and in_rel.tolist() == rel
    with pytest.raises(IndexError):
        ops.in_edges_by_node(ei, ranges, 3)
    with pytest.raises(_lib.TipkError):
        ops.in_edges_by_node(ei, torch.tensor([[0, 4], [4, 7]]), 5)
    empty = ops.in_edges_by_node(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3)
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1].numel() == 0


@pytest.mark.parametrize('kind', ['distmult', 'nn'])
@pytest.mark.parametrize('side', ['u', 'v'])
def test_probe_is_the_gradient_of_the_logit(kind, side):
    torch.manual_seed(3)
    n, d, R, T = 9, 6, 4, 11
    dec = (MultiInnerProductDecoder(d, R) if kind == 'distmult' else NNDecoder(d, R, l1_dim=5)).double()
    z = torch.randn(n, d, dtype=torch.float64)
    idx, et = torch.randint(0, n, (2, T)), torch.randint(0, R, (T,))

    def logit(zu, zv):                                                   # the plain-torch formula, rows of z as leaves
        if kind == 'distmult':
            return (zu * dec.weight[et] * zv).sum(1)
        return (torch.relu(zu @ dec.w1_l1) * dec.w1_l2[et]).sum(1) + (torch.relu(zv @ dec.w2_l1) * dec.w2_l2[et]).sum(1)

    zu, zv = z[idx[0]].clone().requires_grad_(True), z[idx[1]].clone().requires_grad_(True)
    want = logit(zu, zv)
    grad = torch.autograd.grad(want.sum(), zv if side == 'v' else zu)[0]
    node, probe, offset = dec.probe(z, idx, et, side)
    assert node.dtype == torch.int64 and torch.equal(node, idx[1] if side == 'v' else idx[0])
    assert probe.shape == (T, d) and offset.shape == (T,) and not probe.requires_grad
    torch.testing.assert_close(probe, grad, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(offset + (probe * z[node]).sum(1), want.detach(), rtol=1e-13, atol=1e-13)
    if kind == 'distmult':
        assert bool((offset == 0).all())


def _call(k=3, n_q=1, null=None, n=5, n_rel=2, B=1, d_in=4, d_out=4, n_edges=7):
    """tipk_rgcn_attribution with fake non-NULL addresses (nothing is launched on the paths tested here)."""
    p = {name: 4096 for name in ('h', 'basis', 'att', 'root', 'in_ptr', 'in_src', 'in_rel', 'q_node', 'probe', 'oc', 'os',
                                 'or', 'own', 'sum')}
    if null:
        p[null] = None
    return _lib.lib().tipk_rgcn_attribution(p['h'], d_in, n, d_in, p['basis'], p['att'], B, n_rel, B, p['root'], d_out,
                                            p['in_ptr'], p['in_src'], p['in_rel'], n_edges, p['q_node'], p['probe'], d_out,
                                            n_q, k, p['oc'], p['os'], p['or'], p['own'], p['sum'], None, None)


def test_c_entry_statuses_without_a_device():
    L = _lib.lib()
    for name in ('tipk_rgcn_attribution_supported', 'tipk_rgcn_attribution_lds_route',
                 'tipk_rgcn_attribution_workspace_bytes', 'tipk_rgcn_attribution'):
        assert name in _lib.SIGNATURES, name                            # the binding read them from the header unaided
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30
    sup = L.tipk_rgcn_attribution_supported
    assert sup(645, 1097, 32, 32, 16, 10) == 1
    assert sup(645, 1097, 32, 32, 16, 1024) == 1 and sup(645, 1097, 32, 32, 16, 1025) == 0
    assert sup(645, 1097, 32, 128, 128, 10) == 1 and sup(645, 1097, 32, 129, 16, 10) == 0 and sup(645, 1097, 32, 32, 129, 10) == 0
    assert sup(645, 1097, 64, 32, 16, 10) == 1 and sup(645, 1097, 65, 32, 16, 10) == 0
    assert sup(46340, 65536, 1, 1, 1, 1) == 1 and sup(46341, 1097, 32, 32, 16, 10) == 0 and sup(645, 65537, 32, 32, 16, 10) == 0
    assert sup(0, 1097, 32, 32, 16, 10) == 0 and sup(645, 1097, 32, 32, 16, 0) == 0 and sup(37, 7, 2, 7, 3, 8) == 1
    # statuses: EINVAL first, then EUNSUPPORTED, and n_q == 0 is OK with no launch
    assert _call(k=0) == EINVAL and _call(k=-1) == EINVAL and _call(n_q=-1) == EINVAL and _call(n_edges=-1) == EINVAL
    for name in ('h', 'basis', 'att', 'root', 'in_ptr', 'in_src', 'in_rel', 'q_node', 'probe', 'oc', 'os', 'or', 'own', 'sum'):
        assert _call(null=name) == EINVAL, name
    assert _call(k=0, d_in=129) == EINVAL                                # EINVAL wins over EUNSUPPORTED
    assert _call(k=1025) == EUNSUPPORTED and _call(d_in=129) == EUNSUPPORTED and _call(B=65) == EUNSUPPORTED
    assert _call(n_q=0) == OK and _call(n_q=0, k=1024, d_in=128, d_out=128, B=64) == OK
    assert _call(n_q=0, k=1025) == EUNSUPPORTED and _call(n_q=0, k=0) == EINVAL
    # routes and workspace
    route, ws = L.tipk_rgcn_attribution_lds_route, L.tipk_rgcn_attribution_workspace_bytes
    assert _lib.get_option('attribution_global') == 0
    assert route(645, 32) == 1 and ws(645, 32, 16384) == 0               # BioSNAP: the table lives in LDS
    assert route(46340, 64) == 0 and ws(46340, 64, 1) == 46340 * 64 * 4
    assert ws(46340, 64, 10 ** 6) == ws(46340, 64, 256)                  # one slice per workgroup, a bounded number of them
    assert ws(645, 32, -1) == -1 and ws(0, 32, 1) == -1 and ws(645, 65, 1) == -1
    _lib.set_option('attribution_global', 1)
    try:
        assert route(645, 32) == 0 and ws(645, 32, 3) == 3 * 645 * 32 * 4
        assert _call() == EINVAL                                         # the global route needs a workspace
    finally:
        _lib.set_option('attribution_global', 0)
    assert route(645, 32) == 1


def test_op_refuses_host_tensors_and_wrong_shapes():
    ei, ranges, _ = _tiny_graph()
    in_edges = ops.in_edges_by_node(ei, ranges, 5)
    h, basis, att, root = cases.operands(5, 3, 2, 4, 3, 0)
    q, g = torch.tensor([1]), torch.ones(1, 3)
    with pytest.raises(_lib.TipkError, match='device'):
        ops.rgcn_edge_attribution(h, basis, att, root, in_edges, q, g, 2)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.rgcn_edge_attribution(h.double(), basis, att, root, in_edges, q, g, 2)
    layer = MyRGCNConv2(4, 3, 3, 2, after_relu=True, bias=True)
    with pytest.raises(NotImplementedError, match='bias'):
        layer.attribute(h, ei, ranges, q, g, 2)
    layer = MyRGCNConv2(4, 3, 3, 2, after_relu=True)
    layer.shard = object()
    with pytest.raises(NotImplementedError, match='shard'):
        layer.attribute(h, ei, ranges, q, g, 2)
    layer.shard = None
    with pytest.raises(_lib.TipkError, match='device'):
        layer.attribute(h, ei, ranges, q, g, 2)


def test_explain_refusals():
    assert Explanation._fields == ('logit', 'offset', 'own', 'neighbours', 'contribution', 'partner', 'relation', 'degree')
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.explain(types.SimpleNamespace(shard=object()))
    bare = types.SimpleNamespace(shard=None)
    with pytest.raises(ValueError, match='side'):
        TIP.explain(bare, side='w')
    with pytest.raises(ValueError, match='direction'):
        TIP.explain(bare, direction='down')


def test_spec_against_itself_and_the_identity():
    ei, ranges, et = _tiny_graph()
    n, R, B, d_in, d_out, k = 5, 3, 2, 4, 3, 3
    in_edges = ops.in_edges_by_node(ei, ranges, n)
    h, basis, att, root = (t.double() for t in cases.operands(n, R, B, d_in, d_out, 7))
    q = torch.tensor([0, 1, 2, 3, 4, 1, -1, 5])
    g = torch.randn(q.numel(), d_out, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    c, s, r, own, total, pos = spec_attribution(h, basis, att, root, in_edges, q, g, k)
    # the identity: probe . z[v] == own + the sum of all contributions, to fp64 rounding
    z = rgcn_layer64(h, basis, att, root, ei, et)
    ok = q.clamp(0, n - 1)[:6]
    torch.testing.assert_close(own[:6] + total[:6], (g[:6] * z[ok]).sum(1), rtol=1e-13, atol=1e-14)
    assert bool(own[6:].isnan().all()) and bool(total[6:].isnan().all())
    assert total[4] == 0 and bool((s[4] == -1).all()) and bool(torch.isneginf(c[4]).all())      # the isolated node
    for i in range(q.numel()):                                          # ordered: value descending, ties by position
        m = int((pos[i] >= 0).sum())
        keys = [(-float(c[i, j]), int(pos[i, j])) for j in range(m)]
        assert keys == sorted(keys) and len(set(pos[i, :m].tolist())) == m
    assert (pos >= 0).sum(1).tolist() == [2, 3, 1, 1, 0, 3, 0, 0]        # min(k, deg); padding beyond
    # the spec's own result, rounded to fp32, passes the rule: one rounding per value is inside tau
    good = (c.float(), s.int(), r.int(), own.float(), total.float())
    res = check_attribution(h, basis, att, root, in_edges, q, g, k, good, 'spec')
    assert res['used_edge'] <= 1.0 and res['used_own'] <= 1.0 and res['used_total'] <= 1.0
    torch.testing.assert_close(res['own64'][:6], own[:6], rtol=0, atol=0)
    torch.testing.assert_close(res['total64'][:6], total[:6], rtol=0, atol=0)

    # and the rule catches what it must
    def broken(i, fn):
        bad = [t.clone() for t in good]
        fn(bad)
        with pytest.raises(AssertionError):
            check_attribution(h, basis, att, root, in_edges, q, g, k, tuple(bad), 'broken %d' % i)

    def swap(b):
        b[0][1, [0, 1]], b[1][1, [0, 1]], b[2][1, [0, 1]] = b[0][1, [1, 0]], b[1][1, [1, 0]], b[2][1, [1, 0]]

    def drop_best(b):                                                    # node 1 has 4 edges, k = 3: list ranks 2..4
        full = spec_attribution(h, basis, att, root, in_edges, q[1:2], g[1:2], 4)
        b[0][1], b[1][1], b[2][1] = full[0][0, 1:].float(), full[1][0, 1:].int(), full[2][0, 1:].int()

    broken(0, lambda b: b[0].__setitem__((1, 0), b[0][1, 0] + 1e-3))     # a value off
    broken(1, lambda b: b[1].__setitem__((1, 0), 4))                     # not an in-edge
    broken(2, lambda b: b[2].__setitem__((1, 0), 1))                     # the wrong relation
    if c[1, 0] != c[1, 1]:
        broken(3, swap)                                                  # out of order
    broken(4, drop_best)                                                 # a larger contribution is missing
    broken(5, lambda b: b[1].__setitem__((0, 1), -1))                    # padding inside the list (node 0 has 2 edges)
    broken(6, lambda b: b[3].__setitem__(1, b[3][1] + 1e-3))             # own off
    broken(7, lambda b: b[4].__setitem__(1, b[4][1] + 1e-3))             # total off
    broken(8, lambda b: b[3].__setitem__(6, 0.0))                        # a node out of range must give NaN
    single = next(j for j in range(k) if (int(s[1, j]), int(r[1, j])) != (0, 0))      # an edge of node 1 that is no duplicate

    def twice(b):
        other = (single + 1) % k
        b[0][1, other], b[1][1, other], b[2][1, other] = b[0][1, single], b[1][1, single], b[2][1, single]

    broken(9, twice)                                                     # one edge listed twice
