"""-m gpu: `tipk_rgcn_attribution` (include/tipk.h section 4j), `MyRGCNConv2.attribute` and `TIP.explain` against the fp64
acceptance rule of tests/attribution_spec.py -- the reference-generated R-GCN fixtures (they pin the edge direction and the
mean), small random directed graphs with every kind of node (tests/attribution_cases.py), both table routes bit for bit,
and the decomposition logit = offset + own + neighbours on the small pickle and on the bundled BioSNAP model."""
import os

import pytest
import torch

import attribution_cases as cases
from attribution_spec import U, check_attribution
from conftest import GOLDEN, load_golden
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _report(what, res):
    print('%s: used of tau -- listed %.3f own %.3f total %.3f' % (what, res['used_edge'], res['used_own'], res['used_total']))


# ------------------------------------------------------------------ reference-generated fixtures: direction and mean
@pytest.mark.parametrize('name', ['rgcn_directed', 'rgcn_fast_directed', 'rgcn_fast_sym'])
def test_fixture_outputs_split_into_own_and_edges(name):
    g = load_golden(name)
    pre = 'l2.' if 'hidden' in g else ''
    h = torch.relu(g['hidden']) if pre else g['x']
    basis, att, root, out = g[pre + 'basis'], g[pre + 'att'], g[pre + 'root'], g['out']
    n, d_out, k = h.shape[0], out.shape[1], 8
    in_edges = ops.in_edges_by_node(g['dd_idx'].to(DEV), g['dd_range'], n)
    if name == 'rgcn_directed':                                          # a source / destination swap cannot pass here
        indeg = torch.bincount(g['dd_idx'][1], minlength=n)
        assert int((indeg != torch.bincount(g['dd_idx'][0], minlength=n)).sum()) == 32
        assert torch.equal((in_edges[0][1:] - in_edges[0][:-1]).cpu(), indeg)
    q = torch.arange(n).repeat_interleave(d_out)                         # unit probes e_j for every node and column
    probe = torch.eye(d_out).repeat(n, 1)
    got = ops.rgcn_edge_attribution(*_dev(h, basis, att, root), in_edges, q.to(DEV), probe.to(DEV), k)
    res = check_attribution(h, basis, att, root, in_edges, q, probe, k, got, name)
    _report(name, res)
    parts = (got[3].double() + got[4].double()).cpu()
    err = (parts - out.double().reshape(-1)).abs()
    bound = 2e-6 * float(out.abs().max()) + res['tau_sum'] + res['tau_own']
    print('%s: |own + total - out| max %.3e, least slack %.3e' % (name, float(err.max()), float((bound - err).min())))
    assert bool((err <= bound).all()), (name, float((err - bound).max()))


# ------------------------------------------------------------------ random directed graphs
@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_random_directed_graph(shape):
    n, R, B, d_in, d_out, k = shape
    seed = sum(shape)
    ei, et = cases.directed_graph(n, R, seed)
    h, basis, att, root = cases.operands(n, R, B, d_in, d_out, seed)
    q, probe = cases.queries(n, d_out, seed)
    in_edges = ops.in_edges_by_node(ei.to(DEV), et.to(DEV), n)
    deg = (in_edges[0][1:] - in_edges[0][:-1]).cpu()
    assert int(deg[cases.HUB]) > 2 * cases.SEL_CAP and int(deg[cases.ONE]) == 1 and int(deg[cases.ISOLATED]) == 0
    assert not bool((et == R - 1).any())                                 # the last relation has no edge (att still has its row)
    got = ops.rgcn_edge_attribution(*_dev(h, basis, att, root), in_edges, q.to(DEV), probe.to(DEV), k)
    res = check_attribution(h, basis, att, root, in_edges, q, probe, k, got, str(shape))
    _report(str(shape), res)
    c, s, r, own, total = (t.cpu() for t in got)
    # the zero probe (query 6, the hub): every contribution ties at 0 and the first k positions of the segment are listed
    e0 = int(in_edges[0][cases.HUB])
    m = min(k, int(deg[cases.HUB]))
    assert bool((c[6, :m] == 0).all()) and float(own[6]) == 0 and float(total[6]) == 0
    assert torch.equal(s[6, :m], in_edges[1][e0:e0 + m].cpu()) and torch.equal(r[6, :m], in_edges[2][e0:e0 + m].cpu())
    # one node under two probes: two different lists of the same segment
    assert not torch.equal(c[0], c[5])
    assert float(total[cases.ISOLATED]) == 0 and bool(own[8:].isnan().all()) and bool(total[8:].isnan().all())


# ------------------------------------------------------------------ routes and repeats
def test_routes_and_repeats_agree_bit_for_bit():
    n, R, B, d_in, d_out, k = 645, 11, 32, 32, 16, 100
    ei, et = cases.directed_graph(n, R, 99, hub_edges=3000)
    h, basis, att, root = _dev(*cases.operands(n, R, B, d_in, d_out, 99))
    gen = torch.Generator().manual_seed(5)
    q = torch.arange(48).to(DEV)                                         # the hub, every role, ordinary nodes
    probe = torch.randn(q.numel(), d_out, generator=gen).to(DEV)
    in_edges = ops.in_edges_by_node(ei.to(DEV), et.to(DEV), n)
    route = _lib.lib().tipk_rgcn_attribution_lds_route
    assert _lib.get_option('attribution_global') == 0 and route(n, B) == 1
    a = ops.rgcn_edge_attribution(h, basis, att, root, in_edges, q, probe, k)
    b = ops.rgcn_edge_attribution(h, basis, att, root, in_edges, q, probe, k)
    _lib.set_option('attribution_global', 1)
    try:
        assert route(n, B) == 0
        c = ops.rgcn_edge_attribution(h, basis, att, root, in_edges, q, probe, k)
    finally:
        _lib.set_option('attribution_global', 0)
    torch.cuda.synchronize()
    for x, y, z, what in zip(a, b, c, ('contrib', 'src', 'rel', 'own', 'total')):
        assert torch.equal(x, y), ('repeat', what)
        assert torch.equal(x, z), ('routes', what)
    assert int((a[1][0] >= 0).sum()) == k and not bool(a[4].isnan().any())


# ------------------------------------------------------------------ TIP.explain
def _layer_inputs(model):
    d = model.data
    with torch.no_grad():
        h, z = model.encoder.encode_layers(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, d.p_feat,
                                           d.pp_train_indices, d.dp_edge_index, d.dp_range_list)
    r2 = model.encoder.rgcn2
    return h, z, r2.basis.detach(), r2.att.detach(), r2.root.detach(), ops.in_edges_by_node(d.dd_train_idx, d.dd_train_range, d.n_drug)


def _logit_terms(model, z, idx, et):
    """sum of the magnitudes of the products the decoder's logit of (u, v, r) adds up, float64 [T] on the host: what its
    fp32 rounding scales with (the screen spec's sum_k |z_u z_v w_r|; for the NN decoder both halves, through both layers)."""
    dec, z64 = model.decoder, z.double()
    zu, zv = z64[idx[0]].abs(), z64[idx[1]].abs()
    if model.decoder_kind == 'distmult':
        return (zu * zv * dec.weight.detach().double()[et].abs()).sum(1).cpu()
    first = ((zu @ dec.w1_l1.detach().double().abs()) * dec.w1_l2.detach().double()[et].abs()).sum(1)
    return (first + ((zv @ dec.w2_l1.detach().double().abs()) * dec.w2_l2.detach().double()[et].abs()).sum(1)).cpu()


def _check_explanation(model, idx, et, k, side, ex, what):
    """The identity and the lists of an Explanation, with h, the parameters and the probes taken from the model."""
    h, z, basis, att, root, in_edges = _layer_inputs(model)
    node, probe, offset = model.decoder.probe(z, idx, et, side)
    assert torch.equal(ex.offset, offset) and torch.equal(ex.degree, in_edges[0][node + 1] - in_edges[0][node])
    got = (ex.contribution, ex.partner, ex.relation, ex.own, ex.neighbours)
    res = check_attribution(h, basis, att, root, in_edges, node, probe, k, got, what)
    _report(what, res)
    terms = [ex.offset.double().cpu(), ex.own.double().cpu(), ex.neighbours.double().cpu()]
    mag = sum(t.abs() for t in terms)
    err = (ex.logit.double().cpu() - sum(terms)).abs()
    bound = res['tau_sum'] + res['tau_own'] + U * mag + 1e-6 * (1.0 + _logit_terms(model, z, idx, et))
    print('%s: |logit - (offset + own + neighbours)| max %.3e, least slack %.3e' % (what, float(err.max()), float((bound - err).min())))
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    return node, probe, in_edges


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_explain_small(decoder):
    from tip_amd.layers import TIP, Explanation, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d, k = model.data, 16
    deg = torch.bincount(d.dd_train_idx[1], minlength=d.n_drug)
    assert int(deg.max()) == 359 and int((deg == 0).sum()) == 87
    # 300 held-out triples, plus triples that end (side 'v') and start (side 'u') at isolated drugs and at the hub
    gen = torch.Generator().manual_seed(1)
    pick = torch.randperm(d.dd_test_idx.shape[1], generator=gen)[:300].to(DEV)
    iso = torch.nonzero(deg == 0).reshape(-1)[:4]
    hub = deg.argmax().reshape(1)
    special = torch.cat([iso, hub])
    other = torch.full_like(special, 7)
    idx = torch.cat([d.dd_test_idx[:, pick], torch.stack([other, special]), torch.stack([special, other])], 1)
    et = torch.cat([d.dd_test_et[pick], torch.arange(2 * special.numel(), device=DEV) % d.n_dd_et])
    before = model.embeddings.clone()
    for side in ('v', 'u'):
        ex = model.explain((idx, et), k=k, side=side)
        assert isinstance(ex, Explanation) and ex.partner.dtype == torch.int64 and ex.relation.dtype == torch.int64
        node, probe, in_edges = _check_explanation(model, idx, et, k, side, ex, '%s side %s' % (decoder, side))
        assert torch.equal(node, idx[1] if side == 'v' else idx[0])
        # isolated drugs: all padding, neighbours == 0
        lonely = ex.degree == 0
        assert int(lonely.sum()) >= 4
        assert bool((ex.neighbours[lonely] == 0).all()) and bool((ex.partner[lonely] == -1).all())
        assert bool(torch.isneginf(ex.contribution[lonely]).all()) and bool((ex.relation[lonely] == -1).all())
        # straight after construction the logit is `pred`'s (the layer-level tolerance of tests/test_gpu_layers.py)
        # (NN decoder: the tables' logit, and the logit of the returned score where fp32 sigma is invertible to that
        # tolerance: at |logit| = 8 the rounding of 1 - sigma moves the logit by 2e-4, a quarter of rtol * 8)
        with torch.no_grad():
            if decoder == 'distmult':
                want = model.decoder(model.embeddings, idx, et, sigmoid=False)
            else:
                want = ops.pair_table_score(*model.decoder._tables(model.embeddings), idx, et, sigmoid=False)
                mild = want.abs() < 8
                back = torch.logit(model.decoder(model.embeddings, idx, et).double()).float()
                print('nn: %d of %d logits below 8 in magnitude' % (int(mild.sum()), mild.numel()))
                torch.testing.assert_close(ex.logit[mild], back[mild], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(ex.logit, want, rtol=1e-4, atol=1e-5)
        # 'lower' is 'raise' of the negated probe, negated back
        low = model.explain((idx, et), k=k, side=side, direction='lower')
        h, z, basis, att, root, _ = _layer_inputs(model)
        c, s, r, own, total = ops.rgcn_edge_attribution(h, basis, att, root, in_edges, node, -probe, k)
        assert torch.equal(low.contribution, -c) and torch.equal(low.partner, s.long()) and torch.equal(low.relation, r.long())
        assert torch.equal(low.own, -own) and torch.equal(low.neighbours, -total) and torch.equal(low.logit, ex.logit)
        assert torch.equal(low.own, ex.own) and bool(torch.isposinf(low.contribution[lonely]).all())
        full = ex.degree >= k
        assert bool((low.contribution[full][:, 0] <= ex.contribution[full][:, -1]).all())
    assert torch.equal(model.embeddings, before)                         # explain re-encodes; it does not overwrite
    held = model.explain(k=3)                                            # None = the held-out set
    assert held.logit.shape == (d.dd_test_idx.shape[1],) and held.contribution.shape == (d.dd_test_idx.shape[1], 3)


def test_tip_explain_bundled_biosnap():
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for _ in range(3):
        opt.zero_grad()
        model().backward()
        opt.step()
    with torch.no_grad():
        model()
    d, k = model.data, 10
    deg = torch.bincount(d.dd_train_idx[1], minlength=d.n_drug)
    hub = deg.argmax().reshape(1)
    assert int(deg.max()) > 2 * cases.SEL_CAP
    pick = torch.randperm(d.dd_test_idx.shape[1], generator=torch.Generator().manual_seed(2))[:64].to(DEV)
    idx = torch.cat([d.dd_test_idx[:, pick], torch.stack([torch.full_like(hub, 3), hub])], 1)
    et = torch.cat([d.dd_test_et[pick], torch.zeros(1, dtype=d.dd_test_et.dtype, device=DEV)])
    ex = model.explain((idx, et), k=k, side='v')
    _check_explanation(model, idx, et, k, 'v', ex, 'biosnap')
    assert int(ex.degree[-1]) == int(deg.max()) and bool((ex.partner[-1] >= 0).all())
