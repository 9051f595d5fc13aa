"""CPU checks of `tests/protein_cases.py`: the graphs hold the edge cases the GPU tests rely on, the fp64 restatement of the stage
reproduces the recorded results of the project this one was modelled on, correct fp32 arithmetic meets the tolerance, and no
ReLU-gated value is close enough to zero for fp32 rounding to flip its mask."""
import pytest
import torch

import protein_cases as P
from conftest import load_golden
from oracle import tip_oracle as O


@pytest.mark.parametrize('variant', P.VARIANTS)
@pytest.mark.parametrize('size', range(len(P.SIZES)))
def test_graphs_hold_their_edge_cases(size, variant):
    n_prot, n_drug, seed = P.SIZES[size]
    assert 300 <= n_prot <= 700 and 40 <= n_drug <= 130
    pp, pd, d_norm = P.protein_graph(n_prot, n_drug, seed, variant)
    P.check_protein_graph(pp, pd, d_norm, n_prot, n_drug, variant)
    again = P.protein_graph(n_prot, n_drug, seed, variant)
    assert all(torch.equal(a, b) for a, b in zip((pp, pd, d_norm), again))
    for v in P.isolated_proteins(n_prot):
        assert not bool((pp == v).any())


def test_every_case_of_the_route_table_uses_a_checked_graph():
    for cid, row in P.ROUTE_CASES.items():
        assert 0 <= row[0] < len(P.SIZES) and row[1] in P.VARIANTS and row[1] != 'no_pd_edges_to_targets', cid


def test_check_protein_graph_notices_a_lost_edge_case():
    n_prot, n_drug, seed = P.SIZES[0]
    pp, pd, d_norm = P.protein_graph(n_prot, n_drug, seed, 'pruned')
    with pytest.raises(AssertionError):
        P.check_protein_graph(pp[:, pp[0] != pp[1]], pd, d_norm, n_prot, n_drug, 'pruned')           # no self-loops
    with pytest.raises(AssertionError):
        P.check_protein_graph(pp, pd[:, pd[1] >= n_prot], d_norm, n_prot, n_drug, 'pruned')           # no edge to a protein row
    with pytest.raises(AssertionError):
        P.check_protein_graph(pp, pd[:, pd[0] != P.BIG_SRC], d_norm, n_prot, n_drug, 'pruned')        # no source beyond max_edges
    with pytest.raises(AssertionError):
        P.check_protein_graph(pp[:, pp[1] != P.HUB], pd, d_norm, n_prot, n_drug, 'pruned')            # no hub


def _close(got, want, what):
    want = want.double()
    tol = 2e-5 * float(want.abs().max()) + 1e-12                              # the goldens are fp32 results of the original
    assert float((got.double() - want).abs().max()) <= tol, what


@pytest.mark.parametrize('name', ['pp_encoder', 'pp_encoder_dense'])
def test_reference_reproduces_the_recorded_pp_encoder(name):
    g = load_golden(name)
    n = int(g['n_prot']) if 'n_prot' in g else g['x'].shape[0]
    p = {'conv1.weight': g['conv1.lin.weight'], 'conv1.bias': g['conv1.bias'], 'conv2.weight': g['conv2.lin.weight'], 'conv2.bias': g['conv2.bias']}
    p = {k: v.double().requires_grad_() for k, v in p.items()}
    x = g['x'].double().requires_grad_() if 'x' in g else None
    h2, _ = P.pp_forward(p, g['pp_idx'], n, x)
    h2.backward(g['upstream'].double())
    _close(h2.detach(), g['out'], 'out')
    for k in p:
        _close(p[k].grad, g['grad.' + k.replace('.weight', '.lin.weight')], k)
    if x is not None:
        _close(x.grad, g['grad_x'], 'grad_x')


def test_reference_reproduces_the_recorded_hierarchy_conv():
    g = load_golden('hier_conv')
    ref = P.hier_layer_reference(g['dp_idx'], g['x'].shape[0], int(g['n_source']), g['x'], g['weight'], g['upstream'])
    _close(ref['out'], g['out'], 'out')
    _close(ref['g_x'], g['grad_x'], 'grad_x')
    _close(ref['g_w'], g['grad.weight'], 'grad.weight')


@pytest.mark.parametrize('name', ['encoder_cat_small', 'encoder_add_small'])
def test_reference_reproduces_the_stage_of_the_recorded_encoder(name):
    """x0 of `stage_forward` through the oracle's two R-GCN layers is the recorded z, and the gradients that flow back through x0
    into the stage's parameters are the recorded ones."""
    g = load_golden(name)
    n_prot, n_drug, mod = int(g['n_prot']), int(g['n_drug']), str(g['mod'])
    p = {'embed': g['embed'], 'hgcn.weight': g['hgcn.weight']}
    for c in ('conv1', 'conv2'):
        p[c + '.weight'], p[c + '.bias'] = g['pp_encoder.%s.lin.weight' % c], g['pp_encoder.%s.bias' % c]
    p = {k: v.double().requires_grad_() for k, v in p.items()}
    x0, _ = P.stage_forward(p, (g['pp_idx'], g['dp_idx'], g['d_norm']), n_prot, n_drug, None, mod)
    r = {k: g[k].double() for k in ('rgcn1.basis', 'rgcn1.att', 'rgcn1.root', 'rgcn2.basis', 'rgcn2.att', 'rgcn2.root')}
    a1, _ = O.rgcn_fwd(x0, g['dd_idx'], g['dd_range'], r['rgcn1.basis'], r['rgcn1.att'], r['rgcn1.root'])
    z, _ = O.rgcn_fwd(torch.relu(a1), g['dd_idx'], g['dd_range'], r['rgcn2.basis'], r['rgcn2.att'], r['rgcn2.root'])
    z.backward(g['upstream'].double())
    _close(z.detach(), g['z'], 'z')
    names = {'embed': 'embed', 'hgcn.weight': 'hgcn.weight', 'conv1.weight': 'pp_encoder.conv1.lin.weight', 'conv1.bias': 'pp_encoder.conv1.bias',
             'conv2.weight': 'pp_encoder.conv2.lin.weight', 'conv2.bias': 'pp_encoder.conv2.bias'}
    assert set(names) == set(P.GRAD_NAMES)
    for k, full in names.items():
        _close(p[k].grad, g['grad.' + full], k)


@pytest.mark.parametrize('cid', list(P.ROUTE_CASES))
def test_fp32_meets_the_tolerance_and_no_relu_mask_can_flip(cid):
    c = P.route_case(cid)
    ref, mag, c32 = c.ref(), c.mag(), c.cpu32()
    (pp_in, pp_out), (pd_in, pd_out) = P.degrees(c.graphs[0], c.graphs[1], c.n_prot, c.n_drug)
    assert c.k['pre1'] == pp_in + c.in_terms + 1 + P.W_ROUNDINGS == P.k_pre1(c.graphs[0], c.n_prot, c.in_terms)
    assert c.k['grad.embed'] == 2 and float(torch.as_tensor(c.k['x0']).min()) == (2 if c.mod == 'cat' else float(c.k['x0']))
    assert float(torch.as_tensor(c.k['x0']).max()) < 2 * (max(pp_in, pd_in) + c.in_terms + c.hid1 + c.hid2 + c.pd_dim)
    names = ['x0', 'pre1'] + ['grad.' + k for k in P.GRAD_NAMES] + (['grad.x_prot'] if c.feat != 'identity' else [])
    assert set(names) == set(ref) == set(mag) == set(c32)
    for name in names:
        assert bool((mag[name] * (1 + 1e-12) + 1e-300 >= ref[name].abs()).all()), name           # A bounds the value itself
        assert P.worst_ratio(c32[name], ref[name], mag[name], c.k_of(name)) <= 1, name
    # no conv1 pre-activation (= no ReLU-gated value) within MARGIN x its tolerance of zero: nothing is excluded from a comparison
    assert c.relu_margin() > P.MARGIN
    assert bool(torch.equal(c32['pre1'] > 0, ref['pre1'] > 0))
    on = (ref['pre1'] > 0).double().mean(0)
    assert bool(((on > 0) & (on < 1)).any()), 'the mask does not vary within a channel'
    # the reference is shared between tests and stays as it is
    assert c.ref() is ref


def test_one_layer_references_agree_with_the_stage():
    c = P.route_case('A_cat_dense')
    pp = c.graphs[0]
    p = c.params
    up = torch.randn(c.n_prot, c.hid1, generator=torch.Generator().manual_seed(1))
    one = P.gcn_layer_reference(pp, c.n_prot, c.x, p['conv1.weight'], p['conv1.bias'], True, up)
    assert torch.equal(one['pre'], c.ref()['pre1'])
    mag = P.gcn_layer_reference(pp, c.n_prot, c.x, p['conv1.weight'], p['conv1.bias'], True, up, absolute=True, mask=(one['pre'] > 0).double())
    for k in ('out', 'g_x', 'g_w', 'g_b'):
        assert bool((mag[k] * (1 + 1e-12) >= one[k].abs()).all()), k
