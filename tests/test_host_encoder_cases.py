"""tests/encoder_cases.py on the CPU (libtipk built, for its host queries; no device): every case's graphs hold the edge cases
their generators promise, both ReLUs are clear of their kink with nothing excluded, the bound k 2^-24 A holds for the fp32 CPU
oracle on z and all twelve gradients, every probe (one dropped, doubled or misfiled edge) moves some compared element by at least
10 bounds in fp64, and the table covers what tests/test_gpu_encoder_step_edges.py relies on.  Every figure is printed (`-s`);
profiles/encoder_step_errors.md records them."""
import pytest
import torch

import encoder_cases as E
import protein_cases as P
from oracle import tip_oracle as O

PROBED = list(E.FUSED_IDS) + ['tiny_9']


@pytest.mark.parametrize('cid', E.CASE_IDS)
def test_graphs_hold_their_edge_cases(cid):
    c = E.case(cid)
    E.check_graphs(c)
    assert c.data['dd_train_range'].shape == (c.R, 2) and int(c.data['dd_train_range'][-1, 1]) == c.data['dd_train_idx'].shape[1]
    assert int(c.data['dd_train_idx'].max()) < c.n_drug


@pytest.mark.parametrize('cid', E.CASE_IDS)
def test_both_relus_are_clear_of_the_kink(cid):
    """(b): |pre-activation| > MARGIN x its own bound elementwise, for conv1 (`protein_cases.make_params`) and for a1 (constructed);
    a1's mask takes both values in every column and in at least a quarter of the rows; the dominant term is at most DOMINANT
    x the RMS of the rest; the fp32 CPU run has the same two masks as fp64."""
    c = E.case(cid)
    for name in ('pre1', 'a1'):
        m = c.relu_margin(name)
        print('MARGIN %s %s %.0f' % (cid, name, m))
        assert m > P.MARGIN, (cid, name, m)
    ref, c32 = c.ref(), c.cpu32()
    mask = ref['a1'] > 0
    assert bool(mask.any(0).all()) and bool((~mask).any(0).all()), 'a column of the mask is constant'
    assert float((mask.any(1) & (~mask).any(1)).float().mean()) >= 0.25
    assert c.dominance() <= E.DOMINANT * (1 + 1e-6), c.dominance()
    assert torch.equal(c32['a1'] > 0, mask) and torch.equal(c32['h1'] > 0, ref['h1'] > 0)
    h1 = ref['h1'] > 0
    assert bool(h1.any()) and bool((~h1).any())


@pytest.mark.parametrize('cid', E.CASE_IDS)
def test_fp32_cpu_oracle_is_within_the_bound(cid):
    """(c): correct fp32 arithmetic, in the oracle's own order of operations, stays within k 2^-24 A on z and all twelve
    gradients; the composition A is computed from is the oracle's encoder (to 1e-12 of max |want|)."""
    c = E.case(cid)
    ref, c32 = c.ref(), c.cpu32()
    q = {k: v.double() for k, v in c.params.items()}
    z, a1, _ = E.composed(q, c.data, c.mod)
    for got, want in ((z, ref['z']), (a1, ref['a1'])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert set(E.TENSORS) <= set(c.k) and all(c.k[n] > 0 for n in E.TENSORS)
    for name in E.TENSORS:
        assert ref[name].shape == c.mag()[name].shape
        assert bool((ref[name].abs() <= c.mag()[name] * (1 + 1e-12) + 1e-300).all()), name          # A bounds |want| itself
        r = c.ratio(name, c32[name])
        print('CPU32 %s %s %.4f (k = %d)' % (cid, name, r, c.k[name]))
        assert r <= 1, (cid, name, r)


@pytest.mark.parametrize('cid', PROBED)
def test_probes_move_some_element_by_ten_bounds(cid):
    """(d): the evidence that the GPU comparison would fail on a dropped, doubled or misfiled edge."""
    c = E.case(cid)
    kinds = []
    for kind, data, moves in E.probes(c):
        effect, where = E.probe_effect(c, data)
        print('PROBE %s %s %.1f %s' % (cid, kind, effect, where))
        kinds.append(kind)
        if moves:
            assert effect >= E.PROBE_FACTOR, (cid, kind, effect, where)
        else:
            assert effect == 0, (cid, kind, effect, where)              # GCNConv replaces self-loops: nothing may move
    want = {'dir': ('dup_triple', 'hub_in_edge'), 'one_edge': ('rel1_edge', 'move_edge')}.get(c.kind, ('dup_triple', 'hub_in_edge'))
    if c.R >= 4:
        want += ('rel1_edge', 'move_edge')
    assert set(want) | {'pd_single', 'pp_self_loop', 'pp_edge'} <= set(kinds), (cid, kinds)


def test_case_table_covers():
    rows = [E.row(cid) for cid in E.CASE_IDS]
    by = {r['id']: r for r in rows}
    fused = [r for r in rows if r['expect'] == 'fused']
    assert {r['id'] for r in fused} == set(E.FUSED_IDS) and {r['id'] for r in rows if r['expect'] == 'refused'} == set(E.REFUSED_IDS)
    assert {r['kind'] for r in rows} == set(E.DD_KINDS) and {r['variant'] for r in rows} == set(E.PROT_VARIANTS)
    assert by['tiny_9']['expect'] == 'any' and (by['tiny_9']['n_drug'], by['tiny_9']['n_prot']) == (9, 12)
    # the fused rows: every D-D kind, both mods, both widths, and the sizes the issue names
    assert {r['kind'] for r in fused} == {'dir', 'sym', 'near', 'dense', 'one_edge'}
    assert {r['mod'] for r in fused} == {'cat', 'add'} and {r['n_hid2'] for r in fused} == {16, 32}
    assert {(r['mod'], r['n_hid2']) for r in fused} >= {('cat', 16), ('cat', 32), ('add', 16), ('add', 32)}
    assert (by['cat_sym_41']['n_drug'], by['cat_sym_41']['kind']) == (41, 'sym')
    assert (by['add_dir_130_h32']['n_drug'], by['add_dir_130_h32']['kind'], by['add_dir_130_h32']['mod'], by['add_dir_130_h32']['n_hid2']) == (130, 'dir', 'add', 32)
    assert (by['cat_near_41_h32']['n_drug'], by['cat_near_41_h32']['kind'], by['cat_near_41_h32']['n_hid2']) == (41, 'near', 32)
    assert by['r1']['R'] == 1
    assert (by['n1024']['n_drug'], by['n1024']['R'], by['n1024']['kind']) == (1024, 20, 'near')
    assert by['n64']['n_drug'] % 64 == 0 and by['dense_41']['n_drug'] == 41
    assert any(r['n_drug'] % 16 for r in fused) and any(r['n_drug'] > 64 and r['n_drug'] % 64 for r in fused)     # no multiple of a tile, several blocks
    # boundaries come from the library's predicates
    r1 = by['split1_last']['R']
    assert E.split_of(r1) == 1 and E.split_of(r1 + 1) != 1 and by['split2_first']['R'] == r1 + 1
    assert by['n1025']['n_drug'] == by['n1024']['n_drug'] + 1
    for key in ('R', 'kind', 'mod', 'n_hid2', 'variant', 'n_prot', 'seed'):                  # the refused twin differs in ONE thing
        assert by['n1025'][key] == by['n1024'][key] and (key == 'R' or by['split2_first'][key] == by['split1_last'][key])
    assert {by[v]['variant'] for v in ('all_sources', 'drug_source', 'no_pd_edges_to_targets')} == set(P.VARIANTS) - {'pruned'}
    assert all(r['variant'] == 'pruned' for r in fused)
    # every probe kind is exercised by some fused case, every fused case by at least four of them
    seen = set()
    for cid in E.FUSED_IDS:
        kinds = {k for k, _, _ in E.probes(E.case(cid))}
        assert len(kinds) >= 4, (cid, kinds)
        seen |= kinds
    assert seen >= set(E.PROBE_KINDS)


def test_dd_statistics_of_the_edge_cases():
    """What the edge cases are FOR, in numbers: the dense case fills every pair cell of its live drugs and stacks every used
    relation on the hub's; the one-edge case leaves all but one drug at in-degree 0; n1024 is at the library's own limit."""
    c = E.case('dense_41')
    st = E.dd_stats(c.data['dd_train_idx'], c.data['dd_train_range'], c.n_drug)
    live = c.n_drug - max(1, c.n_drug // 12)
    assert st['din'] >= live - 1 and st['dout'] >= live - 1 and st['cell'] >= c.R - 3          # (+ 1: a self-loop)
    c = E.case('one_edge')
    deg = O.in_degree(c.data['dd_train_idx'][1], c.n_drug, torch.float64)
    assert int((deg == 1).sum()) == c.n_drug and int(torch.bincount(c.data['dd_train_idx'][1], minlength=c.n_drug).max()) == 1
    assert E.dd_stats(E.case('n1024').data['dd_train_idx'], E.case('n1024').data['dd_train_range'], 1024)['din'] >= 32
