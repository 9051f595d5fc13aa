"""Not gpu: the host side of the drug fold-in (include/tipk.h section 4k) -- the three C symbols and their statuses without a
device, the refusals of the op and of `TIP.embed_new_drugs`, and the fp64 spec (tests/fold_in_spec.py) against the
reference-generated two-layer fixture, against the attribution spec's layer, and against the mistakes its rule must catch."""
import types

import pytest
import torch

import fold_in_cases as cases
from attribution_spec import rgcn_layer64
from conftest import load_golden
from fold_in_spec import U, check_fold_in, gamma, layer_row64, spec_fold_in, x0_row64
from oracle import tip_oracle as O
from tip_amd import _lib, ops
from tip_amd.layers import TIP, FMEncoder, NewDrugs

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _call(n_new=1, null=None, ne=48, p=16, pd=16, d1=32, d2=16, B=32, cat=1, n_tgt=3, n_edges=5, ld_x0=None):
    """tipk_drug_fold_in with fake non-NULL addresses (nothing is launched on the paths tested here)."""
    names = ('h_prot', 'hgcn_w', 'x0', 'h1', 'basis1', 'att1', 'root1', 'basis2', 'att2', 'root2', 'xd', 'tgt_ptr', 'tgt_prot',
             'in_ptr', 'in_src', 'in_rel', 'x0_new', 'h1_new', 'z_new')
    a = {name: 4096 for name in names}
    if null:
        a[null] = None
    d0 = ne + pd if cat else ne
    return _lib.lib().tipk_drug_fold_in(a['h_prot'], p, 40, p, a['hgcn_w'], pd, a['x0'], d0 if ld_x0 is None else ld_x0, a['h1'], d1,
                                        61, a['basis1'], a['att1'], B, a['root1'], a['basis2'], a['att2'], B, a['root2'], 7, B,
                                        d1, d2, a['xd'], ne, ne, cat, a['tgt_ptr'], a['tgt_prot'], n_tgt, a['in_ptr'],
                                        a['in_src'], a['in_rel'], n_edges, n_new, a['x0_new'], d0, a['h1_new'], d1, a['z_new'],
                                        d2, None, None)


def test_symbols_and_statuses_without_a_device():
    L = _lib.lib()
    for name in ('tipk_drug_fold_in', 'tipk_drug_fold_in_supported', 'tipk_drug_fold_in_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(L, name), name           # declared in the header, exported by the library
    assert L.tipk_abi_version() == 30 and _lib.ABI_VERSION == 30            # purely additive
    sup = L.tipk_drug_fold_in_supported                                     # (n_nodes, n_prot, n_rel, B, ne, p, pd, d1, d2, cat)
    for ne, pd, d1, d2, B, cat, p in cases.DIMS:
        assert sup(cases.N, cases.N_PROT, cases.R, B, ne, p, pd, d1, d2, int(cat)) == 1
        assert ops.drug_fold_in_supported(cases.N, cases.N_PROT, cases.R, B, ne, p, pd, d1, d2, cat)
    assert sup(645, 19081, 1097, 32, 48, 16, 16, 32, 16, 1) == 1            # tip.py, cat
    assert sup(645, 19081, 1097, 32, 64, 16, 64, 32, 16, 0) == 1            # tip.py, add
    assert sup(645, 500, 6, 64, 64, 64, 64, 64, 64, 1) == 1                 # every width at its limit: d0 = 128
    assert sup(645, 500, 6, 64, 65, 64, 64, 64, 64, 1) == 0                 # d0 = 129
    assert sup(645, 500, 6, 32, 128, 16, 1, 32, 16, 1) == 0                 # d0 = 129 again
    assert sup(645, 500, 6, 32, 127, 16, 1, 1, 1, 1) == 1 and sup(3, 1, 1, 1, 1, 1, 1, 1, 1, 0) == 1
    assert sup(645, 500, 6, 65, 48, 16, 16, 32, 16, 1) == 0 and sup(645, 500, 6, 32, 48, 65, 16, 32, 16, 1) == 0
    assert sup(645, 500, 6, 32, 48, 16, 65, 32, 16, 1) == 0 and sup(645, 500, 6, 32, 48, 16, 16, 65, 16, 1) == 0
    assert sup(645, 500, 6, 32, 48, 16, 16, 32, 65, 1) == 0 and sup(645, 500, 6, 32, 48, 16, 16, 32, 16, 0) == 0   # add: ne != pd
    assert sup(0, 500, 6, 32, 48, 16, 16, 32, 16, 1) == 0 and sup(645, 0, 6, 32, 48, 16, 16, 32, 16, 1) == 0
    ws = L.tipk_drug_fold_in_workspace_bytes
    assert ws(645, 500, 6, 32, 48, 16, 16, 32, 16, 1, 4096, 1 << 20) >= 0
    assert ws(645, 500, 6, 32, 48, 16, 16, 32, 16, 1, -1, 0) == -1 and ws(645, 500, 6, 65, 48, 16, 16, 32, 16, 1, 1, 0) == -1
    # statuses: EINVAL first, then EUNSUPPORTED -- "unsupported" in the library's words --, and M == 0 succeeds unlaunched
    assert _call(n_new=-1) == EINVAL and _call(n_edges=-1) == EINVAL and _call(n_tgt=-1) == EINVAL and _call(d1=0) == EINVAL
    assert _call(ld_x0=63) == EINVAL and _call(cat=0) == EINVAL             # a stride shorter than its row; add with ne != pd
    for name in ('h_prot', 'hgcn_w', 'x0', 'h1', 'basis1', 'att1', 'root1', 'basis2', 'att2', 'root2', 'xd', 'tgt_ptr', 'tgt_prot',
                 'in_ptr', 'in_src', 'in_rel', 'x0_new', 'h1_new', 'z_new'):
        assert _call(null=name) == EINVAL, name
    assert _call(null='tgt_prot', n_tgt=0, n_new=0) == OK and _call(null='in_src', n_edges=0, n_new=0) == OK
    assert _call(ne=120, pd=9) == EUNSUPPORTED and _call(B=65) == EUNSUPPORTED and _call(d2=65) == EUNSUPPORTED
    assert b'unsupported' in L.tipk_strerror(EUNSUPPORTED)
    assert _call(n_new=0) == OK and _call(n_new=0, ne=64, pd=64, p=64, d1=64, d2=64, B=64) == OK
    assert _call(n_new=0, ne=120, pd=9) == EUNSUPPORTED and _call(n_new=0, d1=0) == EINVAL


def test_op_refuses_host_tensors_and_wrong_shapes():
    c = cases.make_case(cases.DIMS[1])
    with pytest.raises(_lib.TipkError, match='device'):
        ops.drug_fold_in(*c)
    with pytest.raises(_lib.TipkError, match='fp32'):
        ops.drug_fold_in(*c._replace(x0=c.x0.double()))


def test_embed_new_drugs_refusals():
    assert NewDrugs._fields == ('x0', 'h', 'z', 'degree', 'n_targets')
    assert callable(FMEncoder.fold_in_tables)
    with pytest.raises(NotImplementedError, match='shard'):
        TIP.embed_new_drugs(types.SimpleNamespace(shard=object()), [[]])
    data = types.SimpleNamespace(n_prot=40, n_drug=61, n_dd_et=7)
    bare = types.SimpleNamespace(shard=None, data=data, encoder=None)
    for kw in (dict(targets=[[40]]), dict(targets=[[-1]]), dict(targets=[[]], interactions=[[(61, 0)]]),
               dict(targets=[[]], interactions=[[(0, 7)]]), dict(targets=[[1], []], interactions=[[], [(3, 2), (0, -1)]])):
        with pytest.raises(ValueError, match='out of range'):
            TIP.embed_new_drugs(bare, **kw)
    with pytest.raises(ValueError, match='one list per new drug'):
        TIP.embed_new_drugs(bare, [[1], [2]], interactions=[[]])


# ------------------------------------------------------------------ the spec
def _in_edges_of(ei, v):
    return torch.nonzero(ei[1] == v).reshape(-1)


def test_spec_reproduces_the_reference_generated_two_layer_fixture():
    """Every node of rgcn_fast_sym as if it were folded in: its layer rows from (x, its in-edges) and (relu(hidden), its in-edges).
    The fixture was recorded from the reference in fp32, so its own rounding (about 1e-6 of a row's magnitude) is what a direct
    comparison can show; the reference's arithmetic in fp64 on the fixture's inputs -- oracle/tip_oracle.py `rgcn_fwd`, itself
    pinned to the fixture by tests/test_oracle_golden.py -- is reproduced to 1e-12 relative."""
    g = load_golden('rgcn_fast_sym', torch.float64)
    ei, rg = g['dd_idx'], g['dd_range']
    n = g['x'].shape[0]
    rel = torch.bucketize(torch.arange(ei.shape[1]), rg[:, 1].contiguous(), right=True)
    l1 = tuple(g['l1.' + k] for k in ('basis', 'att', 'root'))
    l2 = tuple(g['l2.' + k] for k in ('basis', 'att', 'root'))
    hidden64 = O.rgcn_fwd(g['x'], ei, rg, *l1)[0]
    x1 = torch.relu(g['hidden'])                                         # the fixture's own hidden layer feeds layer 2
    out64 = O.rgcn_fwd(x1, ei, rg, *l2)[0]
    assert hidden64.dtype == torch.float64 and int((torch.bincount(ei[1], minlength=n) == 0).sum()) > 0   # isolated drugs too
    worst = [0.0, 0.0, 0.0, 0.0]
    for v in range(n):
        e = _in_edges_of(ei, v)
        row1 = layer_row64(g['x'], *l1, g['x'][v], ei[0][e], rel[e])[0]
        row2 = layer_row64(x1, *l2, x1[v], ei[0][e], rel[e])[0]
        for i, (have, want) in enumerate(((torch.relu(row1), torch.relu(hidden64[v])), (row2, out64[v]),
                                          (torch.relu(row1), x1[v]), (row2, g['out'][v]))):
            worst[i] = max(worst[i], float((have - want).abs().max() / want.abs().max().clamp(min=1e-30)))
    print('spec rows vs the reference arithmetic in fp64: relu(hidden) %.2e, out %.2e; vs the recorded fp32: %.2e, %.2e' % tuple(worst))
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12
    assert worst[2] <= 1e-5 and worst[3] <= 1e-5                         # (rtol of tests/test_oracle_golden.py for this fixture)


def test_spec_agrees_with_the_attribution_specs_layer():
    c = cases.make_case(cases.DIMS[1], seed=3)
    g = torch.Generator().manual_seed(9)
    n, n_edges = cases.N, 400
    ei = torch.randint(0, n, (2, n_edges), generator=g)
    ei[1][ei[1] == 7] = 8                                                # node 7 is isolated
    rel = torch.randint(0, cases.R, (n_edges,), generator=g)
    basis, att, root = (t.double() for t in c.layer2)
    z = rgcn_layer64(c.h1, basis, att, root, ei, rel)
    for v in range(n):
        e = _in_edges_of(ei, v)
        row = layer_row64(c.h1.double(), basis, att, root, c.h1[v].double(), ei[0][e], rel[e])[0]
        torch.testing.assert_close(row, z[v], rtol=1e-13, atol=1e-14)


def test_the_rule_passes_the_spec_and_bites():
    c = cases.make_case(cases.DIMS[1])
    x0, h1, z = spec_fold_in(*c)
    deg = (c.interactions[0][1:] - c.interactions[0][:-1]).tolist()
    tgt = (c.targets[0][1:] - c.targets[0][:-1]).tolist()
    assert deg[cases.HUB] == cases.HUB_EDGES and deg[cases.BARE] == 0 and tgt[cases.BARE] == 0 and deg[cases.ONE_EDGE] == 1
    assert len(set(zip(*(t[int(c.interactions[0][cases.HUB]):int(c.interactions[0][cases.HUB + 1])].tolist()
                         for t in c.interactions[1:])))) == cases.HUB_PAIRS
    assert int((c.interactions[2] == cases.UNUSED_REL).sum()) == 0 and int((c.interactions[2] == cases.R - 1).sum()) > 0
    assert {0, cases.N - 1} <= set(c.interactions[1].tolist()) and cases.UNTARGETED in c.targets[1].tolist()
    assert bool((c.xd[cases.BARE] == 0).all()) and bool((z[cases.BARE] == 0).all())     # nothing known: the zero embedding
    # the definition, spelled once more with plain loops, for one ordinary drug
    m = cases.ENDS
    a, b = int(c.interactions[0][m]), int(c.interactions[0][m + 1])
    ta, tb = int(c.targets[0][m]), int(c.targets[0][m + 1])
    mean = sum(c.h_prot[int(q)].double() for q in c.targets[1][ta:tb]) / (tb - ta)
    x0m = torch.cat([c.xd[m].double(), mean @ c.hgcn_w.double()])
    agg = sum(torch.einsum('b,i,bio->o', c.layer1[1][int(r)].double(), c.x0[int(s)].double(), c.layer1[0].double())
              for s, r in zip(c.interactions[1][a:b], c.interactions[2][a:b])) / (b - a)
    torch.testing.assert_close(x0[m], x0m, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(h1[m], torch.relu(agg + x0m @ c.layer1[2].double()), rtol=1e-13, atol=1e-14)
    # the spec's own result, rounded to fp32 once per stage, passes: one rounding is inside every bound
    good = (x0.float(), h1.float(), z.float())
    res = check_fold_in(*c, good, 'spec')
    assert max(res['used_x0'], res['used_h1'], res['used_z'], res['used_chain']) <= 1.0
    assert gamma(3) > 3 * U and res['tau_z'].shape == z.shape

    def broken(what, bad):
        with pytest.raises(AssertionError):
            check_fold_in(*c, bad, what)

    off = z.float().clone()                                              # one entry of z moved by 4 tau
    off[cases.EDGES_ONLY, 1] += float(4 * res['tau_z'][cases.EDGES_ONLY, 1])
    assert float(res['tau_z'][cases.EDGES_ONLY, 1]) > 0
    broken('z entry moved by 4 tau', (good[0], good[1], off))
    # a wrong denominator of the means: deg instead of max(deg, 1) (drugs without an edge divide by zero), and a plain sum
    with_zero_deg = tuple(t.float() for t in spec_fold_in(*c, denom=lambda k: k))
    assert not bool(torch.isfinite(with_zero_deg[2][cases.BARE]).all())
    broken('deg instead of max(deg, 1)', with_zero_deg)
    broken('a sum instead of a mean', tuple(t.float() for t in spec_fold_in(*c, denom=lambda k: 1)))
    # layer 1 run with att2's rows and layer 2 with att1's
    swapped = c._replace(layer1=(c.layer1[0], c.layer2[1], c.layer1[2]), layer2=(c.layer2[0], c.layer1[1], c.layer2[2]))
    broken('att1 / att2 swapped', tuple(t.float() for t in spec_fold_in(*swapped)))
    # and the single stages: each is held on its own
    broken('x0 off', (good[0] + 1e-3, good[1], good[2]))
    broken('h1 off', (good[0], good[1] - 1e-3, good[2]))
    row = x0_row64(c.xd[3].double(), c.h_prot.double(), c.hgcn_w.double(), c.targets[1][:0], True)[0]
    assert torch.equal(row[c.xd.shape[1]:], torch.zeros(c.hgcn_w.shape[1], dtype=torch.float64))      # no target: pd = 0
