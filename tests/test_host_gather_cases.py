"""CPU checks of `tests/gather_cases.py`: the ladder graphs hold the edge cases the GPU tests rely on, the `exact` family
is exact, the fp64 reference agrees with the oracle, and the plan builder covers every row of an edgeless graph."""
import pytest
import torch

import gather_cases as C
from oracle import tip_oracle as O
from tip_amd.plan import ITEM_DIRECT, build_csr_plan, build_gather_plan, execute_csr_reference, execute_plan_reference, group_slots_for

ALL_WIDTHS = [(d, None) for d in C.VEC_WIDTHS] + C.SCALAR_WIDTHS


def test_helpers_agree_with_the_plan_builder():
    for d in C.VEC_WIDTHS + [d for d, v in C.SCALAR_WIDTHS if v is None]:
        assert C.group_slots(d) == group_slots_for(d), d
    assert C.group_slots(64, False) == 16 and C.lanes_for(64, False) == 64 and C.lanes_for(200) == 64 and C.lanes_for(12) == 4


@pytest.mark.parametrize('chunk', C.CHUNKS)
@pytest.mark.parametrize('d,vec', ALL_WIDTHS)
def test_ladder_holds_its_edge_cases(d, vec, chunk):
    L, G = C.lanes_for(d, vec), C.group_slots(d, vec)
    deg = C.degree_ladder(L, chunk, G)
    step = max(L, 8)
    for k in (0, 1, L, L + 1, 7, 8, 9, step, step + 1, 2 * step - 1, 2 * step + 1, chunk, chunk + 1, 8 * chunk, 8 * chunk + 1,
              G * chunk, G * chunk + 1):
        assert k in deg, k
    assert deg[0] == 0 and deg[-2:] == [0, 0] and deg.count(G * chunk) == 2 and sum(deg) < 10000 and len(deg) < 400
    out_row, table_row = C.ladder_graph(deg, 50, seed=d + chunk)
    assert torch.equal(torch.bincount(out_row, minlength=len(deg)), torch.tensor(deg))
    assert sorted(set(table_row.tolist())) == list(range(50))                # every table row is gathered
    hub = deg.index(max(deg))
    in_hub = table_row[out_row == hub]
    assert int((in_hub == 0).sum()) >= 2 and int((in_hub == 49).sum()) >= 2  # duplicates of both end rows inside the hub
    assert table_row[out_row == deg.index(1)].tolist() == [0]
    small = deg.index(min(k for k in deg if k >= 2))
    assert {0, 49} <= set(table_row[out_row == small].tolist())
    assert not torch.equal(out_row, torch.sort(out_row).values)              # caller order is shuffled
    for weighted in (False, True):
        w = torch.rand(out_row.numel()) if weighted else None
        C.check_ladder(build_gather_plan(out_row, table_row, len(deg), 50, w, chunk), deg)
        C.check_ladder(build_gather_plan(out_row, table_row, len(deg), 50, w, chunk, group_slots=G), deg, G)


@pytest.mark.parametrize('chunk', C.CHUNKS)
@pytest.mark.parametrize('d,vec', ALL_WIDTHS)
@pytest.mark.parametrize('weighted', [False, True])
def test_exact_family_is_exact(d, vec, chunk, weighted):
    c = C.Case(d, chunk, weighted, 'exact', vec=vec)
    c.assert_exact()
    # ... and the plans compute the reference (fp64 interpretation of the plan, any order: exact as well)
    for G in (0, c.G):
        got = execute_plan_reference(c.plan(G), c.table.double())
        assert torch.equal(got, c.ref(False))


@pytest.mark.parametrize('max_slots', [8, 9])
@pytest.mark.parametrize('d', [128, 256, 12, 3, 50])
def test_truncated_ladders_for_finalize(d, max_slots):
    chunk = 16
    c = C.Case(d, chunk, True, 'exact', max_degree=8 * chunk + (max_slots - 8))
    c.assert_exact()
    assert c.plan(0).max_slots == max_slots and c.deg[0] == 0 and c.deg[-1] == 0


@pytest.mark.parametrize('d,d2', C.LIN_SHAPES)
@pytest.mark.parametrize('weighted', [False, True])
def test_exact_family_of_the_linear_map(d, d2, weighted):
    c = C.lin_case(d, d2, weighted)
    assert max(c.deg) == c.chunk + 1
    for scale in (None, c.scale):
        agg = C.reference(c.table.double(), c.out_row, c.table_row, c.n_out, None if c.w is None else c.w.double(), scale)
        mag = C.magnitude(c.table.double(), c.out_row, c.table_row, c.n_out, None if c.w is None else c.w.double(), scale)
        C.assert_exact(agg, mag)
        for b2, relu in ((None, False), (c.bias2, True)):
            C.assert_exact(C.lin_reference(agg, c.weight, b2, relu), C.lin_magnitude(mag, c.weight, b2))
    plan = c.plan(c.G)
    assert plan.n_slots == 0 and bool((plan.items[:, 3] & 4).any())           # split rows: leaders finish rows for the map


def test_reference_agrees_with_the_oracle():
    for weighted in (False, True):
        for family in ('exact', 'normal'):
            c = C.Case(20, 16, weighted, family)
            w64 = None if c.w is None else c.w.double()
            want = O.gather_sum(c.table.double(), c.table_row, c.out_row, c.n_out, w64)
            got = c.ref(False)
            if family == 'exact':
                assert torch.equal(got, want)
            else:
                torch.testing.assert_close(got, want, rtol=0, atol=1e-12 * float(c.mag().max()))
            full = torch.relu(want * c.scale.double().unsqueeze(1) + c.bias.double())
            torch.testing.assert_close(c.ref(True), full, rtol=0, atol=1e-12 * float(c.mag(True).max()))
            # the fp32 restatement is the same formula
            assert float((c.cpu32(True).double() - c.ref(True)).abs().max()) <= 1e-5 * float(c.mag(True).max())


def test_gate_in_the_reference():
    c = C.Case(12, 16, False, 'exact')
    gate = torch.randn(c.n_out, 12, generator=torch.Generator().manual_seed(1))
    gate[0, :4] = torch.tensor([0.0, -0.0, -1.0, 1.0])
    ref = c.ref(True, gate=gate)
    assert torch.equal(ref, torch.where(gate > 0, c.ref(True), torch.zeros(c.n_out, 12, dtype=torch.float64)))
    assert ref[0, :3].abs().max() == 0


@pytest.mark.parametrize('G', [0, 16, 128])
def test_plan_of_an_edgeless_graph_has_one_empty_direct_item_per_row(G):
    e = torch.zeros(0, dtype=torch.long)
    for n_out in (1, 13):
        plan = build_gather_plan(e, e, n_out, 5, None, 16, group_slots=G)
        it = plan.items.long()
        assert it.shape == (n_out, 4) and plan.n_slots == 0 and plan.split_rows.shape[0] == 0 and plan.max_slots == 0
        assert bool((it[:, 0] == it[:, 1]).all()) and bool((it[:, 3] == ITEM_DIRECT).all())
        assert sorted(it[:, 2].tolist()) == list(range(n_out))
        assert plan.row_id.numel() == 0 and plan.group_slots == G
        assert torch.equal(execute_plan_reference(plan, torch.ones(5, 4)), torch.zeros(n_out, 4))


@pytest.mark.parametrize('d', C.CSR_WIDTHS)
def test_csr_cases(d):
    rp = C.csr_rows_per_task(d)
    assert rp == {8: 1, 12: 3, 32: 7, 64: 15, 128: 16, 200: 16, 256: 16}[d]
    ns = C.csr_n_outs(rp)
    assert {1, rp, rp + 1} <= set(ns) and (rp == 1 or any(n % rp for n in ns))
    deg = C.csr_degrees(rp, max(ns))
    assert {7, 8, 9, 17} <= set(deg)
    tasks = [deg[i:i + rp] for i in range(0, len(deg), rp)]
    if rp > 1:
        assert any(t[0] == 0 and sum(t) > 0 for t in tasks) and any(t[-1] == 0 and sum(t) > 0 for t in tasks)
    assert any(sum(t) == 0 and i > 0 and sum(tasks[i - 1]) > 0 and sum(tasks[i + 1]) > 0 for i, t in enumerate(tasks[:-1]))
    for n_out in ns:
        dg = C.csr_degrees(rp, n_out)
        out_row, table_row = C.ladder_graph(dg, 11, seed=d + n_out) if sum(dg) >= 15 else (
            torch.repeat_interleave(torch.arange(n_out), torch.tensor(dg)), torch.arange(sum(dg)) % 11)
        plan = build_csr_plan(out_row, table_row, n_out, 11)
        table = torch.randint(-8, 9, (11, d)).double()
        ref = C.reference(table, out_row, table_row, n_out)
        assert torch.equal(execute_csr_reference(plan, table), ref)
        C.assert_exact(ref, C.magnitude(table, out_row, table_row, n_out))


def test_edge_graph_has_its_deliberate_edges():
    ei, hub, iso = C.edge_graph(300)
    src, dst = ei
    assert not bool((ei == iso).any()) and int((dst == hub).sum()) >= 600
    assert int((src == src * 0 + dst).sum()) >= 10                             # self-loops
    pairs = (src * 300 + dst).tolist()
    assert len(pairs) - len(set(pairs)) >= 40                                  # duplicate edges
    assert C.edge_graph(1)[0].shape == (2, 2)


@pytest.mark.parametrize('n', [300, 1])
@pytest.mark.parametrize('kind', ['aggregate', 'gcn_conv', 'agg_first'])
def test_autograd_cases_keep_clear_of_the_relu_kink(kind, n):
    """No pre-activation within 1e-5 of its sum of |terms| of zero: fp32 rounding (1e-7 of that sum) cannot flip a ReLU mask,
    so the gradients of the GPU test are compared on one branch.  The reference reproduces the oracle's normalisation."""
    a = C.autograd_case(kind, n)
    out_row, table_row, w, n_out = a['edges']
    ref = C.conv_reference(kind, a['x'], None if kind == 'aggregate' else a['wt'].t(), a['bias'], a['up'], out_row, table_row, w, n_out)
    assert ref['margin'] > 1e-5, ref['margin']
    for name in ('out', 'd_x', 'd_bias'):
        r64, c32, mag = ref[name]
        assert r64.shape == c32.shape == mag.shape and bool((mag + 1e-12 >= r64.abs()).all())
        assert float((c32.double() - r64).abs().max()) <= 1e-5 * float(mag.max())
    ei = C.edge_graph(n)[0]
    ro, co, wo = O.gcn_norm(ei, n, torch.float64)
    dense = torch.zeros(n, n, dtype=torch.float64).index_put_((co, ro), wo, accumulate=True)
    mine = torch.zeros(n_out, n, dtype=torch.float64).index_put_((out_row, table_row), w.double(), accumulate=True)
    torch.testing.assert_close(mine, dense if a['rows'] is None else dense[a['rows']], rtol=0, atol=1e-6)
    if kind == 'agg_first' and n > 1:
        assert {0, n - 1, 3, 5} <= set(a['rows'].tolist())
