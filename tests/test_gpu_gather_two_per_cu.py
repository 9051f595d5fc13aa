"""-m gpu: the grouped gather kernel at two 1024-thread workgroups per CU (`tip_amd/csrc/tipk_gather_sum.hip`).

To fit 64 VGPRs the kernel picks edge ids with ds_swizzle, addresses a gathered row as table base + ONE 32-bit byte offset with
the lane's column offset folded in, and fetches the weights behind the row loads; the rider's 4-lane vector slab sum reads its
slabs from a scalar base + one offset register.  This file asserts the residency (`tipk_gather_sum_occupancy`) and runs the
paths that arithmetic can break, on ONE graph: rows of 0, 1, 7, 8, 9, 16 and 17 edges, a hub of more than 128 x 16 edges
(128 pieces, one workgroup), about 270 output rows over a table of 300 rows (several workgroups).

Values are the `exact` family of `tests/gather_cases.py`: every partial sum is exact in fp32, so every result must equal the
fp64 reference BIT FOR BIT (the bound of tests/test_gpu_gather_paths.py sections A-H), a second launch must repeat it, and the
grouped route must equal the ungrouped (partial + finalize) one.
"""
import functools

import pytest
import torch

import gather_cases as C

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N_TABLE = 300
CHUNK = 16
HUB = 128 * CHUNK + 5
DEGREES = [0, 1, 7, 8, 9, 16, 17, HUB] + [(0, 1, 7, 8, 9, 16, 17, 33)[i % 8] for i in range(260)] + [0]


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def assert_bits(got, ref64, what=''):
    want = ref64.to(torch.float32)
    assert torch.equal(want.double(), ref64), 'reference not representable in fp32'
    g = got.detach().cpu().reshape(want.shape)
    same = bits(g) == bits(want)
    if not bool(same.all()):
        bad = tuple(torch.nonzero(~same)[0].tolist())
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r, want %r'
                             % (what, int((~same).sum()), same.numel(), bad, float(g[bad]), float(want[bad])))


class Graph(object):
    """The graph above with exact values for width d (CPU)."""

    def __init__(self, d, weighted, t_max=8):
        from tip_amd.plan import group_slots_for
        self.d, self.weighted = d, weighted
        self.n_out = len(DEGREES)
        self.out_row, self.table_row = C.ladder_graph(DEGREES, N_TABLE, seed=d * 7 + int(weighted))
        self.E = int(self.out_row.numel())
        self.table, self.w, self.scale, self.bias = C.exact_values(N_TABLE, d, self.E, self.n_out, d + 50 * int(weighted), weighted, t_max=t_max)
        self.G = group_slots_for(d)

    def plan(self, grouped=True):
        from tip_amd.plan import build_gather_plan
        return build_gather_plan(self.out_row, self.table_row, self.n_out, N_TABLE, self.w, CHUNK, 'two_per_cu',
                                 group_slots=self.G if grouped else 0).to(DEV)

    def w64(self):
        return None if self.w is None else self.w.double()

    def ref(self, epilogue, gate=None):
        epi = (self.scale, self.bias) if epilogue else (None, None)
        args = (self.table.double(), self.out_row, self.table_row, self.n_out, self.w64()) + epi
        ungated = C.reference(*args, relu=epilogue)
        C.assert_exact(ungated, C.magnitude(*args))
        return ungated if gate is None else C.reference(*args, relu=epilogue, gate=gate)


@functools.lru_cache(maxsize=None)
def graph(d, weighted, t_max=8):
    return Graph(d, weighted, t_max)


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops as o
    return o


def test_the_plan_holds_the_cases():
    """128 pieces of the hub in one workgroup, pieces longer than the chunk, rows of every length, several workgroups."""
    from tip_amd.plan import ITEM_LEADER, ITEM_PIECE
    g = graph(32, True)
    plan = g.plan()
    it = plan.items.cpu().long()
    fl = it[:, 3]
    assert plan.group_slots == g.G == 128 and plan.n_slots == 0
    lead = fl[(fl & ITEM_LEADER) != 0] >> 8
    assert int(lead.max()) == 128 and int(lead.min()) == 2
    piece_len = (it[:, 1] - it[:, 0])[(fl & ITEM_PIECE) != 0]
    assert int(piece_len.max()) == -(-HUB // 128) == 17
    assert it.shape[0] > 3 * 128
    assert {0, 1, 7, 8, 9, 16}.issubset(set((it[:, 1] - it[:, 0]).tolist()))


# ------------------------------------------------------------------------------------------------ residency
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('d', [16, 32])
def test_two_workgroups_of_the_grouped_gather_per_cu(ops, d, weighted):
    """`tipk_gather_sum_occupancy` (hipOccupancyMaxActiveBlocksPerMultiprocessor of the instance, with the launch's block
    size and dynamic LDS): at least 2 for the plain kernel, the fused linear map with 2 outputs per lane (LIN = 2) and the
    gate + column-sum kernel (LIN = -1; 1024-thread workgroups only)."""
    from tip_amd.plan import group_slots_for
    G = group_slots_for(d)
    L = d // 4
    assert ops.gather_sum_occupancy(d, G, weighted, 0) >= 2
    assert ops.gather_sum_occupancy(d, G, weighted, 2 * L) >= 2
    assert ops.gather_sum_lin_supported(d, 2 * L, G)
    if G * L == 1024:
        assert ops.gather_sum_occupancy(d, G, weighted, -1) >= 2
    else:
        with pytest.raises(Exception):
            ops.gather_sum_occupancy(d, G, weighted, -1)


def test_two_workgroups_of_the_hand_over_kernel_per_cu(ops):
    for d_out in (16, 32, 24):
        assert ops.sum_slabs_xb_occupancy(d_out) >= 2


def test_occupancy_query_refuses_what_no_launch_takes(ops):
    from tip_amd._lib import TipkError
    for args in ((30, 128, 0, 0), (32, 0, 0, 0), (128, 128, 0, 0), (32, 128, 0, 4), (20, 128, 0, 8)):
        with pytest.raises(TipkError):
            ops.gather_sum_occupancy(*args)
    with pytest.raises(TipkError):
        ops.sum_slabs_xb_occupancy(33)


# ------------------------------------------------------------------------------------------------ the gather paths
def run(ops, g, plan, table, epilogue, out=None):
    kw = dict(row_scale=g.scale.to(DEV), bias=g.bias.to(DEV), relu=True) if epilogue else {}
    if out is None:
        out = torch.full((g.n_out, g.d), float('nan'), device=DEV)
    ops.gather_sum(plan, table, out=out, **kw)
    return out


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('d', [32, 24, 16])
def test_grouped_gather_exact_repeatable_and_equal_to_ungrouped(ops, d, weighted):
    """d = 24: two of a slot's eight lanes lie beyond the width and load nothing.  Plain and with row_scale / bias / relu."""
    g = graph(d, weighted)
    table = g.table.to(DEV)
    grouped, ungrouped = g.plan(True), g.plan(False)
    assert ungrouped.n_slots > 0
    for epilogue in (False, True):
        what = 'd=%d weighted=%s epilogue=%s' % (d, weighted, epilogue)
        out = run(ops, g, grouped, table, epilogue)
        assert_bits(out, g.ref(epilogue), what)
        assert torch.equal(bits(out), bits(run(ops, g, grouped, table, epilogue))), what + ': second launch'
        assert torch.equal(bits(out), bits(run(ops, g, ungrouped, table, epilogue))), what + ': ungrouped route'


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('d', [32, 16])
def test_table_and_out_with_a_row_stride_larger_than_the_width(ops, d, weighted):
    """The `cat` layout: the table is a column block of a wider buffer (its other columns NaN), so the row stride that
    multiplies the id is not the width whose column offset is folded into the same 32-bit byte offset; out likewise."""
    g = graph(d, weighted)
    wide_t = torch.full((N_TABLE, d + 48), float('nan'), device=DEV)
    wide_t[:, 16:16 + d] = g.table.to(DEV)
    for epilogue in (False, True):
        wide_o = torch.full((g.n_out, d + 32), -123.4375, device=DEV)
        run(ops, g, g.plan(), wide_t[:, 16:16 + d], epilogue, out=wide_o[:, 16:16 + d])
        assert_bits(wide_o[:, 16:16 + d], g.ref(epilogue), 'd=%d weighted=%s epilogue=%s' % (d, weighted, epilogue))
        side = torch.full((g.n_out, 16), -123.4375)
        assert torch.equal(bits(wide_o[:, :16]), bits(side)) and torch.equal(bits(wide_o[:, 16 + d:]), bits(side))


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('d', [32, 16])
def test_linear_map_with_two_outputs_per_lane(ops, d, weighted):
    """tipk_gather_sum_lin with d2 = d / 2 (LIN = 2): agg and out2 bit-equal to fp64, with and without bias2 / relu."""
    g = graph(d, weighted, 2)
    d2 = d // 2
    gen = torch.Generator().manual_seed(d)
    weight = torch.randint(-4, 5, (d2, d), generator=gen).float()
    bias2 = torch.randint(-3, 4, (d2,), generator=gen).float()
    agg64, mag = g.ref(False), C.magnitude(g.table.double(), g.out_row, g.table_row, g.n_out, g.w64())
    plan, table = g.plan(), g.table.to(DEV)
    for b2, relu in ((None, False), (bias2, True)):
        want2 = C.lin_reference(agg64, weight, b2, relu)
        C.assert_exact(C.lin_reference(agg64, weight, b2), C.lin_magnitude(mag, weight, b2))
        seen = []
        for rep in range(2):
            agg, out2 = ops.gather_sum_lin(plan, table, weight.to(DEV), None if b2 is None else b2.to(DEV), relu)
            assert_bits(agg, agg64, 'agg d=%d weighted=%s' % (d, weighted))
            assert_bits(out2, want2, 'out2 d=%d weighted=%s bias=%s' % (d, weighted, b2 is not None))
            seen.append(bits(out2))
        assert torch.equal(seen[0], seen[1])


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('d', [32, 24])
def test_gate_column_sums_and_rider_slab_sums(ops, d, weighted):
    """tipk_gather_sum_riders (LIN = -1) with riders on each layout of the slab body: the 16-lane vector layout, the 4-lane
    vector layout (11 slabs: one batch of eight and three more; 4 224 elements: the second workgroup is partial) with
    row_scale / addend / relu, and the dword layout.  out and the column sums against fp64, the riders bit-equal to `sum_slabs`."""
    g = graph(d, weighted)
    plan, table = g.plan(), g.table.to(DEV)
    assert ops.gather_sum_epilogue_supported(plan, d)
    gen = torch.Generator().manual_seed(d + 1)
    gate = torch.randn(g.n_out, d, generator=gen)
    gate[DEGREES.index(HUB), 0::3] = -0.0
    gate[0, 1::2] = -1.5
    ref = g.ref(True, gate=gate)
    C.assert_exact(ref.sum(0, keepdim=True), C.magnitude(g.table.double(), g.out_row, g.table_row, g.n_out, g.w64(), g.scale, g.bias).sum(0, keepdim=True))
    slabs = [torch.randn(40, 3, 32, generator=gen).to(DEV), torch.randn(11, 33, 128, generator=gen).to(DEV), torch.randn(9, 5, 16, generator=gen).to(DEV)]
    rs = (torch.rand(33, generator=gen) + 0.5).to(DEV)
    ad = torch.randn(33, 128, generator=gen).to(DEV)
    extra = [dict(), dict(row_scale=rs, addend=ad, relu=True), dict()]
    alone = [ops.sum_slabs(s, alpha=0.5, **kw) for s, kw in zip(slabs, extra)]
    seen = []
    for rep in range(2):
        jobs = [ops.slab_job(s, alpha=0.5, **kw) for s, kw in zip(slabs, extra)]
        out = torch.full((g.n_out, d), float('nan'), device=DEV)
        res, parts = ops.gather_sum(plan, table, row_scale=g.scale.to(DEV), bias=g.bias.to(DEV), relu=True, out=out, riders=jobs,
                                    gate=gate.to(DEV), colsum=True)
        assert res is out
        assert_bits(out, ref, 'gated d=%d weighted=%s' % (d, weighted))
        assert parts.shape == (-(-plan.items.shape[0] // plan.group_slots), 1, d)
        assert_bits(parts.double().cpu().sum((0, 1)).float(), ref.sum(0), 'column sums d=%d' % d)
        for j, a in zip(jobs, alone):
            assert torch.equal(bits(j.out), bits(a))
        seen.append((bits(out), bits(parts)))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
