"""-m gpu: the large write-once outputs of the pair form, row by row.  The pair cells of `tipk_stream_gather` kind 1 /
`tipk_stream_gather_two` and the d att slabs of `tipk_stream_gather_parts_two` leave through 16-byte streaming stores
(tipk_common.h `st4_stream`); the pair-gradient rows of `tipk_rgcn_pair_grads` are plain stores (profiles/store_drain.md:
streaming them was measured and lost) and are pinned here all the same, so that whoever changes the shape of that store
next has the rows checked.

What the kernel tests of test_gpu_kernels.py do not look at: the gradient rows themselves (they see them through the d att
sum only) and the rows a launch must leave alone.  Every output here starts as a sentinel; fp64 references; inputs of small
integers with 1 / deg = 1 / 2 make every product and every sum exact in fp32, so those comparisons are bit for bit.
Shapes: at most 80 nodes, except the hub graph -- a node with more than 4 tiles of 32 slots has 129 neighbours at least.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NB = 32
SENTINEL = -12345.0


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops as o
    return o


def _symmetric(pairs):
    """(u, v, r) undirected -> directed edge lists with both directions (a self pair once)."""
    src, dst, rel = [], [], []
    for u, v, r in pairs:
        src.append(u); dst.append(v); rel.append(r)
        if u != v:
            src.append(v); dst.append(u); rel.append(r)
    return torch.tensor(src), torch.tensor(dst), torch.tensor(rel)


def _fan(u, vs, r=0):
    return [(u, v, r) for v in vs]


def _pair_grads_graphs():
    """name -> (N, R, src, dst, rel, symmetric, tiles of 32 slots the plan must have).  Directed graphs give a node tiles
    only where it is a source, so the tile count of the whole plan is chosen freely."""
    G = {}
    directed = lambda tr: tuple(torch.tensor(c) for c in zip(*tr))
    # exactly one tile in the whole plan (one role-2 workgroup, three idle waves); nodes 4, 5 without edges
    G['one_tile'] = (6, 2, *directed(_fan(0, [1, 2, 3]) + [(0, 2, 1)]), False, 1)
    # 5, 6, 7 tiles: the last role-2 workgroup has 3, 2, 1 idle waves; node 11 without edges
    for k in (5, 6, 7):
        tr = [(u, (u + 1 + j) % 11, (u + j) % 3) for u in range(k) for j in range(2 + u % 3)]
        G['tiles_%d' % k] = (12, 3, *directed(tr), False, k)
    # node 0 has exactly 32 neighbours (a full tile), node 1 has 33 (a second tile of one real slot and 31 pads);
    # symmetric, so the mirrored rows (second table of pg) are written too; nodes 34 .. 39 without edges
    tr = _fan(0, range(1, 33)) + _fan(1, range(2, 34), 1) + [(5, 9, 2), (5, 9, 3)]
    G['deg_32_33'] = (40, 4, *_symmetric(tr), True, 1 + 2 + 31 + 1)
    return G


def _hub_graph():
    """A hub with 5 tiles needs 129 neighbours at least: the one shape of this file above 80 nodes (136).  Node 5 is linked
    to 131 others (4 full tiles + 3 slots), a few pairs among the others, nodes 132 .. 135 without edges."""
    g = torch.Generator().manual_seed(136)
    tr = [(5, v, int(v) % 7) for v in range(132) if v != 5]
    u, v = torch.randint(0, 132, (60,), generator=g), torch.randint(0, 132, (60,), generator=g)
    seen = set()
    for a, b in zip(u.tolist(), v.tolist()):
        a, b = min(a, b), max(a, b)
        if a != b and 5 not in (a, b) and (a, b) not in seen:
            seen.add((a, b))
            tr.append((a, b, (a + b) % 7))
    return (136, 7, *_symmetric(tr), True, None)


_GRAPHS = _pair_grads_graphs()
_GRAPHS['hub_5_tiles'] = _hub_graph()


@pytest.mark.parametrize('d', [16, 32])
@pytest.mark.parametrize('name', sorted(_GRAPHS))
def test_pair_gradient_rows(ops, name, d):
    """`ops.pair_grads` into a pg buffer full of a sentinel: the row of every real slot == g'[v] . XB[u]^T (bit for bit on
    integers, within 2e-5 of fp64 on random inputs), every row no slot names still holds the sentinel (the plan's spare
    row, where the pad slots write, excepted), and a second call leaves the same bits."""
    from tip_amd.plan import build_pair_bwd_plan
    N, R, src, dst, rel, symmetric, want_tiles = _GRAPHS[name]
    assert N <= 80 or name == 'hub_5_tiles'
    g = torch.Generator().manual_seed(N + d)
    n_pad = -(-N // 8) * 8

    def run(scale, xb, gz):
        plan = build_pair_bwd_plan(src, dst, rel, N, R, scale, symmetric, 32, NB // 4, ops.rel_stream_piece())
        n_tiles = plan.n_slots // 32
        if want_tiles is not None:
            assert n_tiles == want_tiles
        else:
            assert int(plan.node_desc[0, 2]) > 4                                # the hub: heaviest node first
        u, v, slot = plan.slot_of_pair.unbind(1)
        dest = plan.slots[:, 3].to(torch.int64)
        spare = 2 * plan.n_alloc
        real = dest[slot]
        assert int(real.max()) < spare and int(torch.unique(real).numel()) == int(real.numel())
        assert bool((dest[dest != spare].sort().values == real.sort().values).all())
        want = torch.einsum('pbc,pc->pb', xb.double()[u], (gz.double() * scale.double().unsqueeze(1))[v])
        plan = plan.to(DEV)
        pg0 = torch.full((spare + 1, NB), SENTINEL, device=DEV)
        plan.pg[DEV] = pg0
        xb_pad = torch.zeros(n_pad, NB, 32)
        xb_pad[:N, :, :d] = xb
        xb_pad = xb_pad.to(DEV)
        cells = torch.zeros(n_pad, N, NB, device=DEV)
        pg, _ = ops.pair_grads(plan, cells, xb_pad[:, :, :d], gz.to(DEV))
        assert pg.data_ptr() == pg0.data_ptr()
        first = pg.clone()
        pg2, _ = ops.pair_grads(plan, cells, xb_pad[:, :, :d], gz.to(DEV))
        assert torch.equal(pg2, first)                                           # bitwise repeat
        got = first.cpu()
        untouched = torch.ones(spare + 1, dtype=torch.bool)
        untouched[real] = False
        untouched[spare] = False
        assert bool((got[untouched] == SENTINEL).all()), 'a row that no slot names was written'
        if bool((dest == spare).any()):                                         # pad slots: factor 0
            assert bool((got[spare] == 0).all())
        return got[real].double(), want

    # exact on integers with 1 / deg = 1 / 2
    xi = torch.randint(-3, 4, (N, NB, d), generator=g).float()
    gi = torch.randint(-3, 4, (N, d), generator=g).float()
    got, want = run(torch.full((N,), 0.5), xi, gi)
    assert torch.equal(got, want)
    # random inputs, the layer's own 1 / in-degree
    scale = 1.0 / torch.bincount(dst, minlength=N).clamp(min=1).float()
    got, want = run(scale, torch.randn(N, NB, d, generator=g), torch.randn(N, d, generator=g))
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5 * float(want.abs().max()))


def _small_symmetric_graph(N, R, seed):
    """Symmetric graph on N nodes: self pairs, pairs linked by several relations, relation R - 2 without edges, relation
    R - 1 with one, the last two nodes without edges."""
    g = torch.Generator().manual_seed(seed)
    tr = set()
    for r in range(R - 2):
        m = 2 + int(torch.randint(0, N, (1,), generator=g))
        u, v = torch.randint(0, N - 2, (m,), generator=g), torch.randint(0, N - 2, (m,), generator=g)
        tr |= {(min(a, b), max(a, b), r) for a, b in zip(u.tolist(), v.tolist())}
    tr |= {(0, 0, 0), (3, 3, 1), (1, 2, R - 1)}
    return _symmetric(sorted(tr))


@pytest.fixture(scope='module', params=[(7, 5), (33, 40)], ids=['n7', 'n33'])
def small_graph(request):
    N, R = request.param
    src, dst, rel = _small_symmetric_graph(N, R, N + R)
    assert int((src == dst).sum()) >= 2 and int((rel == R - 1).sum()) == 2
    g = torch.Generator().manual_seed(N)
    att0 = torch.randint(-3, 4, (R, NB), generator=g).float()
    att1 = torch.randint(-3, 4, (R, NB), generator=g).float()
    return N, R, src, dst, rel, att0, att1


def test_pair_cells_leave_unlinked_rows_alone(ops, small_graph):
    """`ops.stream_gather(write_zeros=False, kind=1)` and `ops.stream_gather_two` into sentinel-filled cell buffers: linked
    cells == the fp64 sum of att over their relations, exactly (integer tables); unlinked cells keep the sentinel."""
    from tip_amd.plan import build_stream_plan_rows
    N, R, src, dst, rel, att0, att1 = small_graph
    row = dst * N + src
    assert ops.stream_gather_split(R, NB, 1) == 1
    sp = build_stream_plan_rows(row, rel, N * N, R, 2, NB // 4, ops.rel_stream_piece()).to(DEV)
    linked = torch.zeros(N * N, dtype=torch.bool)
    linked[row] = True
    assert 0 < int(linked.sum()) < N * N

    def check(cells, att):
        got = cells.cpu().double()
        want = torch.zeros(N * N, NB, dtype=torch.float64).index_add_(0, row, att.double()[rel])
        assert torch.equal(got[linked], want[linked])
        assert bool((got[~linked] == SENTINEL).all()), 'the cell of an unlinked pair was written'

    cells = torch.full((N * N, NB), SENTINEL, device=DEV)
    ops.stream_gather(sp, att0.to(DEV), write_zeros=False, out=cells, kind=1)
    check(cells, att0)
    c0, c1 = torch.full((N * N, NB), SENTINEL, device=DEV), torch.full((N * N, NB), SENTINEL, device=DEV)
    ops.stream_gather_two(sp, att0.to(DEV), att1.to(DEV), c0, c1)
    check(c0, att0)
    check(c1, att1)
    assert torch.equal(c0, cells)


def test_att_slabs_are_sums_or_zeros(ops, small_graph):
    """`encoder.pair_att_gather_two`: every (partition, relation) row of both slab tensors == the exact sum of the
    symmetrised gradient rows of the pairs the relation links inside the partition -- zero where it links none (those rows
    come from the plan's zero_rows: the slabs are fresh allocations, nothing else writes them)."""
    from tip_amd import encoder
    from tip_amd.plan import build_pair_bwd_plan
    N, R, src, dst, rel, _, _ = small_graph
    scale = 1.0 / torch.bincount(dst, minlength=N).clamp(min=1).float()
    plan = build_pair_bwd_plan(src, dst, rel, N, R, scale, True, 32, NB // 4, ops.rel_stream_piece(), part_rows_max=64)
    assert (plan.n_parts > 1) == (N > 7)                                          # one partition, and several
    u, v, slot = plan.slot_of_pair.unbind(1)
    row_of_pair = torch.full((N * N,), -1, dtype=torch.int64)
    up = u <= v
    row_of_pair[(u * N + v)[up]] = plan.slots[:, 3].to(torch.int64)[slot[up]]     # first table: the pairs with u <= v
    ek = src <= dst                                                               # the edges the gather walks
    t = row_of_pair[(src * N + dst)[ek]]
    assert int(t.min()) >= 0 and int(t.max()) < plan.n_alloc
    g = torch.Generator().manual_seed(R)
    tables = [torch.randint(-3, 4, (2 * plan.n_alloc + 1, NB), generator=g).float() for _ in range(2)]
    n_zero = int(plan.gather.zero_ptr[-1])
    assert n_zero > 0                                                             # some (partition, relation) rows are zero_rows
    plan = plan.to(DEV)
    jobs = encoder.pair_att_gather_two(plan, tables[0].to(DEV), tables[1].to(DEV))
    for job, pg in zip(jobs, tables):
        slabs = job.keep[0]
        assert slabs.shape == (plan.n_parts, R, NB)
        both = (pg[:plan.n_alloc] + pg[plan.n_alloc:2 * plan.n_alloc]).double()
        want = torch.zeros(plan.n_parts * R, NB, dtype=torch.float64)
        want.index_add_(0, (t // plan.part_len) * R + rel[ek], both[t])
        assert torch.equal(slabs.cpu().double().view(-1, NB), want)
        assert int((want.abs().sum(1) == 0).sum()) >= n_zero
