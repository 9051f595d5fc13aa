"""Cases for the gather-sum family (`tip_amd/csrc/tipk_gather_sum.hip`): graphs whose in-degrees sit on every length the
kernels branch on, an fp64 reference, and two families of values.  No GPU, no fixtures: `tests/test_host_gather_cases.py`
checks on the CPU that the cases hold what they promise, `tests/test_gpu_gather_paths.py` runs the kernels on them.

The kernel's lengths (gather_sum_kernel): a slot of L lanes owns one work item of <= `chunk` edges; it fetches edge ids in
batches of STEP = max(L, 8) and keeps U = 8 rows in flight; a row of more than `chunk` edges is cut into pieces that the
finalize kernels (<= 8 slots: slot per row; more: wave per row) or, on a grouped plan, the workgroup's leader (<= G pieces,
G pieces fill the whole block) add in order.
"""
import torch

from tip_amd.plan import ITEM_DIRECT, ITEM_LEADER, ITEM_NULL, ITEM_PIECE

U = 8
EXACT_LIMIT = float(2 ** 22)          # magnitudes below it, values on a 2^-2 grid: 24 significant bits suffice


def pow2_at_least(x):
    p = 1
    while p < x:
        p *= 2
    return p


def lanes_for(d, vec=None):
    """Lanes per slot: d/4 rounded up to a power of two on the vector path (d % 4 == 0, everything 16-byte aligned), d rounded
    up on the scalar path.  vec=None: what an aligned call takes."""
    if vec is None:
        vec = d % 4 == 0
    return pow2_at_least(d // 4) if vec else pow2_at_least(d)


def group_slots(d, vec=None):
    """`plan.group_slots_for` for either path: a d % 4 == 0 row that is gathered by the scalar kernels (misaligned table / bias
    / out) needs the block size of ITS lane count."""
    lanes = lanes_for(d, vec)
    return max(min(128, 1024 // lanes), 64 // lanes)


def degree_ladder(L, chunk, G):
    """In-degrees of the output rows, in row order (see the module doc for what each length is a boundary of)."""
    step = max(L, U)
    deg = [0, 1, L - 1, L, L + 1, 7, 8, 9, step - 1, step, step + 1, 2 * step - 1, 2 * step, 2 * step + 1,
           chunk - 1, chunk, chunk + 1, 8 * chunk, 8 * chunk + 1, G * chunk, G * chunk + 1]
    seen, out = set(), []
    for k in deg:
        if k >= 0 and k not in seen:
            seen.add(k)
            out.append(k)
    return out + [G * chunk, 0, 0]          # a second full block; the last rows are empty like the first


def ladder_graph(deg, n_table, seed, shuffle=True):
    """(out_row, table_row), int64 [E]: output row r has deg[r] edges.  Every table row in [0, n_table) is gathered at least
    once.  Table rows 0 and n_table - 1: both twice in the largest row (a hub; duplicates within one row), row 0 alone in the
    row of degree 1, and both in the smallest row of degree >= 2 (a direct row wherever chunk >= its degree).
    shuffle: the edges come in a random caller order (the plan builders sort them)."""
    g = torch.Generator().manual_seed(seed)
    deg_t = torch.tensor(deg, dtype=torch.long)
    E = int(deg_t.sum())
    out_row = torch.repeat_interleave(torch.arange(len(deg)), deg_t)
    start = torch.cumsum(deg_t, 0) - deg_t
    table_row = torch.randint(0, n_table, (E,), generator=g)
    reserved = torch.zeros(E, dtype=torch.bool)

    def put(row, k, value):
        table_row[start[row] + k] = value
        reserved[start[row] + k] = True

    hub = int(torch.argmax(deg_t))
    assert deg[hub] >= 4
    for k, v in enumerate((0, 0, n_table - 1, n_table - 1)):
        put(hub, k, v)
    if 1 in deg:
        put(deg.index(1), 0, 0)
    small = [k for k in deg if k >= 2 and deg.index(k) != hub]
    if small:
        r = deg.index(min(small))
        put(r, 0, n_table - 1)
        put(r, 1, 0)
    free = torch.nonzero(~reserved).view(-1)
    assert free.numel() >= n_table, 'too few edges to use every table row'
    free = free[torch.randperm(free.numel(), generator=g)]
    table_row[free[:n_table]] = torch.arange(n_table)
    if shuffle:
        p = torch.randperm(E, generator=g)
        out_row, table_row = out_row[p], table_row[p]
    return out_row.contiguous(), table_row.contiguous()


def check_ladder(plan, deg, G=0):
    """The built plan holds the edge cases the ladder was made for (so that no test silently loses one)."""
    it = plan.items.cpu().long()
    n_out = len(deg)
    assert plan.n_out == n_out and plan.n_edges == sum(deg)
    if not G:
        assert plan.group_slots == 0
        slots = (plan.split_rows[:, 2] - plan.split_rows[:, 1]).cpu().long()
        assert plan.max_slots >= 9, plan.max_slots
        assert bool((slots == 8).any()), 'no row cut into exactly 8 slots'
        direct = it[it[:, 3] == ITEM_DIRECT]
    else:
        assert plan.group_slots == G and plan.n_slots == 0
        fl = it[:, 3]
        lead = fl[(fl & ITEM_LEADER) != 0]
        assert bool(((lead >> 8) == G).any()), 'no leader whose pieces fill the whole block'
        assert bool((fl == ITEM_NULL).any()), 'no padding items'
        n_blocks = int((fl != ITEM_DIRECT).sum()) // G
        assert bool((fl[:n_blocks * G] != ITEM_DIRECT).all()) and bool((fl[n_blocks * G:] == ITEM_DIRECT).all())
        # a leader's pieces are the next (flags >> 8) items of its own block
        for i in torch.nonzero((fl & ITEM_LEADER) != 0).view(-1).tolist():
            cnt = int(fl[i] >> 8)
            assert i // G == (i + cnt - 1) // G and bool(((fl[i:i + cnt] & ITEM_PIECE) != 0).all())
            assert bool((it[i:i + cnt, 2] == it[i, 2]).all())
        longer = (it[:, 1] - it[:, 0])[(fl & ITEM_PIECE) != 0]
        assert int(longer.max()) > plan.chunk, 'no row of more than G * chunk edges (longer pieces)'
        direct = it[fl == ITEM_DIRECT]
    assert bool((direct[:, 1] == direct[:, 0]).any()), 'no empty direct item'
    # every output row is delivered exactly once: as a direct item, a split row or a leader
    rows = [direct[:, 2]]
    rows.append(plan.split_rows[:, 0].cpu().long() if not G else it[(it[:, 3] & ITEM_LEADER) != 0, 2])
    assert sorted(torch.cat(rows).tolist()) == list(range(n_out))
    assert deg[0] == 0 and deg[-1] == 0


# ------------------------------------------------------------------------------------------------ reference
def reference(table64, out_row, table_row, n_out, w64=None, row_scale=None, bias=None, relu=False, gate=None):
    """out[o] = gate > 0 ? relu?(row_scale[o] * sum_{e: out_row[e] = o} w[e] table[table_row[e]] + bias) : 0, in float64."""
    rows = table64.double()[table_row]
    if w64 is not None:
        rows = rows * w64.double().unsqueeze(1)
    out = torch.zeros((n_out, table64.shape[1]), dtype=torch.float64).index_add_(0, out_row, rows)
    if row_scale is not None:
        out = out * row_scale.double().unsqueeze(1)
    if bias is not None:
        out = out + bias.double()
    if relu:
        out = torch.clamp_min(out, 0.0)
    if gate is not None:
        out = torch.where(gate.double() > 0, out, torch.zeros_like(out))
    return out


def magnitude(table64, out_row, table_row, n_out, w64=None, row_scale=None, bias=None):
    """sum |w t| |scale| + |bias| per output element: what every partial sum of the kernel is bounded by."""
    return reference(table64.abs(), out_row, table_row, n_out, None if w64 is None else w64.abs(),
                     None if row_scale is None else row_scale.abs(), None if bias is None else bias.abs())


def same_formula_fp32(table, out_row, table_row, n_out, w=None, row_scale=None, bias=None, relu=False, gate=None):
    """The reference's formula in fp32 on the CPU (plain torch): its distance from the fp64 result is what fp32 costs."""
    rows = table.float()[table_row]
    if w is not None:
        rows = rows * w.float().unsqueeze(1)
    out = torch.zeros((n_out, table.shape[1]), dtype=torch.float32).index_add_(0, out_row, rows)
    if row_scale is not None:
        out = out * row_scale.float().unsqueeze(1)
    if bias is not None:
        out = out + bias.float()
    if relu:
        out = torch.clamp_min(out, 0.0)
    if gate is not None:
        out = torch.where(gate > 0, out, torch.zeros_like(out))
    return out


def assert_exact(ref64, mag64):
    """The `exact` condition: every value on the 2^-2 grid and every magnitude below 2^22 -- then every partial sum, in any
    order and with or without fused multiply-adds, is a multiple of 2^-2 below 2^22, i.e. exact in fp32."""
    assert torch.equal(ref64 * 4, torch.round(ref64 * 4)), 'values off the 2^-2 grid'
    assert float(mag64.max()) < EXACT_LIMIT, float(mag64.max())
    assert bool((mag64 >= ref64.abs()).all())


# ------------------------------------------------------------------------------------------------ values
W_SET = (-1.0, 0.25, 0.5, 1.0, 2.0)


def exact_values(n_table, d, E, n_out, seed, weighted, t_max=8):
    """table: integers in [-t_max, t_max]; w: from W_SET (or None); row_scale: powers of two in {1, 2, 4}; bias: integers in
    [-3, 3].  All float32."""
    g = torch.Generator().manual_seed(seed + 1000)
    table = torch.randint(-t_max, t_max + 1, (n_table, d), generator=g).float()
    w = torch.tensor(W_SET)[torch.randint(0, len(W_SET), (E,), generator=g)] if weighted else None
    scale = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (n_out,), generator=g)]
    bias = torch.randint(-3, 4, (d,), generator=g).float()
    return table, w, scale, bias


def normal_values(n_table, d, E, n_out, seed, weighted):
    g = torch.Generator().manual_seed(seed + 2000)
    table = torch.randn(n_table, d, generator=g)
    w = torch.rand(E, generator=g) if weighted else None
    scale = torch.rand(n_out, generator=g) + 0.5
    bias = torch.randn(d, generator=g)
    return table, w, scale, bias


class Case(object):
    """One ladder graph with values: everything a test needs on the CPU."""

    def __init__(self, d, chunk, weighted, family='exact', vec=None, max_degree=None, n_table=50, t_max=8, seed=None):
        self.d, self.chunk, self.weighted, self.family = d, chunk, weighted, family
        self.L = lanes_for(d, vec)
        self.G = group_slots(d, vec)
        deg = degree_ladder(self.L, chunk, self.G)
        if max_degree is not None:                       # truncated ladder; the rows at both ends stay empty
            deg = [k for k in deg if k <= max_degree]
        self.deg, self.n_out, self.n_table = deg, len(deg), n_table
        self.seed = (d * 131 + chunk * 7 + int(weighted)) if seed is None else seed
        self.out_row, self.table_row = ladder_graph(deg, n_table, self.seed)
        self.E = int(self.out_row.numel())
        make = exact_values if family == 'exact' else normal_values
        kw = {'t_max': t_max} if family == 'exact' else {}
        self.table, self.w, self.scale, self.bias = make(n_table, d, self.E, self.n_out, self.seed, weighted, **kw)

    def plan(self, G=0):
        from tip_amd.plan import build_gather_plan
        return build_gather_plan(self.out_row, self.table_row, self.n_out, self.n_table, self.w, self.chunk, 'ladder', G)

    def ref(self, epilogue=False, gate=None, table=None):
        t = self.table if table is None else table
        w64 = None if self.w is None else self.w.double()
        if epilogue:
            return reference(t.double(), self.out_row, self.table_row, self.n_out, w64, self.scale, self.bias, True, gate)
        return reference(t.double(), self.out_row, self.table_row, self.n_out, w64, gate=gate)

    def mag(self, epilogue=False):
        w64 = None if self.w is None else self.w.double()
        if epilogue:
            return magnitude(self.table.double(), self.out_row, self.table_row, self.n_out, w64, self.scale, self.bias)
        return magnitude(self.table.double(), self.out_row, self.table_row, self.n_out, w64)

    def cpu32(self, epilogue=False, gate=None):
        if epilogue:
            return same_formula_fp32(self.table, self.out_row, self.table_row, self.n_out, self.w, self.scale, self.bias, True, gate)
        return same_formula_fp32(self.table, self.out_row, self.table_row, self.n_out, self.w, gate=gate)

    def assert_exact(self):
        assert self.family == 'exact'
        assert_exact(self.ref(False), self.mag(False))
        assert_exact(self.ref(True), self.mag(True))


# widths of section A: (d, vec).  vec=False with d % 4 == 0: the table is offset by one float
VEC_WIDTHS = [4, 8, 12, 20, 32, 40, 64, 96, 128, 200, 256]
SCALAR_WIDTHS = [(1, None), (3, None), (6, None), (33, None), (50, None), (64, False)]
CHUNKS = [16, 1]
LIN_SHAPES = [(16, 4), (16, 8), (16, 16), (32, 8), (32, 16), (64, 16)]
CSR_WIDTHS = [8, 12, 32, 64, 128, 200, 256]


def lin_case(d, d2, weighted, chunk=16):
    """`exact` case of gather_sum_lin: table in [-4, 4], degrees <= chunk + 1, an integer map in [-4, 4] and bias2 in [-3, 3]."""
    c = Case(d, chunk, weighted, 'exact', max_degree=chunk + 1, t_max=4, seed=d * 17 + d2)
    g = torch.Generator().manual_seed(c.seed + 5)
    c.weight = torch.randint(-4, 5, (d2, d), generator=g).float()
    c.bias2 = torch.randint(-3, 4, (d2,), generator=g).float()
    return c


def lin_reference(agg64, weight, bias2=None, relu=False):
    out2 = agg64 @ weight.double().t()
    if bias2 is not None:
        out2 = out2 + bias2.double()
    return torch.clamp_min(out2, 0.0) if relu else out2


def lin_magnitude(agg_mag64, weight, bias2=None):
    return lin_reference(agg_mag64, weight.abs(), None if bias2 is None else bias2.abs())


def csr_rows_per_task(d):
    """Rows one slot of the csr kernel takes: L - 1 up to 16, L = max(2, d/4 rounded up to a power of two) lanes."""
    L = max(2, pow2_at_least(d // 4))
    return L - 1 if L <= 16 else 16


def csr_degrees(rp, n_out):
    """Row lengths for `gather_rows_csr` over tasks of rp rows: lengths 7, 8, 9, 17 (the 8 rows in flight), a task whose first
    rows are empty, one whose last rows are empty, and an entirely empty task between two full ones -- cut or padded with
    a short pattern to n_out rows."""
    if n_out == 1:
        return [9]
    first_empty = [0] * (rp - 1) + [9] if rp > 1 else [9]
    last_empty = [8] + [0] * (rp - 1)
    full = [7, 8, 9, 17, 1, 2, 3, 5]
    full = (full * (rp // len(full) + 1))[:rp]
    deg = first_empty + last_empty + full + [0] * rp + full[::-1] + [17, 0, 7]
    while len(deg) < n_out:
        deg += [1, 0, 3, 0, 0, 9, 2]
    return deg[:n_out]


def csr_n_outs(rp):
    """1, rp, rp + 1 and 6 rp + 5: no multiple of rp for rp in {3, 7, 15, 16}, and long enough for all of `csr_degrees`."""
    return sorted({1, rp, rp + 1, 6 * rp + 5})


# ------------------------------------------------------------------------------------------------ autograd graph (section J)
def edge_graph(n, seed=3):
    """COO edge_index [2, E] on n nodes with: isolated nodes (no edge at all), self-loops, duplicate edges, a hub (node 3 as
    destination of a third of the edges).  -> (edge_index, hub, isolated)."""
    if n == 1:
        return torch.zeros((2, 2), dtype=torch.long), 0, 0          # two self-loops on the only node
    g = torch.Generator().manual_seed(seed)
    e = 6 * n
    live = torch.arange(n)[(torch.arange(n) % 7) != 5]               # nodes 5, 12, 19, ... stay isolated
    src = live[torch.randint(0, live.numel(), (e,), generator=g)]
    dst = live[torch.randint(0, live.numel(), (e,), generator=g)]
    dst[: e // 3] = 3
    src[e // 3: e // 3 + 10] = dst[e // 3: e // 3 + 10]              # self-loops
    src = torch.cat([src, src[:40]])
    dst = torch.cat([dst, dst[:40]])                                 # duplicates
    return torch.stack([src, dst]), 3, 5


def norm_edges(edge_index, n, rows=None):
    """`layers.gcn_norm_graph` built on the CPU: (graph with CPU plans, out_row, table_row, w fp32 in caller order, n_out) of
    the forward aggregation -- the weights are the ones the plans hold, so a reference shares the kernel's inputs."""
    from tip_amd.layers import gcn_norm_graph
    graph = gcn_norm_graph(edge_index, n, 16, d=32, rows=rows)
    row, col = edge_index[0], edge_index[1]
    keep = row != col
    loop = torch.arange(n)
    row, col = torch.cat([row[keep], loop]), torch.cat([col[keep], loop])
    n_out = n
    if rows is not None:
        inv = torch.full((n,), -1, dtype=torch.long)
        inv[rows] = torch.arange(rows.numel())
        sel = inv[col] >= 0
        row, col = row[sel], inv[col[sel]]
        n_out = int(rows.numel())
    fwd = graph.fwd
    w = torch.zeros(row.numel(), dtype=torch.float32)
    w[fwd.perm] = fwd.edge_w
    assert torch.equal(fwd.row_id.long(), row[fwd.perm])
    return graph, col, row, w, n_out


def conv_pre(kind, x, weight, bias, out_row, table_row, w, n_out):
    """Pre-activation of the three autograd entries in the dtype of its inputs: 'aggregate' A x + b, 'gcn_conv' A (x W^T) + b,
    'agg_first' (A x) W^T + b."""
    def agg(t):
        return torch.zeros((n_out, t.shape[1]), dtype=t.dtype).index_add_(0, out_row, t[table_row] * w.to(t.dtype).unsqueeze(1))
    if kind == 'aggregate':
        return agg(x) + bias
    if kind == 'gcn_conv':
        return agg(x @ weight.t()) + bias
    return agg(x) @ weight.t() + bias


def conv_reference(kind, x, weight, bias, up, out_row, table_row, w, n_out):
    """-> {name: (ref64, cpu32, mag64)} for out and the gradients of x, weight ('aggregate': none), bias under relu.
    mag: the same expression over absolute values with the fp64 ReLU mask -- the sum of |terms| of every element."""
    res = {}
    leaves = {}
    for dt in (torch.float64, torch.float32):
        xs = [None if t is None else t.detach().to(dt).clone().requires_grad_() for t in (x, weight, bias)]
        pre = conv_pre(kind, xs[0], xs[1], xs[2], out_row, table_row, w, n_out)
        out = torch.relu(pre)
        out.backward(up.to(dt))
        leaves[dt] = (pre.detach(), out.detach(), xs)
    pre64, out64, l64 = leaves[torch.float64]
    _, out32, l32 = leaves[torch.float32]
    mask = (pre64 > 0).double()
    xa = [None if t is None else t.detach().double().abs().requires_grad_() for t in (x, weight, bias)]
    pre_abs = conv_pre(kind, xa[0], xa[1], xa[2], out_row, table_row, w.abs(), n_out)
    (pre_abs * (up.double().abs() * mask)).sum().backward()
    res['out'] = (out64, out32, pre_abs.detach())
    for name, i in (('d_x', 0), ('d_weight', 1), ('d_bias', 2)):
        if l64[i] is not None:
            res[name] = (l64[i].grad, l32[i].grad, xa[i].grad)
    res['margin'] = float((pre64.abs() / pre_abs.detach().clamp(min=1e-300)).min())
    return res


def autograd_case(kind, n, d_in=32, d_out=16):
    """Inputs of section J on the CPU: the graph of `edge_graph`, kept rows (hub, an isolated node, 0, n - 1 and every third
    node) for 'agg_first'."""
    g = torch.Generator().manual_seed(n * 3 + len(kind))
    ei, hub, iso = edge_graph(n)
    rows = None
    if kind == 'agg_first':
        rows = torch.tensor(sorted(set([0, n - 1, hub, iso] + list(range(0, n, 3)))) if n > 1 else [0])
    graph, out_row, table_row, w, n_out = norm_edges(ei, n, rows)
    d_x = d_out if kind == 'aggregate' else d_in
    x = torch.randn(n, d_x, generator=g)
    wt = torch.randn(d_in, d_out, generator=g)          # [in, out] storage behind a [out, in] view, as the layers keep it
    bias = torch.randn(d_out, generator=g)
    up = torch.randn(n_out, d_out, generator=g)
    return dict(kind=kind, n=n, graph=graph, rows=rows, x=x, wt=wt, bias=bias, up=up,
                edges=(out_row, table_row, w, n_out))
