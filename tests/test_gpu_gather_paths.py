"""-m gpu: the gather-sum family (`tip_amd/csrc/tipk_gather_sum.hip`: tipk_gather_sum, _finalize, _riders, _lin and
tipk_gather_rows_csr) against fp64 at the lengths, widths and layouts the kernels branch on (`tests/gather_cases.py`).

Sections A-H use the `exact` family: every partial sum is exact in fp32 in any order, so the kernels must equal the fp64
reference BIT FOR BIT -- one dropped, doubled or misplaced edge changes a result by at least 2^-2.  Sections I and J use
normal values and the per-element bound of `tests/test_gpu_eval_paths.py`:
    |got - fp64| <= max(8 x |torch fp32 CPU same formula - fp64|, 4 fp32 ulps of the element's sum of |terms|).
The errors seen on an MI355X next to these bounds are recorded in profiles/gather_paths_errors.md.
"""
import functools
import os

import numpy as np
import pytest
import torch

import gather_cases as C

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -123.4375


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops as o
    return o


def tipk_error():
    from tip_amd._lib import TipkError
    return TipkError


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def assert_bits(got, ref64, what=''):
    """got (fp32) == the fp64 reference bit for bit (the reference is representable in fp32: `exact` family)."""
    want = ref64.to(torch.float32)
    assert torch.equal(want.double(), ref64) or not torch.isfinite(ref64).all()
    g = got.detach().cpu().reshape(want.shape)
    same = bits(g) == bits(want)
    if not bool(same.all()):
        bad = torch.nonzero(~same)
        raise AssertionError('%s: %d of %d elements differ, in %d rows; first at %s: got %r, want %r'
                             % (what, int((~same).sum()), same.numel(), int((~same).reshape(same.shape[0], -1).any(1).sum()),
                                tuple(bad[0].tolist()), float(g[tuple(bad[0].tolist())]), float(want[tuple(bad[0].tolist())])))


@functools.lru_cache(maxsize=None)
def case(d, chunk, weighted, vec=None, family='exact', max_degree=None):
    c = C.Case(d, chunk, weighted, family, vec=vec, max_degree=max_degree)
    if family == 'exact':
        c.assert_exact()
    return c


def offset_by_one_float(t):
    """A copy of t on the device whose storage starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def run_both_epilogues(ops, c, plan, table, bias=None, what=''):
    """gather_sum over a NaN-filled output, plain and with row_scale / bias / relu: bit-equal to fp64, twice the same bits."""
    scale = c.scale.to(DEV)
    bias = c.bias.to(DEV) if bias is None else bias
    for epi in (False, True):
        kw = dict(row_scale=scale, bias=bias, relu=True) if epi else {}
        out = torch.full((c.n_out, c.d), float('nan'), device=DEV)
        ops.gather_sum(plan, table, out=out, **kw)
        assert_bits(out, c.ref(epi), '%s epilogue=%s' % (what, epi))
        assert torch.equal(bits(out), bits(ops.gather_sum(plan, table, **kw))), what


# ------------------------------------------------------------------------------------------------ A. gather_sum, exact
WIDTHS = [(d, None) for d in C.VEC_WIDTHS] + C.SCALAR_WIDTHS


@pytest.mark.parametrize('chunk', C.CHUNKS)
@pytest.mark.parametrize('d,vec', WIDTHS)
def test_gather_sum_exact_on_the_ladder(ops, d, vec, chunk):
    """Every width (vector path: also d % 4 == 0 that are no power of two, whose slots have masked lanes; scalar path: also a
    64-float row behind a misaligned table) x weighted / unweighted x ungrouped + finalize / grouped, on the degree ladder:
    bit-equal to fp64 with and without the epilogue, every row written (both ends of the output are empty rows), repeatable."""
    for weighted in (False, True):
        c = case(d, chunk, weighted, vec)
        table = offset_by_one_float(c.table) if vec is False else c.table.to(DEV)
        for G in (0, c.G):
            plan = c.plan(G).to(DEV)
            C.check_ladder(plan, c.deg, G)
            run_both_epilogues(ops, c, plan, table, what='d=%d chunk=%d weighted=%s G=%d' % (d, chunk, weighted, G))


@pytest.mark.parametrize('G', [0, 128])
def test_gather_sum_of_an_edgeless_graph_writes_every_row(ops, G):
    """E = 0: the plan holds one empty item per row and the kernel writes the epilogue of a zero sum (row_id has no storage)."""
    from tip_amd.plan import build_gather_plan
    e = torch.zeros(0, dtype=torch.long)
    plan = build_gather_plan(e, e, 13, 5, None, 16, group_slots=G).to(DEV)
    table = torch.ones(5, 8, device=DEV)
    bias = torch.arange(8.0, device=DEV) - 3
    out = torch.full((13, 8), float('nan'), device=DEV)
    ops.gather_sum(plan, table, out=out)
    assert_bits(out, torch.zeros(13, 8, dtype=torch.float64))
    ops.gather_sum(plan, table, out=out, row_scale=torch.full((13,), 2.0, device=DEV), bias=bias, relu=True)
    assert_bits(out, torch.clamp_min(bias.double().cpu(), 0).expand(13, 8))


# ------------------------------------------------------------------------------------------------ B. layouts
@pytest.mark.parametrize('d', [12, 32, 200, 6, 33])
def test_out_and_table_as_column_slices(ops, d):
    """out = a column slice of a wider buffer (ld_out = d + 32): the columns on both sides keep their sentinel; table = the
    middle third of a [n_table, 3 d] buffer whose other columns are NaN."""
    c = case(d, 16, True)
    wide_t = torch.full((c.n_table, 3 * d), float('nan'), device=DEV)
    wide_t[:, d:2 * d] = c.table.to(DEV)
    for G in (0, c.G):
        plan = c.plan(G).to(DEV)
        for epi in (False, True):
            kw = dict(row_scale=c.scale.to(DEV), bias=c.bias.to(DEV), relu=True) if epi else {}
            wide = torch.full((c.n_out, d + 32), SENTINEL, device=DEV)
            ops.gather_sum(plan, wide_t[:, d:2 * d], out=wide[:, 16:16 + d], **kw)
            assert_bits(wide[:, 16:16 + d], c.ref(epi), 'd=%d G=%d' % (d, G))
            side = torch.full((c.n_out, 16), SENTINEL)
            assert torch.equal(bits(wide[:, :16]), bits(side)) and torch.equal(bits(wide[:, 16 + d:]), bits(side))


@pytest.mark.parametrize('which', ['table', 'bias'])
@pytest.mark.parametrize('d', [12, 32, 64, 96, 200])
def test_misaligned_table_or_bias(ops, d, which):
    """A table or a bias that starts one float past a 16-byte boundary takes the scalar kernels: exact for d <= 64, refused
    (TipkError, nothing computed) for wider rows."""
    c = case(d, 16, True, False if d <= 64 else None)
    table = offset_by_one_float(c.table) if which == 'table' else c.table.to(DEV)
    bias = offset_by_one_float(c.bias) if which == 'bias' else c.bias.to(DEV)
    if d <= 64:
        for G in (0, c.G):
            plan = c.plan(G).to(DEV)
            if which == 'table':
                run_both_epilogues(ops, c, plan, table, bias, 'd=%d G=%d' % (d, G))
            else:
                out = torch.full((c.n_out, d), float('nan'), device=DEV)
                ops.gather_sum(plan, table, out=out, row_scale=c.scale.to(DEV), bias=bias, relu=True)
                assert_bits(out, c.ref(True), 'd=%d G=%d' % (d, G))
        return
    for G in (0, c.G):
        out = torch.full((c.n_out, d), SENTINEL, device=DEV)
        with pytest.raises(tipk_error()):
            ops.gather_sum(c.plan(G).to(DEV), table, out=out, bias=bias)
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(torch.full((c.n_out, d), SENTINEL)))


def test_group_slots_that_do_not_fit_the_width_are_refused(ops):
    c = case(128, 16, True)
    with pytest.raises(tipk_error()):                       # 64 items x 32 lanes: more than one workgroup
        ops.gather_sum(c.plan(64).to(DEV), c.table.to(DEV))
    c = case(64, 16, True)                                  # the vector path's G = 64 behind a misaligned table: 64 x 64 lanes
    with pytest.raises(tipk_error()):
        ops.gather_sum(c.plan(64).to(DEV), offset_by_one_float(c.table))


# ------------------------------------------------------------------------------------------------ C. finalize
@pytest.mark.parametrize('max_slots', [8, 9])
@pytest.mark.parametrize('d', [128, 256, 12, 3, 50])
def test_finalize_at_eight_and_nine_slots(ops, d, max_slots):
    """Ungrouped plans whose most split row has exactly 8 / 9 slots: the slot-per-row kernel (vector path, d <= 128) and the
    wave-per-row kernel; exact."""
    chunk = 16
    c = case(d, chunk, True, None, 'exact', 8 * chunk + (max_slots - 8))
    plan = c.plan(0).to(DEV)
    assert plan.max_slots == max_slots and plan.n_slots > 0
    run_both_epilogues(ops, c, plan, c.table.to(DEV), what='d=%d max_slots=%d' % (d, max_slots))


# ------------------------------------------------------------------------------------------------ D. riders, gate, column sums
def ladder_gate(c, seed=1):
    """gate [n_out, d]: normal values; exact zeros, negative zeros and negative values on the hub rows and on the empty rows."""
    gate = torch.randn(c.n_out, c.d, generator=torch.Generator().manual_seed(seed))
    special = [0, c.n_out - 1, c.n_out - 2] + [r for r, k in enumerate(c.deg) if k >= c.G * c.chunk]
    for r in special:
        gate[r, 0::4] = 0.0
        gate[r, 1::4] = -0.0
        gate[r, 2::4] = -1.5
    return gate


def with_padding_block(plan, G):
    """The plan with one more block of G null items behind its grouped blocks: a workgroup that holds only padding."""
    from tip_amd.plan import GatherPlan, ITEM_DIRECT, ITEM_NULL
    it = plan.items
    n_grouped = int((it[:, 3] != ITEM_DIRECT).sum())
    pad = torch.zeros((G, 4), dtype=torch.int32, device=it.device)
    pad[:, 3] = ITEM_NULL
    items = torch.cat([it[:n_grouped], pad, it[n_grouped:]], 0).contiguous()
    return GatherPlan(plan.n_out, plan.n_table, plan.row_id, plan.edge_w, items, plan.split_rows, 0, plan.perm, plan.chunk,
                      plan.tag, G), n_grouped // G


@pytest.mark.parametrize('d', [32, 20, 12])
def test_riders_gate_and_column_sums(ops, d):
    """tipk_gather_sum_riders on the ladder: out bit-equal to the masked plain gather and to fp64, the per-workgroup column
    sums add up to the fp64 column sums exactly, a workgroup of padding writes a zero row, three riders equal `sum_slabs`."""
    c = case(d, 16, True)
    plan, pad_block = with_padding_block(c.plan(c.G).to(DEV), c.G)
    table, scale, bias = c.table.to(DEV), c.scale.to(DEV), c.bias.to(DEV)
    g = torch.Generator().manual_seed(d)
    slabs = [torch.randn(256, 1, 32, generator=g).to(DEV), torch.randn(11, 32, 16, generator=g).to(DEV), torch.randn(57, 1, 16, generator=g).to(DEV)]
    plain = ops.gather_sum(plan, table, row_scale=scale, bias=bias, relu=True)
    assert_bits(plain, c.ref(True))
    assert ops.gather_sum_epilogue_supported(plan, d) == (d in (32, 20))
    assert bool(ops.lib().tipk_gather_sum_riders_supported(d, plan.group_slots)) == (d in (32, 20))
    if d == 12:                                             # 128 items x 4 lanes: the riders take a launch of their own
        jobs = [ops.slab_job(s, alpha=0.5) for s in slabs]
        assert torch.equal(bits(ops.gather_sum(plan, table, row_scale=scale, bias=bias, relu=True, riders=jobs)), bits(plain))
        for j, s in zip(jobs, slabs):
            assert torch.equal(bits(j.out), bits(ops.sum_slabs(s, alpha=0.5)))
        return
    gate = ladder_gate(c)
    ref = c.ref(True, gate=gate)
    C.assert_exact(ref.sum(0, keepdim=True), c.mag(True).sum(0, keepdim=True))
    masked = torch.where(gate.to(DEV) > 0, plain, torch.zeros_like(plain))
    seen = []
    for rep in range(2):
        jobs = [ops.slab_job(s, alpha=0.5) for s in slabs]
        out = torch.full((c.n_out, d), float('nan'), device=DEV)
        res, parts = ops.gather_sum(plan, table, row_scale=scale, bias=bias, relu=True, out=out, riders=jobs, gate=gate.to(DEV), colsum=True)
        assert res is out
        assert torch.equal(bits(out), bits(masked))
        assert_bits(out, ref, 'gated d=%d' % d)
        assert parts.shape == (-(-plan.items.shape[0] // plan.group_slots), 1, d)
        assert_bits(parts.double().cpu().sum((0, 1)).float(), ref.sum(0), 'column sums d=%d' % d)
        assert_bits(parts[pad_block, 0], torch.zeros(d, dtype=torch.float64), 'padding workgroup')
        for j, s in zip(jobs, slabs):
            assert torch.equal(bits(j.out), bits(ops.sum_slabs(s, alpha=0.5)))
        seen.append(bits(parts))
    assert torch.equal(seen[0], seen[1])
    assert torch.equal(bits(ops.gather_sum(plan, table, row_scale=scale, bias=bias, relu=True, gate=gate.to(DEV))), bits(masked))


# ------------------------------------------------------------------------------------------------ E. gather_sum_lin
@pytest.mark.parametrize('d,d2', C.LIN_SHAPES)
def test_gather_sum_lin_all_instantiations(ops, d, d2):
    """All six (lanes, outputs per lane) forms; the weight as [d2, d] contiguous and as the transposed view of [d, d2] storage;
    with and without bias / relu / row_scale: agg and out2 bit-equal to fp64."""
    assert ops.gather_sum_lin_supported(d, d2, C.group_slots(d))
    for weighted in (False, True):
        c = C.lin_case(d, d2, weighted)
        plan = c.plan(c.G).to(DEV)
        table = c.table.to(DEV)
        w64 = None if c.w is None else c.w.double()
        layouts = [c.weight.to(DEV).contiguous(), c.weight.t().contiguous().to(DEV).t()]
        assert layouts[0].stride() == (d, 1) and layouts[1].stride() == (1, d2)
        for scale in (None, c.scale):
            agg64 = C.reference(c.table.double(), c.out_row, c.table_row, c.n_out, w64, scale)
            for b2, relu in ((None, False), (c.bias2, True), (c.bias2, False)):
                want2 = C.lin_reference(agg64, c.weight, b2, relu)
                for wt in layouts:
                    agg, out2 = ops.gather_sum_lin(plan, table, wt, None if b2 is None else b2.to(DEV), relu,
                                                   row_scale=None if scale is None else scale.to(DEV))
                    what = 'd=%d d2=%d weighted=%s scale=%s bias=%s relu=%s strides=%s' % (
                        d, d2, weighted, scale is not None, b2 is not None, relu, wt.stride())
                    assert_bits(agg, agg64, 'agg ' + what)
                    assert_bits(out2, want2, 'out2 ' + what)


@pytest.mark.parametrize('d,d2', [(16, 32), (32, 4), (64, 8), (64, 32), (20, 5), (128, 32), (8, 8)])
def test_gather_sum_lin_refuses_other_shapes(ops, d, d2):
    assert not ops.gather_sum_lin_supported(d, d2, C.group_slots(d))
    c = case(d, 16, False, None, 'exact', 17)
    with pytest.raises(tipk_error()):
        ops.gather_sum_lin(c.plan(c.G).to(DEV), c.table.to(DEV), torch.ones(d2, d, device=DEV))


# ------------------------------------------------------------------------------------------------ F. gather_rows_csr
def csr_call(ops, plan, table, out):
    """tipk_gather_rows_csr into a caller's buffer (the wrapper allocates its own)."""
    from tip_amd._lib import check, lib, ptr, stream_ptr
    check(lib().tipk_gather_rows_csr(ptr(table), table.stride(0), table.shape[0], ptr(plan.row_ptr), ptr(plan.row_id), plan.n_out,
                                     ptr(out), out.stride(0), table.shape[1], stream_ptr(table.device)), 'tipk_gather_rows_csr')


@pytest.mark.parametrize('d', C.CSR_WIDTHS)
def test_gather_rows_csr_exact_at_task_edges(ops, d):
    """n_out = 1, rp, rp + 1 and no multiple of rp (rp rows per slot); tasks whose first / last rows are empty, an empty task
    between two full ones, row lengths 7, 8, 9, 17; E = 0.  Exact; every row written over NaN."""
    from tip_amd.plan import build_csr_plan
    rp = C.csr_rows_per_task(d)
    n_table = 11
    table = torch.randint(-8, 9, (n_table, d), generator=torch.Generator().manual_seed(d)).float()
    for n_out in C.csr_n_outs(rp):
        deg = C.csr_degrees(rp, n_out)
        if sum(deg) >= 15:
            out_row, table_row = C.ladder_graph(deg, n_table, seed=d + n_out)
        else:
            out_row, table_row = torch.repeat_interleave(torch.arange(n_out), torch.tensor(deg)), torch.arange(sum(deg)) % n_table
        ref = C.reference(table.double(), out_row, table_row, n_out)
        plan = build_csr_plan(out_row.to(DEV), table_row.to(DEV), n_out, n_table)
        out = torch.full((n_out, d), float('nan'), device=DEV)
        csr_call(ops, plan, table.to(DEV), out)
        assert_bits(out, ref, 'd=%d n_out=%d' % (d, n_out))
        assert torch.equal(bits(out), bits(ops.gather_rows_csr(plan, table.to(DEV))))
    e = torch.zeros(0, dtype=torch.long, device=DEV)
    for n_out in (1, rp + 1, 40):
        out = torch.full((n_out, d), float('nan'), device=DEV)
        csr_call(ops, build_csr_plan(e, e, n_out, n_table), table.to(DEV), out)
        assert_bits(out, torch.zeros(n_out, d, dtype=torch.float64), 'E=0 d=%d n_out=%d' % (d, n_out))


# ------------------------------------------------------------------------------------------------ G. offsets around 2^31 and 2^32
def big_table_case(n_table, d):
    """Five table rows of a table of 128-byte rows: row 0, the last row that ends at byte 2^31, the two rows that start at and
    after byte 2^31 (with a power-of-two row stride -- the only strides for which n_table * ld * 4 can be 2^32 -- no row
    straddles that byte: these are the rows on both sides of it), and the last row.  Output rows gather them one by one,
    all together (one of them twice), and not at all."""
    k = (1 << 31) // (d * 4)
    special = [0, k - 1, k, k + 1, n_table - 1]
    pairs = [(i + 1, s) for i, s in enumerate(special)] + [(6, s) for s in special] + [(6, special[2]), (7, special[4]), (7, special[1])]
    out_row = torch.tensor([p[0] for p in pairs])
    table_row = torch.tensor([p[1] for p in pairs])
    vals = torch.randint(-8, 9, (5, d), generator=torch.Generator().manual_seed(n_table % 1000)).float()
    compact = torch.tensor([special.index(int(t)) for t in table_row])
    ref = C.reference(vals.double(), out_row, compact, 9)
    return special, out_row, table_row, vals, ref


def run_big_table(ops, n_floats, n_table, d, misaligned, expect_small):
    from tip_amd.plan import build_csr_plan, build_gather_plan
    special, out_row, table_row, vals, ref = big_table_case(n_table, d)
    buf = torch.empty(n_floats + (1 if misaligned else 0), dtype=torch.float32, device=DEV)
    try:
        table = buf[1 if misaligned else 0:].view(n_table, d)
        assert (table.data_ptr() % 16 == 4) == misaligned
        assert (n_table * d * 4 < (1 << 32)) == expect_small
        table[torch.tensor(special, device=DEV)] = vals.to(DEV)
        for G in (0, C.group_slots(d, vec=not misaligned)):
            plan = build_gather_plan(out_row, table_row, 9, n_table, None, 2, group_slots=G).to(DEV)
            out = torch.full((9, d), float('nan'), device=DEV)
            ops.gather_sum(plan, table, out=out)
            assert_bits(out, ref, 'G=%d' % G)
            wts = torch.tensor(C.W_SET)[torch.arange(out_row.numel()) % 5]
            plan = build_gather_plan(out_row, table_row, 9, n_table, wts, 2, group_slots=G).to(DEV)
            compact = torch.tensor([special.index(int(t)) for t in table_row])
            ops.gather_sum(plan, table, out=out)
            assert_bits(out, C.reference(vals.double(), out_row, compact, 9, wts.double()), 'weighted G=%d' % G)
        if misaligned:
            return
        csr = build_csr_plan(out_row.to(DEV), table_row.to(DEV), 9, n_table)
        lin_plan = build_gather_plan(out_row, table_row, 9, n_table, None, 2, group_slots=C.group_slots(d)).to(DEV)
        weight = torch.eye(d, device=DEV)[:16].contiguous()
        if expect_small:
            assert_bits(ops.gather_rows_csr(csr, table), ref, 'csr')
            agg, out2 = ops.gather_sum_lin(lin_plan, table, weight)
            assert_bits(agg, ref, 'lin agg')
            assert_bits(out2, ref[:, :16], 'lin out2')
        else:
            with pytest.raises(tipk_error()):
                ops.gather_rows_csr(csr, table)
            with pytest.raises(tipk_error()):
                ops.gather_sum_lin(lin_plan, table, weight)
    finally:
        del buf
        torch.cuda.empty_cache()


def test_table_just_below_4_gib_takes_32_bit_offsets(ops):
    """(a) n_table * ld * 4 = 2^32 - ld * 4: byte offsets up to 2^32 - 256 in 32 bits (a signed offset would go wrong from
    2^31 on) -- gather_sum, gather_rows_csr and gather_sum_lin all run, exact."""
    d = 32
    n_table = (1 << 32) // (d * 4) - 1
    run_big_table(ops, n_table * d, n_table, d, False, True)


def test_table_of_exactly_4_gib_takes_the_general_route(ops):
    """(b) exactly 2^32 bytes: 64-bit row addresses in gather_sum; gather_rows_csr and gather_sum_lin refuse the table."""
    d = 32
    n_table = (1 << 32) // (d * 4)
    run_big_table(ops, n_table * d, n_table, d, False, False)


def test_unaligned_table_of_exactly_4_gib_takes_the_scalar_general_route(ops):
    """(c) as (b), one float past a 16-byte boundary: the scalar kernels with 64-bit row addresses, d = 32."""
    d = 32
    n_table = (1 << 32) // (d * 4)
    run_big_table(ops, n_table * d, n_table, d, True, False)


# ------------------------------------------------------------------------------------------------ H. non-finite rows
@pytest.mark.parametrize('form', ['ungrouped', 'grouped', 'csr'])
def test_non_finite_table_rows_reach_exactly_their_output_rows(ops, form):
    """+inf, -inf and NaN in one table row each (unweighted sums): IEEE addition carries them to exactly the output rows that
    gather those rows (the hub gathers +inf and -inf: NaN, as in the reference); every other output row keeps the bits of
    the run on the finite table."""
    from tip_amd.plan import build_csr_plan
    d = 20 if form != 'csr' else 12
    c = case(d, 16, False)
    poisoned = c.table.clone()
    poisoned[0], poisoned[c.n_table - 1], poisoned[25] = float('inf'), float('-inf'), float('nan')
    if form == 'csr':
        plan = build_csr_plan(c.out_row.to(DEV), c.table_row.to(DEV), c.n_out, c.n_table)
        run = lambda t: ops.gather_rows_csr(plan, t.to(DEV))
    else:
        plan = c.plan(0 if form == 'ungrouped' else c.G).to(DEV)
        run = lambda t: ops.gather_sum(plan, t.to(DEV))
    clean, got = run(c.table).cpu(), run(poisoned).cpu()
    assert_bits(clean, c.ref(False))
    ref = c.ref(False, table=poisoned)
    hit = torch.zeros(c.n_out, dtype=torch.bool)
    hit[c.out_row[(c.table_row == 0) | (c.table_row == c.n_table - 1) | (c.table_row == 25)]] = True
    assert 0 < int(hit.sum()) < c.n_out and bool((~torch.isfinite(ref[hit])).all()) and bool(torch.isfinite(ref[~hit]).all())
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), 'non-finite pattern differs'
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[torch.isinf(ref)].double(), ref[torch.isinf(ref)])
    assert bool(torch.isnan(ref[c.deg.index(max(c.deg))]).all())            # the hub: +inf + -inf
    assert torch.equal(bits(got[~hit]), bits(clean[~hit]))


# ------------------------------------------------------------------------------------------------ I. normal values
def ulp32(x64):
    return torch.from_numpy(np.spacing(x64.abs().numpy().astype(np.float32)).astype(np.float64))


def check_bound(name, got, ref64, cpu32, mag64):
    """Per element: |got - ref64| <= max(8 x |cpu32 - ref64|, 4 fp32 ulps of mag64) -- both from the CPU, none from `got`."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    cost = (cpu32.detach().double().reshape(ref64.shape) - ref64).abs()
    floor = 4 * ulp32(mag64.reshape(ref64.shape))
    bound = torch.maximum(8 * cost, floor)
    err = (got - ref64).abs()
    used = err / bound
    if os.environ.get('TIPK_ERRLOG'):
        i = int(torch.argmax(used))
        print('ERR %-28s n=%-6d max err=%.3e  worst element: err=%.3e bound=%.3e (8 x fp32 cost %.3e, 4 ulp %.3e) used=%.3f  max|ref|=%.3e'
              % (name, err.numel(), float(err.max()), float(err.view(-1)[i]), float(bound.view(-1)[i]), 8 * float(cost.view(-1)[i]),
                 float(floor.view(-1)[i]), float(used.max()), float(ref64.abs().max())))
    assert bool(torch.isfinite(got).all()), name
    assert float(used.max()) <= 1.0, '%s: %d elements beyond their bound, worst %.3f x' % (name, int((used > 1).sum()), float(used.max()))


@pytest.mark.parametrize('form', ['ungrouped', 'grouped'])
def test_normal_values_gather_sum(ops, form):
    for d in (40, 50):
        c = case(d, 16, True, None, 'normal')
        plan = c.plan(0 if form == 'ungrouped' else c.G).to(DEV)
        assert (plan.n_slots > 0) == (form == 'ungrouped')
        got = ops.gather_sum(plan, c.table.to(DEV))
        check_bound('%s d=%d sum' % (form, d), got, c.ref(False), c.cpu32(False), c.mag(False))
        got = ops.gather_sum(plan, c.table.to(DEV), row_scale=c.scale.to(DEV), bias=c.bias.to(DEV), relu=True)
        check_bound('%s d=%d epilogue' % (form, d), got, c.ref(True), c.cpu32(True), c.mag(True))


def test_normal_values_riders(ops):
    d = 20
    c = case(d, 16, True, None, 'normal')
    plan = c.plan(c.G).to(DEV)
    gate = ladder_gate(c)
    out, parts = ops.gather_sum(plan, c.table.to(DEV), row_scale=c.scale.to(DEV), bias=c.bias.to(DEV), relu=True, gate=gate.to(DEV), colsum=True)
    ref, cpu = c.ref(True, gate=gate), c.cpu32(True, gate=gate)
    check_bound('riders d=%d out' % d, out, ref, cpu, c.mag(True))
    kept = torch.where(gate > 0, c.mag(True), torch.zeros_like(ref))
    check_bound('riders d=%d column sums' % d, parts.sum((0, 1)), ref.sum(0), cpu.sum(0), kept.sum(0))


def test_normal_values_lin(ops):
    d, d2 = 32, 16
    c = case(d, 16, True, None, 'normal')
    g = torch.Generator().manual_seed(9)
    weight, bias2 = torch.randn(d2, d, generator=g), torch.randn(d2, generator=g)
    agg, out2 = ops.gather_sum_lin(c.plan(c.G).to(DEV), c.table.to(DEV), weight.to(DEV), bias2.to(DEV), True, row_scale=c.scale.to(DEV))
    w64 = c.w.double()
    agg64 = C.reference(c.table.double(), c.out_row, c.table_row, c.n_out, w64, c.scale)
    agg32 = C.same_formula_fp32(c.table, c.out_row, c.table_row, c.n_out, c.w, c.scale)
    mag = C.magnitude(c.table.double(), c.out_row, c.table_row, c.n_out, w64, c.scale)
    check_bound('lin agg', agg, agg64, agg32, mag)
    check_bound('lin out2', out2, C.lin_reference(agg64, weight, bias2, True), torch.relu(agg32 @ weight.t() + bias2),
                C.lin_magnitude(mag, weight, bias2))


def test_normal_values_csr(ops):
    from tip_amd.plan import build_csr_plan
    d = 200
    c = case(d, 16, False, None, 'normal')
    plan = build_csr_plan(c.out_row.to(DEV), c.table_row.to(DEV), c.n_out, c.n_table)
    check_bound('csr d=%d' % d, ops.gather_rows_csr(plan, c.table.to(DEV)), c.ref(False), c.cpu32(False), c.mag(False))


# ------------------------------------------------------------------------------------------------ J. through autograd
@pytest.mark.parametrize('n', [300, 1])
@pytest.mark.parametrize('kind', ['aggregate', 'gcn_conv', 'agg_first'])
def test_autograd_entries_on_a_graph_with_deliberate_edges(ops, kind, n):
    """ops.aggregate / gcn_conv / gcn_conv_agg_first (kept rows: the hub, an isolated node, row 0, row n - 1) on a graph with
    isolated nodes, self-loops, duplicate edges and a hub, and on a single node: output and every gradient against fp64
    autograd within the bound of section I; two runs give the same bits."""
    a = C.autograd_case(kind, n)
    graph = ops.AggGraph(a['graph'].fwd.to(DEV), a['graph'].bwd.to(DEV))
    x = a['x'].to(DEV).requires_grad_()
    w = a['wt'].to(DEV).t().requires_grad_()
    b = a['bias'].to(DEV).requires_grad_()
    up = a['up'].to(DEV)
    leaves = [x, b] if kind == 'aggregate' else [x, w, b]
    runs = []
    for rep in range(2):
        for t in leaves:
            t.grad = None
        if kind == 'aggregate':
            out = ops.aggregate(x, graph, bias=b, relu=True)
        elif kind == 'gcn_conv':
            out = ops.gcn_conv(x, w, b, graph, relu=True)
        else:
            out = ops.gcn_conv_agg_first(x, w, b, graph, relu=True)
        out.backward(up)
        runs.append([out.detach().clone()] + [t.grad.clone() for t in leaves])
    for p, q in zip(*runs):
        assert torch.equal(bits(p), bits(q))
    ref = C.conv_reference(kind, a['x'], None if kind == 'aggregate' else a['wt'].t(), a['bias'], a['up'], *a['edges'])
    names = ['out', 'd_x', 'd_bias'] if kind == 'aggregate' else ['out', 'd_x', 'd_weight', 'd_bias']
    for name, got in zip(names, runs[0]):
        r64, c32, mag = ref[name]
        check_bound('%s n=%d %s' % (kind, n, name), got, r64, c32, mag)
