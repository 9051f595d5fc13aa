"""The dense family on the device, pinned against fp64 at the edges of every route (`tests/dense_cases.py`): each product is checked
to take the body written next to it BEFORE it is launched, its result stays within kr * 2^-24 * Abs of the fp64 reference in every
element, integer data comes out exact, the non-finite pattern is the reference's, the sentinels around every output and the NaN
guards around every input survive, split products leave no slab unwritten, and what include/tipk.h calls bit-identical is compared
with torch.equal.  Every comparison prints

    RATIO <case> <max |kernel - fp64| / (2^-24 Abs)> (kr = <roundings>, used = <ratio / kr>)

(`-s`; profiles/dense_routes_errors.md) and asserts used <= 1."""
import pytest
import torch

import dense_cases as D
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _options_restored():
    """A failing test must not leak "gemm_stream_kk" (or the other two) into the tests that follow."""
    before = {name: _lib.get_option(name) for name in D.OPTIONS}
    yield
    for name, value in before.items():
        _lib.set_option(name, value)


def _report(name, got, want, mag, kr):
    r = D.ratio(got, want, mag)
    used = r / kr
    print('RATIO %s %.3f (kr = %d, used = %.4f)' % (name, r, kr, used))
    assert used <= 1.0, (name, r, kr)
    return used


def _launch(t):
    """The two calls of `ops.gemm` (tip_amd/ops.py: tipk_gemm_f32, then tipk_sum_slabs for a split product), copied from there
    so that the slab buffer can be poisoned in between job and launch: an unwritten slab shows as NaN.  (`ops.gemm_group([job])`
    is the grouped launch -- another route -- and gets its own comparison.)"""
    job, L = t.job, _lib.lib()
    st = _lib.stream_ptr(job.out.device)
    if job.slabs is not None:
        job.slabs.fill_(D.NAN)
    _lib.check(L.tipk_gemm_f32(job.desc, st), 'tipk_gemm_f32')
    if job.slabs is not None:
        _lib.check(L.tipk_sum_slabs(_lib.ptr(job.slabs), job.n_slabs, job.per, job.per, job.alpha, int(job.accumulate),
                                    _lib.ptr(job.out), st), 'tipk_sum_slabs')


def _launch_grouped(ts):
    for t in ts:
        if t.job.slabs is not None:
            t.job.slabs.fill_(D.NAN)
    ops.gemm_group([t.job for t in ts])


def _route(t, grouped):
    return _lib.lib().tipk_gemm_route(t.job.desc, int(grouped))


def _check_gemm(t, name=None):
    case = t.case
    torch.cuda.synchronize()
    _, _, so = case.shapes()
    assert D.guards_intact(t.big_o, so, case.lo, D.SENT), 'a write outside the output view'
    assert D.inputs_intact(t), 'an input or a guard around it changed'
    if t.job.slabs is not None:
        slabs = t.job.slabs.cpu()
        assert not bool(torch.isnan(slabs).any()), 'a slab was left unwritten'
        if not case.reduce:                                                   # split K: slabs past the end of k hold zeros
            chunk = -(-(-(-case.k // t.job.n_slabs)) // 32) * 32 or 32
            for s in range(t.job.n_slabs):
                if s * chunk >= case.k:
                    assert bool((slabs[s] == 0).all()), 'empty slab %d is not zero' % s
    if case.m == 0:
        return
    want, mag = case.reference()
    _report(name or case.cid, t.out, want, mag, t.kr)
    if case.integer:
        assert torch.equal(t.out.cpu().double(), want), 'integer data must come out exact'
    if case.inf:
        bad = ~torch.isfinite(t.out.cpu())
        expect = torch.zeros_like(bad)
        expect[case.m // 2, :] = True
        expect[:, case.n // 3] = True
        assert torch.equal(bad, expect), 'exactly the row of the +inf in a and the column of the +inf in b are non-finite'


# ------------------------------------------------------------------------------------------------ tipk_gemm_f32
@pytest.mark.parametrize('case', D.GEMM_CASES, ids=lambda c: c.cid)
def test_gemm_case(case):
    t = D.build_gemm(case, DEV)
    with D.options(**case.opts):
        got = _route(t, 0)
        assert got == case.code, 'route %s, written down: %s' % (D.route_name(got), D.route_name(case.code))
        _launch(t)
    _check_gemm(t)
    if t.job.slabs is not None:
        # the split product as a member of a grouped launch (+ grouped slab sum): bit-identical
        t2 = D.build_gemm(case, DEV)
        with D.options(**case.opts):
            _launch_grouped([t2])
        _check_gemm(t2, case.cid + '[grouped]')
        assert torch.equal(t2.out, t.out)


def test_empty_k_through_ops_gemm():
    """k == 0 is an empty sum (include/tipk.h section 2): zeros, or relu?(c_in) -- torch hands empty operands over as NULL."""
    a, b = torch.zeros(256, 0, device=DEV), torch.zeros(0, 4096, device=DEV)
    out = ops.gemm(a, b)
    assert out.shape == (256, 4096) and bool((out == 0).all())
    out = ops.gemm(a, b, ksplit=3)
    assert bool((out == 0).all())
    c = torch.randn(256, 4096, device=DEV)
    assert torch.equal(ops.gemm(a, b, c_in=c, relu=True, alpha=3.0), torch.relu(c))
    assert torch.equal(ops.gemm(torch.zeros(2, 40, 0, device=DEV), torch.zeros(2, 0, 24, device=DEV)), torch.zeros(2, 40, 24, device=DEV))


@pytest.mark.parametrize('cid,other', D.BIT_IDENTICAL, ids=[c for c, _ in D.BIT_IDENTICAL])
def test_streamed_equals_tiled_bit_for_bit(cid, other):
    case = D.gemm_case(cid)
    t, u = D.build_gemm(case, DEV), D.build_gemm(case, DEV)
    with D.options(**case.opts):
        assert _route(t, 0) == case.code
        _launch(t)
    with D.options(**other):
        assert D.route_name(_route(u, 0)).startswith('t'), 'the cross-check must run the LDS-tiled kernel'
        _launch(u)
    torch.cuda.synchronize()
    assert torch.equal(t.out, u.out)
    if t.job.slabs is not None:
        assert torch.equal(t.job.slabs, u.job.slabs)


# ------------------------------------------------------------------------------------------------ tipk_gemm_f32_group
def test_grouped_launch_members_equal_single_launches():
    opts = D.GROUP_CASES[0].opts
    assert all(c.opts == opts for c in D.GROUP_CASES) and len(D.GROUP_CASES) == _lib.GROUP_MAX
    members = [D.build_gemm(c, DEV) for c in D.GROUP_CASES]
    singles = [D.build_gemm(c, DEV) for c in D.GROUP_CASES]
    with D.options(**opts):
        for t in members:
            got = _route(t, 1)
            assert got == t.case.code, '%s: route %s, written down: %s' % (t.case.cid, D.route_name(got), D.route_name(t.case.code))
        assert [t.case.m for t in members].index(0) not in (0, len(members) - 1), 'the empty member sits in the middle'
        _launch_grouped(members)
        for u in singles:
            _launch(u)
    for t, u in zip(members, singles):
        _check_gemm(t)
        assert torch.equal(t.out, u.out), t.case.cid
        if t.job.slabs is not None:
            assert torch.equal(t.job.slabs, u.job.slabs), t.case.cid


@pytest.mark.parametrize('case', D.GROUP_SINGLES, ids=lambda c: c.cid)
def test_grouped_member_alone(case):
    t, u = D.build_gemm(case, DEV), D.build_gemm(case, DEV)
    assert _route(t, 1) == case.code
    _launch_grouped([t])
    _check_gemm(t)
    # a single launch would stream a thin-k shape through thin_k4, which pairs k differently: the narrow body keeps the tiled order
    with D.options(gemm_thin_k_narrow=1):
        _launch(u)
    torch.cuda.synchronize()
    assert torch.equal(t.out, u.out)


# ------------------------------------------------------------------------------------------------ tipk_gemm_wg_group
def _check_wg(t, name=None):
    case = t.case
    torch.cuda.synchronize()
    _, _, so = case.shapes()
    assert D.guards_intact(t.big_o, so, case.lo, D.SENT), 'a write outside the output view'
    assert D.wg_inputs_intact(t), 'an input or a guard around it changed'
    want, mag = case.reference()
    _report(name or case.cid, t.out, want, mag, case.kr)
    if case.integer:
        assert torch.equal(t.out.cpu().double(), want)
    if case.gate:
        closed = ~(case.values()['gate'] > 0)
        assert bool((t.out.cpu()[closed] == 0).all()), 'NaN, -0 and negative gates are closed'


@pytest.mark.parametrize('case', D.WG_CASES, ids=lambda c: c.cid)
def test_workgroup_split_case(case):
    t = D.build_wg(case, DEV)
    assert (t.job is not None) == case.supported
    if t.job is None:
        return
    ops.wg_gemm_group([t.job])
    _check_wg(t)


def test_workgroup_split_four_products_three_sums():
    """The full launch: 4 products + 3 riding slab sums, the middle one empty.  Every member equals its launch alone."""
    cids = ['wg_m33_n31_kt17_vec_tail4', 'wg_epilogue', 'wg_batch3', 'wg_second_scalar']
    together = [D.build_wg(D.wg_case(c), DEV) for c in cids]
    alone = [D.build_wg(D.wg_case(c), DEV) for c in cids]
    g = D._gen('riders')
    sums, outs = [], []
    for rows, cols, n_slabs in ((40, 48, 5), (0, 8, 3), (1024, 8, 9)):         # dword | empty | 16-byte path (8192 elements)
        slabs = torch.randn(n_slabs, rows, cols, generator=g).to(DEV)
        addend = torch.randn(rows, cols, generator=g).to(DEV)
        sums.append(ops.slab_job(slabs, alpha=0.5, addend=addend, relu=True))
        outs.append(ops.sum_slabs(slabs, alpha=0.5, addend=addend, relu=True) if rows else None)
    ops.wg_gemm_group([t.job for t in together], sums)
    for u in alone:
        ops.wg_gemm_group([u.job])
    for t, u in zip(together, alone):
        _check_wg(t, t.case.cid + '[4+3]')
        assert torch.equal(t.out, u.out)
    for s, o in zip(sums, outs):
        if o is not None:
            assert torch.equal(s.out, o), 'a riding slab sum equals tipk_sum_slabs_ex'


# ------------------------------------------------------------------------------------------------ slab sums
class _Slabs(object):
    """One slab sum on the device: slabs [n_slabs][count] as rows of a NaN-guarded buffer (slab_stride = its leading dimension),
    addend / gate / row_scale in guarded buffers of their own, out inside a sentinel-filled one."""

    def __init__(self, n_slabs, rows, cols, epi, cid, lay_in='r', lay_add='r', lay_out='r', integer=False):
        self.epi, self.rows, self.cols, self.count, self.n = epi, rows, cols, rows * cols, n_slabs
        self.v = D.slab_values(n_slabs, rows, cols, epi, cid, integer)
        flat = lambda t: None if t is None else t.reshape(-1, self.count) if t.dim() == 3 else t.reshape(1, -1)
        self.lay_in, self.lay_add, self.lay_out = lay_in, lay_add, lay_out
        self.big_in, self.slabs = D.place(flat(self.v['slabs']), lay_in, D.NAN, DEV)
        self.stride = self.big_in.stride(0)
        self.big_add, self.addend = D.place(flat(self.v['addend']), lay_add, D.NAN, DEV) if epi.get('addend') else (None, None)
        self.big_gate, self.gate = D.place(flat(self.v['gate']), 'r', D.NAN, DEV) if epi.get('gate') else (None, None)
        self.rs = self.v['row_scale'].to(DEV) if epi.get('row_scale') else None
        self.big_out, self.out = D.place(flat(self.v['prev']), lay_out, D.SENT, DEV, shape=[1, self.count])

    def _in_ptr(self):
        return _lib.ptr(self.slabs) if self.n else None

    def run_ex(self):
        e = self.epi
        assert not e.get('gate')
        _lib.check(_lib.lib().tipk_sum_slabs_ex(self._in_ptr(), self.n, self.stride, self.count, e.get('alpha', 1.0),
                                                int(bool(e.get('accumulate'))), _lib.ptr(self.rs), self.cols, _lib.ptr(self.addend),
                                                int(bool(e.get('relu'))), _lib.ptr(self.out), _lib.stream_ptr(self.out.device)),
                   'tipk_sum_slabs_ex')

    def desc(self):
        e, d = self.epi, _lib.SlabSumDesc()
        d.in_, d.n_slabs, d.slab_stride, d.count = (self.slabs.data_ptr() if self.n else None), self.n, self.stride, self.count
        d.alpha, d.accumulate = e.get('alpha', 1.0), int(bool(e.get('accumulate')))
        d.row_scale, d.cols = (self.rs.data_ptr() if self.rs is not None else None), self.cols
        d.addend = self.addend.data_ptr() if self.addend is not None else None
        d.relu, d.out = int(bool(e.get('relu'))), self.out.data_ptr()
        d.gate = self.gate.data_ptr() if self.gate is not None else None
        return d

    def check(self, name):
        torch.cuda.synchronize()
        assert D.guards_intact(self.big_out, [1, self.count], self.lay_out, D.SENT), 'a write outside the output'
        assert D.guards_intact(self.big_in, [self.n, self.count], self.lay_in, D.NAN)
        want, mag, kr = D.slab_reference(self.v, self.epi)
        _report(name, self.out.reshape(self.rows, self.cols), want, mag, kr)
        if self.gate is not None:
            closed = ~(self.v['gate'] > 0)
            assert bool((self.out.cpu().reshape(self.rows, self.cols)[closed] == 0).all())


def _run_group(items):
    arr = (_lib.SlabSumDesc * len(items))(*[s.desc() for s in items])
    _lib.check(_lib.lib().tipk_sum_slabs_group(arr, len(items), _lib.stream_ptr(items[0].out.device)), 'tipk_sum_slabs_group')


_SHAPE_OF = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13)}
_PLAIN = [e for e in D.EPILOGUES if not e.get('gate')]


@pytest.mark.parametrize('count', D.SLAB_ELEMS)
def test_slab_sums_small(count):
    """n_slabs over its edges (0, the 4-load unroll, the 4 / 16 lane switch at 32, 65) x every epilogue without a gate through
    tipk_sum_slabs_ex; the grouped launch gives the same bits and applies the gate."""
    rows, cols = _SHAPE_OF[count]
    for i, n_slabs in enumerate(D.SLAB_COUNTS):
        for j in ({i % len(_PLAIN), (i + 3) % len(_PLAIN), len(_PLAIN) - 1}):
            epi = _PLAIN[j]
            name = 'slabs_%dx%d_epi%d' % (n_slabs, count, j)
            one = _Slabs(n_slabs, rows, cols, epi, name)
            one.run_ex()
            one.check(name)
            grouped = _Slabs(n_slabs, rows, cols, epi, name, lay_in='ro', lay_out='r1')
            gated = _Slabs(n_slabs, rows, cols, D.EPILOGUES[-1 - (i % 2)], name + 'g')
            _run_group([grouped, gated])
            gated.check(name + '[gate]')
            torch.cuda.synchronize()
            assert torch.equal(grouped.out, one.out), name
    exact = _Slabs(33, rows, cols, dict(alpha=2.0, addend=True, accumulate=True, relu=True), 'slabs_int%d' % count, integer=True)
    exact.run_ex()
    torch.cuda.synchronize()
    assert torch.equal(exact.out.cpu().reshape(rows, cols).double(), D.slab_reference(exact.v, exact.epi)[0])


@pytest.mark.parametrize('n_slabs,count', D.LANE_SWITCH)
def test_slab_sum_lane_switch(n_slabs, count):
    """32 slabs: 16 slab lanes below 2048 workgroups of 64 elements, 4 from 2048 on -- single and grouped launch switch together."""
    epi = dict(alpha=0.5, row_scale=True, addend=True, relu=True)
    one = _Slabs(n_slabs, count // 64, 64, epi, 'lane_switch')
    one.run_ex()
    one.check('slabs_%dx%d' % (n_slabs, count))
    vec, dword = _Slabs(n_slabs, count // 64, 64, epi, 'lane_switch'), _Slabs(n_slabs, count // 64, 64, epi, 'lane_switch', lay_add='r1')
    _run_group([vec, dword])
    torch.cuda.synchronize()
    assert torch.equal(vec.out, one.out) and torch.equal(dword.out, one.out)


@pytest.mark.parametrize('epi', range(len(D.EPILOGUES)))
@pytest.mark.parametrize('count', D.GROUP_ELEMS)
def test_grouped_slab_sum_paths(count, epi):
    """Grouped sums take 16-byte accesses from 4096 elements (count % 4 == 0, aligned operands); 4092 elements, a misaligned
    addend (or, without an addend, a misaligned output) take the dword path.  Both give the bits of tipk_sum_slabs_ex,
    with no slab at all too."""
    epi = D.EPILOGUES[epi]
    rows, cols = count // 4, 4
    for n_slabs in (0, 3, 8, 9, 31):
        name = 'gslabs_%dx%d' % (n_slabs, count)
        vec = _Slabs(n_slabs, rows, cols, epi, name)
        off = _Slabs(n_slabs, rows, cols, epi, name, lay_add='r1') if epi.get('addend') else _Slabs(n_slabs, rows, cols, epi, name, lay_out='r1')
        _run_group([vec, off])
        vec.check(name + '[16-byte]' if count >= 4096 else name)
        off.check(name + '[dword]')
        assert torch.equal(vec.out, off.out)
        if not epi.get('gate'):
            one = _Slabs(n_slabs, rows, cols, epi, name)
            one.run_ex()
            torch.cuda.synchronize()
            assert torch.equal(vec.out, one.out)


# ------------------------------------------------------------------------------------------------ row-wise glue
def test_transpose_tile_edges():
    g = D._gen('transpose')
    for rows in D.TRANSPOSE_SIZES:
        for cols in D.TRANSPOSE_SIZES:
            x = torch.randn(rows, cols, generator=g)
            x.view(-1)[::7] = D.NAN
            got = ops.transpose(x.to(DEV))
            assert got.shape == (cols, rows) and got.is_contiguous()
            assert torch.equal(got.cpu().nan_to_num(5.0), x.t().contiguous().nan_to_num(5.0)), (rows, cols)


@pytest.mark.parametrize('case', D.AFFINE_CASES, ids=lambda c: '%dx%d' % (c[0], c[1]))
def test_rows_affine(case):
    rows, cols, lx, lg, lo, mul, div, gate, acc = case
    g = D._gen('affine%dx%d' % (rows, cols))
    x, prev = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    rm = torch.randn(rows, generator=g) if mul else None
    rd = (torch.rand(rows, generator=g) + 0.5) * (torch.randint(0, 2, (rows,), generator=g) * 2 - 1).float() if div else None
    gt = D.gate_values([rows, cols], g) if gate else None
    big_x, vx = D.place(x, lx, D.NAN, DEV)
    big_g, vg = D.place(gt, lg, D.NAN, DEV) if gate else (None, None)
    big_o, vo = D.place(prev if acc else None, lo, D.SENT, DEV, shape=[rows, cols])
    dev = lambda t: None if t is None else t.to(DEV)
    ops.rows_affine(vx, dev(rm), dev(rd), vg, out=vo, accumulate=acc)
    torch.cuda.synchronize()
    assert D.guards_intact(big_o, [rows, cols], lo, D.SENT) and D.guards_intact(big_x, [rows, cols], lx, D.NAN)
    out = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        v = f(x)
        if mul:
            v = v * f(rm).view(-1, 1)
        if div:
            v = v / f(rd).view(-1, 1)
        if gate:
            v = v * (gt > 0)
        out.append(v + f(prev) if acc else v)
    _report('rows_affine_%dx%d' % (rows, cols), vo, out[0], out[1], 3)         # the product, the quotient, the sum
    if gate:
        closed = ~(gt > 0)
        want_closed = prev[closed] if acc else torch.zeros(int(closed.sum()))
        assert torch.equal(vo.cpu()[closed], want_closed), 'NaN, -0 and negative gates are closed'
    if not (mul or div):
        assert torch.equal(vo.cpu().double(), out[0].float().double() if acc else out[0])


@pytest.mark.parametrize('cols', D.COLSUM_COLS)
def test_col_sum(cols):
    g = D._gen('colsum%d' % cols)
    for rows in D.col_sum_rows(cols):
        x = torch.randn(rows, cols, generator=g)
        big, view = D.place(x, 'r', D.NAN, DEV)                               # a column slice of a wider matrix
        got = ops.col_sum(view)
        torch.cuda.synchronize()
        assert got.shape == (cols,) and D.guards_intact(big, [rows, cols], 'r', D.NAN)
        if rows == 0:
            assert bool((got == 0).all())
            continue
        _report('col_sum_%dx%d' % (rows, cols), got, x.double().sum(0), x.double().abs().sum(0), rows)
        xi = torch.randint(-4, 5, (rows, cols), generator=g).float()
        assert torch.equal(ops.col_sum(D.place(xi, 'ro', D.NAN, DEV)[1]).cpu().double(), xi.double().sum(0))


@pytest.mark.parametrize('cols', D.GATE_COLSUM_COLS)
def test_gate_colsum(cols):
    g = D._gen('gate_colsum%d' % cols)
    for rows in D.gate_colsum_rows(cols):
        x, gt = torch.randn(rows, cols, generator=g), D.gate_values([rows, cols], g)
        big_x, vx = D.place(x, 'ro', D.NAN, DEV)
        big_g, vg = D.place(gt, 'r1', D.NAN, DEV)
        out, scratch = ops.gate_colsum(vx, vg)
        torch.cuda.synchronize()
        assert D.guards_intact(big_x, [rows, cols], 'ro', D.NAN) and D.guards_intact(big_g, [rows, cols], 'r1', D.NAN)
        groups = int(_lib.lib().tipk_gate_colsum_groups(rows, cols))
        assert scratch.shape == (groups, 1, cols) and groups == (1 if rows == 1 else 256)
        want = x * (gt > 0)
        assert torch.equal(out.cpu(), want), 'out = x * (gate > 0), bit for bit'
        _report('gate_colsum_%dx%d' % (rows, cols), scratch.cpu().double().sum(0).view(-1), want.double().sum(0),
                x.double().abs().sum(0), rows)


def test_gate_colsum_refuses_257_columns():
    x = torch.randn(3, 257, device=DEV)
    assert ops.gate_colsum(x, x) is None
