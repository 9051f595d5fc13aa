"""The two refinements of `tipk_gemm_wg_group` (tip_amd/csrc/tipk_gemm.hip) pinned against fp64 where they can go wrong: the
16 x 16 body a job takes when 4 mt nt batch <= 128 (mt, nt: its 32 x 32 tiles), and two batch terms of k <= 16 sharing one K tile
on the 16-byte path.  Cases, operand placement (NaN guards around every input, sentinels around every output), references and
the bound are those of `tests/dense_cases.py`: per element |kernel - fp64| <= kr * 2^-24 * Abs with kr = the reduction length
+ 16 wave partials + 3 (`WgCase.kr`).  Neither body nor packing is observable from outside: the shapes below are chosen so that
the rule written in the kernel's host code sends them where the case's name says.  Integer data must come out EQUAL to fp64,
closed gates (NaN, -0, negative) as exact zeros, and every launch is repeated and compared bit for bit."""
import pytest
import torch

import dense_cases as D
from tip_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
QUARTER_MAX = 128                                          # WGK_QUARTER_MAX of the kernel


def _case(cid, m, n, k, la='r', lb='c', z=1, reduce=False, k2=0, **kw):
    n_kt = (z if reduce else 1) * -(-k // 32) + -(-k2 // 32)
    assert n_kt <= 64
    return D.WgCase(cid, m, n, k, la, lb, n_kt, z=z, reduce=reduce, k2=k2, **kw)


def _quarter(case):
    """What the kernel's rule says for the case: True = 16 x 16 tiles."""
    return 4 * -(-case.m // 32) * -(-case.n // 32) * (1 if (case.reduce or case.z == 1) else case.z) <= QUARTER_MAX


def _check(t, name=None):
    case = t.case
    torch.cuda.synchronize()
    _, _, so = case.shapes()
    assert D.guards_intact(t.big_o, so, case.lo, D.SENT), 'a write outside the output view'
    assert D.wg_inputs_intact(t), 'an input or a guard around it changed'
    want, mag = case.reference()
    r = D.ratio(t.out, want, mag)
    print('RATIO %s %.3f (kr = %d, used = %.4f)' % (name or case.cid, r, case.kr, r / case.kr))
    assert r / case.kr <= 1.0, (name or case.cid, r, case.kr)
    if case.integer:
        assert torch.equal(t.out.cpu().double(), want), 'integer data must come out exact'
    if case.gate:
        closed = ~(case.values()['gate'] > 0)
        assert bool((t.out.cpu()[closed] == 0).all()), 'NaN, -0 and negative gates are closed'


def _run(case, quarter=None):
    """Launch the case alone, twice; -> the built case of the first launch."""
    if quarter is not None:
        assert _quarter(case) == quarter, case.cid
    t, u = D.build_wg(case, DEV), D.build_wg(case, DEV)
    assert t.job is not None and u.job is not None
    ops.wg_gemm_group([t.job])
    ops.wg_gemm_group([u.job])
    _check(t)
    assert torch.equal(t.out, u.out), 'not repeatable bit for bit'
    return t


EDGES = (1, 15, 16, 17, 33)


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('m', EDGES)
def test_quarter_tile_edges(m, integer):
    """Every (m, n) around the 16 x 16 tile edge, 16-byte first product (k = 40: a K tile of 8 valid terms) + dword second product,
    full epilogue; the output view is a column slice (from column 5) or has an odd leading dimension."""
    for n in EDGES:
        _run(_case('qt_edge_m%d_n%d_%d' % (m, n, integer), m, n, 40, k2=5, la2='c', lb2='r', cin='ro', relu=(m + n) % 3 == 0,
                   gate=True, alpha=-0.75, lo='ro' if (m + n) % 2 else 'r1', integer=integer), quarter=True)


# (m, n): 33 x 17 is four + two 16 x 16 tiles; 225 x 193 is 8 x 7 tiles of 32 x 32 (224 > 128: the 32 x 32 body)
BODIES = {'quarter': (33, 17), 'full': (225, 193)}
PACKED = [(16, z, k2) for z in (1, 2, 3, 32) for k2 in (0, 16, 32, 36)] + [(12, 3, 0), (12, 2, 16), (4, 5, 0)]


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('k,z,k2', PACKED, ids=['k%d_z%d_k2_%d' % p for p in PACKED])
@pytest.mark.parametrize('body', sorted(BODIES))
def test_packed_k(body, k, z, k2, integer):
    """Batch terms of k <= 16 on the 16-byte path: one term (nothing to pack), an even and an odd count (the last tile's upper
    half is masked) and 32 terms, k = 12 and 4 (part of each half masked), alone and with a second product of 1 or 2 K tiles."""
    m, n = BODIES[body]
    _run(_case('pack_%s_k%d_z%d_k2_%d_%d' % (body, k, z, k2, integer), m, n, k, z=z, reduce=z > 1, k2=k2, gate=True, alpha=0.5,
               integer=integer), quarter=body == 'quarter')


UNPACKED = [('k20', dict(k=20)), ('b_not_k_contiguous', dict(k=16, lb='r')), ('a_not_k_contiguous', dict(k=16, la='c')),
            ('a_misaligned', dict(k=16, la='r1')), ('a_odd_ld', dict(k=16, la='ro'))]


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('name,kw', UNPACKED, ids=[u[0] for u in UNPACKED])
@pytest.mark.parametrize('body', sorted(BODIES))
def test_narrow_k_that_must_not_pack(body, name, kw, integer):
    """k = 20 spans more than half a K tile; an operand that is not contiguous in k, or not 16-byte aligned, is read dword by
    dword: three batch terms stay three K tiles."""
    m, n = BODIES[body]
    _run(_case('nopack_%s_%s_%d' % (body, name, integer), m, n, z=3, reduce=True, k2=16, cin='r1', integer=integer, **kw),
         quarter=body == 'quarter')


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('z', (32, 33))
def test_both_bodies_on_one_shape(z, integer):
    """17 x 17 outputs in a batch of 32 (4 x 32 = 128: 16 x 16 tiles) and of 33 (132: 32 x 32 tiles); alpha, c_in, ReLU, gate."""
    _run(_case('bodies_z%d_%d' % (z, integer), 17, 17, 36, z=z, cin='r1', relu=True, gate=True, alpha=2.0, lo='ro',
               integer=integer), quarter=z == 32)


def test_group_equals_alone():
    """A 16 x 16 job with packed K, a 32 x 32 job and a riding slab sum in one launch: each equals its launch alone."""
    cases = [_case('grp_quarter', 33, 17, 16, z=3, reduce=True, k2=36, gate=True),
             _case('grp_full', 225, 193, 40, cin='ro', relu=True, alpha=-0.75),
             _case('grp_quarter_scalar', 17, 33, 37, la='c', lb='r', k2=5)]
    assert [_quarter(c) for c in cases] == [True, False, True]
    together, alone = [D.build_wg(c, DEV) for c in cases], [D.build_wg(c, DEV) for c in cases]
    g = D._gen('tail_rider')
    slabs, addend = torch.randn(5, 40, 48, generator=g).to(DEV), torch.randn(40, 48, generator=g).to(DEV)
    rider = ops.slab_job(slabs, alpha=0.5, addend=addend, relu=True)
    ops.wg_gemm_group([t.job for t in together], [rider])
    for u in alone:
        ops.wg_gemm_group([u.job])
    for t, u in zip(together, alone):
        _check(t, t.case.cid + '[group]')
        assert torch.equal(t.out, u.out), t.case.cid
    assert torch.equal(rider.out, ops.sum_slabs(slabs, alpha=0.5, addend=addend, relu=True))


@pytest.mark.parametrize('gated', (False, True), ids=('plain', 'gate_x'))
@pytest.mark.parametrize('d_in,d_out', ((64, 32), (32, 16)))
def test_dense_tail_end_to_end(d_in, d_out, gated):
    """`ops.rgcn_dense_tail` at 70 nodes, 4 bases against fp64: dX (packed K at d_out = 16), d basis and d root, all on 16 x 16
    tiles.  Gradient tolerance of DESIGN.md section 9, its absolute part at the tighter 1e-5 max|want|."""
    n, nb = 70, 4
    g = D._gen('tail_%d_%d' % (d_in, d_out))
    x, gr, g_xb = torch.randn(n, d_in, generator=g), torch.randn(n, d_out, generator=g), torch.randn(nb, n, d_out, generator=g)
    basis, root = torch.randn(nb, d_in, d_out, generator=g), torch.randn(d_in, d_out, generator=g)
    dev = lambda *ts: [t.to(DEV) for t in ts]
    xd, grd, g_xbd, basisd, rootd = dev(x, gr, g_xb, basis, root)
    got = [o.cpu() for o in ops.rgcn_dense_tail(xd, basisd, rootd, grd, g_xbd, xd if gated else None, [])]
    again = [o.cpu() for o in ops.rgcn_dense_tail(xd, basisd, rootd, grd, g_xbd, xd if gated else None, [])]
    f = lambda t: t.double()
    want_x = torch.matmul(f(g_xb), f(basis).transpose(1, 2)).sum(0) + f(gr) @ f(root).t()
    if gated:
        want_x = want_x * (x > 0)
    want = [want_x, torch.matmul(f(x).t(), f(g_xb)), f(x).t() @ f(gr)]
    for name, o, o2, w in zip(('dX', 'd basis', 'd root'), got, again, want):
        assert o.shape == w.shape, name
        top = float(w.abs().max())
        err = float((o.double() - w).abs().max())
        print('TAIL %s in %d out %d: max err %.3g = %.3g max|want|' % (name, d_in, d_out, err, err / top))
        torch.testing.assert_close(o.double(), w, rtol=1e-4, atol=1e-5 * top, msg=name)
        assert torch.equal(o, o2), name
    if gated:
        assert bool((got[0][~(x > 0)] == 0).all())
