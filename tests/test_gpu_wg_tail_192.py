"""The edge of the tile rule of `tipk_gemm_wg_group` (tip_amd/csrc/tipk_gemm.hip) where it stands now: a job takes the 16 x 16
body when 4 mt nt batch <= 192 (mt, nt: its 32 x 32 tiles), so that dX of the first R-GCN layer (645 x 64: 168) runs on quarter
tiles with packed K, and the 32 x 32 body above.  `tests/test_gpu_wg_tail_tiles.py` was written when the constant was 128 and
says so in its docstring and its `QUARTER_MAX`; that is history -- its bound does not depend on the body, and it passes unchanged.

In its manner, with the cases, operand placement (NaN guards, sentinels), references and the bound of `tests/dense_cases.py`: per
element |kernel - fp64| <= kr * 2^-24 * Abs, kr = the reduction length + 16 wave partials + 3 (`WgCase.kr`); integer data equal
to fp64; closed gates exact zeros; every launch made twice.  The body is not observable from outside: the shapes sit on both
sides of the edge as the rule in the kernel's host code counts them --

    17 x 17 (1 x 1 tiles) in batches of 48 and 49:   192 and 196
    65 x 33 (3 x 2 tiles) in batches of 8 and 9:     192 and 216
    129 x 65 (5 x 3 tiles) in batches of 3 and 4:    180 and 240

-- alone and in one launch with other products: the rule is a function of the job's shape alone, so a job's bits must not depend
on its neighbours."""
import pytest
import torch

import dense_cases as D
from tip_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
QUARTER_MAX = 192                                          # WGK_QUARTER_MAX of the kernel

# (m, n, batch below or on the edge, batch above it)
EDGE = [(17, 17, 48, 49), (65, 33, 8, 9), (129, 65, 3, 4)]


def _case(cid, m, n, k, z, integer, reduce=False, k2=0, **kw):
    n_kt = (z if reduce else 1) * -(-k // 32) + -(-k2 // 32)
    assert n_kt <= 64
    return D.WgCase(cid, m, n, k, 'r', 'c', n_kt, z=z, reduce=reduce, k2=k2, integer=integer, **kw)


def _count(case):
    """4 mt nt batch, as the kernel's rule counts it."""
    return 4 * -(-case.m // 32) * -(-case.n // 32) * (1 if case.reduce else case.z)


def _check(t, name):
    case = t.case
    torch.cuda.synchronize()
    _, _, so = case.shapes()
    assert D.guards_intact(t.big_o, so, case.lo, D.SENT), 'a write outside the output view'
    assert D.wg_inputs_intact(t), 'an input or a guard around it changed'
    want, mag = case.reference()
    r = D.ratio(t.out, want, mag)
    print('RATIO %s %.3f (kr = %d, used = %.4f)' % (name, r, case.kr, r / case.kr))
    assert r / case.kr <= 1.0, (name, r, case.kr)
    if case.integer:
        assert torch.equal(t.out.cpu().double(), want), 'integer data must come out exact'
    if case.gate:
        closed = ~(case.values()['gate'] > 0)
        assert bool((t.out.cpu()[closed] == 0).all()), 'NaN, -0 and negative gates are closed'


def _edge_cases(m, n, z_in, z_out, integer):
    kw = dict(cin='r1', relu=True, gate=True, alpha=2.0, lo='ro')
    below = _case('t192_%dx%d_z%d_%d' % (m, n, z_in, integer), m, n, 36, z_in, integer, **kw)
    above = _case('t192_%dx%d_z%d_%d' % (m, n, z_out, integer), m, n, 36, z_out, integer, **kw)
    assert _count(below) <= QUARTER_MAX < _count(above) and _count(below) > 128
    return below, above


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('m,n,z_in,z_out', EDGE, ids=['%dx%d' % e[:2] for e in EDGE])
def test_both_sides_of_the_edge_alone(m, n, z_in, z_out, integer):
    for case in _edge_cases(m, n, z_in, z_out, integer):
        t, u = D.build_wg(case, DEV), D.build_wg(case, DEV)
        assert t.job is not None and u.job is not None
        ops.wg_gemm_group([t.job])
        ops.wg_gemm_group([u.job])
        _check(t, case.cid)
        assert torch.equal(t.out, u.out), 'not repeatable bit for bit'


@pytest.mark.parametrize('integer', (False, True), ids=('float', 'integer'))
@pytest.mark.parametrize('m,n,z_in,z_out', EDGE, ids=['%dx%d' % e[:2] for e in EDGE])
def test_group_equals_alone(m, n, z_in, z_out, integer):
    """Both sides of the edge in ONE launch, between a small 16 x 16 job with packed K and a 32 x 32 job: each equals its launch
    alone."""
    below, above = _edge_cases(m, n, z_in, z_out, integer)
    cases = [_case('t192_grp_quarter_%d' % integer, 33, 17, 16, 3, integer, reduce=True, k2=36, gate=True), below, above,
             _case('t192_grp_full_%d' % integer, 225, 193, 40, 1, integer, cin='ro', relu=True, alpha=-0.75)]
    assert [_count(c) <= QUARTER_MAX for c in cases[1:]] == [True, False, False]
    together, alone = [D.build_wg(c, DEV) for c in cases], [D.build_wg(c, DEV) for c in cases]
    ops.wg_gemm_group([t.job for t in together])
    for u in alone:
        ops.wg_gemm_group([u.job])
    for t, u in zip(together, alone):
        _check(t, t.case.cid + '[group]')
        assert torch.equal(t.out, u.out), t.case.cid
