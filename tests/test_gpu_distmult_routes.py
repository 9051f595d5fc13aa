"""The DistMult decoder outside its fused fast path against fp64, on the device (`-m gpu`): `tipk_distmult_fwd` (V = 4 / V = 1, the
four id / relation width pairs, logit bands up to the overflow of expf, non-finite rows), the three routes of `tipk_distmult_bwd`
(task kernel, generic kernel with the d z image in LDS, generic kernel with global atomics) and `tipk_distmult_loss` on the generic
kernel.  The cases are `tests/distmult_cases.py` (checked on the CPU by tests/test_host_distmult_cases.py), the reference and the
bound `tests/distmult_spec.py`.

Every case runs twice: random values against the bound, and the EXACT variant -- z, w from {-1, 0, 1}, g_score from signed powers
of two, no sigmoid: every partial sum is an exact fp32 number (`distmult_spec.exact_ok`), so every route, the fixed-point one
included, must equal fp64 bit for bit.  Every comparison prints one `DMERR` line; profiles/distmult_routes_errors.md is the table
of the largest shares on an MI355X."""
import ctypes as C

import pytest
import torch

import distmult_cases as T
import distmult_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
IDS = lambda kind: [c['id'] for c in T.CASES if c['kind'] == kind]


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops
    return ops


def _L():
    from tip_amd import _lib
    return _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _place(t, offset):
    """t on the device; offset: its base address 4 bytes past a 16-byte boundary (the kernels then take the V = 1 path)."""
    if not offset:
        d = t.to(DEV).contiguous()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4
    return d


def _device_case(c, x):
    it = torch.int32 if c['idx'] == 4 else torch.int64
    rt = torch.int32 if c['et'] == 4 else torch.int64
    z, w = _place(x['z'], c['offset'] == 'z'), _place(x['w'], c['offset'] == 'w')
    ei = torch.stack([x['u'], x['v']]).to(DEV, it)
    return z, w, ei, x['r'].to(DEV, rt)


def c_fwd(z, w, ei, et, sigmoid):
    L = _L()
    n = ei.shape[1]
    score = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    L.check(L.lib().tipk_distmult_fwd(_p(z), z.shape[0], z.shape[1], _p(w), w.shape[0], _p(ei[0]), _p(ei[1]), ei.element_size(),
                                      _p(et), et.element_size(), n, int(sigmoid), _p(score), L.stream_ptr(z.device)), 'tipk_distmult_fwd')
    return score


def c_bwd(g, score, z, w, ei, et, sigmoid, tasks, g_z, g_w):
    L = _L()
    L.check(L.lib().tipk_distmult_bwd(_p(g), _p(score), _p(z), z.shape[0], z.shape[1], _p(w), w.shape[0], _p(ei[0]), _p(ei[1]),
                                      ei.element_size(), _p(et), et.element_size(), ei.shape[1], int(sigmoid), _p(tasks),
                                      0 if tasks is None else tasks.shape[0], _p(g_z), _p(g_w), L.stream_ptr(z.device)),
            'tipk_distmult_bwd')
    torch.cuda.synchronize()
    return g_z, g_w


def _tasks(ops, c, et):
    if not c['tasks']:
        return None
    tasks = ops.relation_tasks(et)
    assert tasks is not None and int((tasks[:, 2] - tasks[:, 1]).max()) <= ops.TASK_POSITIONS
    return tasks


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def _fwd_variants():
    """(the band and non-finite cases are about their values: they have no exact variant)"""
    out = []
    for c in T.CASES:
        if c['kind'] == 'fwd':
            out += [(c['id'], False)] + [(c['id'], True)] * (c['band'] is None and c['special'] is None)
    return out


@pytest.mark.parametrize('cid,exact', _fwd_variants(), ids=lambda v: {False: 'random', True: 'exact'}.get(v, v))
def test_fwd_vs_fp64(cid, exact):
    c = T.BY_ID[cid]
    n = T.resolved(c)
    x = T.inputs(cid, n, exact)
    z, w, ei, et = _device_case(c, x)
    for sig in ((False,) if exact else (False, True)):
        got = c_fwd(z, w, ei, et, sig)
        want, bound = S.fwd_reference(x['z'], x['w'], x['u'], x['v'], x['r'], sig)
        what = 'score' if sig else 'logit'
        if exact:
            S.check_exact(got, want, cid, what)
        else:
            S.check(got, want, bound, cid, what, same_kind=True)
    if c['special'] == 'rows':
        assert int(torch.isnan(want).sum()) > 0 and int(torch.isfinite(want).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def _bwd_variants():
    out = []
    for c in T.CASES:
        if c['kind'] == 'bwd':
            out += [(c['id'], 'random'), (c['id'], 'exact')] + [(c['id'], 'sigmoid')] * c['sig']
    return out


@pytest.mark.parametrize('cid,variant', _bwd_variants(), ids=lambda v: v)
def test_bwd_routes_vs_fp64(cid, variant, ops):
    c = T.BY_ID[cid]
    n = T.resolved(c)
    assert T.case_route(c, n) == c['route'], (cid, n, T.case_route(c, n))
    exact, sig = variant == 'exact', variant == 'sigmoid'
    x = T.inputs(cid, n, exact)
    z, w, ei, et = _device_case(c, x)
    g = x['g'].to(DEV)
    score = c_fwd(z, w, ei, et, True) if sig else None
    pre = x.get('prefill') if exact else None
    if c['entry'] == 'ops':
        assert (ops.relation_tasks(et) is not None) == c['tasks']
        g_z, g_w = ops.distmult_bwd(g, score, z, w, ei, et, sigmoid=sig)
        torch.cuda.synchronize()
    else:
        g_z = torch.zeros_like(z) if pre is None else pre[0].to(DEV)
        g_w = torch.zeros_like(w) if pre is None else pre[1].to(DEV)
        assert g_z.data_ptr() % 16 == 0
        c_bwd(g, score, z, w, ei, et, sig, _tasks(ops, c, et), g_z, g_w)
    (wz, ww), (bz, bw) = S.bwd_reference(x['g'], x['z'], x['w'], x['u'], x['v'], x['r'], sig, task_route=c['route'] == 'task')
    tag = cid + ('.sig' if sig else '')
    if exact:
        S.exact_ok(x['g'], x['z'], x['w'], x['u'], x['v'], x['r'], pre, unit=1.0)
        if pre is not None:                                  # the accumulate contract: prefill + gradient, untouched rows keep theirs
            wz, ww = wz + pre[0].double(), ww + pre[1].double()
            cold = n // 2
            assert torch.equal(g_z[cold].cpu(), pre[0][cold]) and torch.equal(g_w[0].cpu(), pre[1][0])
        S.check_exact(g_z, wz, tag, 'd_z')
        S.check_exact(g_w, ww, tag, 'd_w')
    else:
        S.check(g_z, wz, bz, tag, 'd_z')
        S.check(g_w, ww, bw, tag, 'd_w')


# ---------------------------------------------------------------------------------------------------------------------
# the objective on the generic kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('need_grad', [True, False], ids=['grad', 'nograd'])
@pytest.mark.parametrize('cid', IDS('loss'))
def test_generic_objective_vs_fp64(cid, need_grad, ops):
    c = T.BY_ID[cid]
    n = T.resolved(c)
    assert T.case_route(c, n) == c['route'], (cid, n, T.case_route(c, n))
    assert T.route_name(n, c['k'], 2, c['tasks'], c['tasks'], 8, True) == 'generic_global'        # without gradients: no image
    x = T.inputs(cid, n, False)
    z, w, pos, et = _device_case(c, x)
    neg = torch.stack([x['nu'], x['nv']]).to(DEV)
    assert (ops.relation_tasks(et, pos) is not None) == c['tasks']
    if c['packed']:                                          # the sampler's packed form: the fused kernel refuses this n, ops falls back
        assert T.route_name(n, c['k'], 1, True, True, 2, True) == _L()._CONSTANTS['EUNSUPPORTED']
        word = x['nu'] | (x['nv'] << 16)
        neg = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(DEV, torch.int32)
        neg._tipk_packed_pairs = True
    loss, g_z, g_w = ops.distmult_loss(z, w, pos, neg, et, need_grad=need_grad)
    torch.cuda.synchronize()
    (wl, wz, ww), (bl, bz, bw) = S.loss_reference(x['z'], x['w'], x['u'], x['v'], x['nu'], x['nv'], x['r'])
    tag = cid + ('' if need_grad else '.nograd')
    S.check(loss, wl.reshape(1), bl, tag, 'loss')
    if need_grad:
        S.check(g_z, wz, bz, tag, 'd_z')
        S.check(g_w, ww, bw, tag, 'd_w')
    else:
        assert g_z is None and g_w is None


# ---------------------------------------------------------------------------------------------------------------------
# non-finite policy (include/tipk.h section 4): nothing that fp64 makes NaN or infinite comes out finite, on any route; the
# generic routes keep every other element inside the bound; the task route may poison more.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', T.NONFINITE_BAD)
@pytest.mark.parametrize('route', list(T.NONFINITE_ROUTES))
def test_bwd_non_finite_policy(route, bad, ops):
    spec = T.NONFINITE_ROUTES[route]
    n = T.resolve(spec['n'], T.route_of)
    assert T.route_of(n, 16, spec['tasks']) == route
    x = T.nonfinite_inputs(n, bad, spec['tasks'])
    z, w, g = x['z'].to(DEV), x['w'].to(DEV), x['g'].to(DEV)
    ei, et = torch.stack([x['u'], x['v']]).to(DEV), x['r'].to(DEV)
    tasks = ops.relation_tasks(et) if spec['tasks'] else None
    g_z, g_w = c_bwd(g, None, z, w, ei, et, False, tasks, torch.zeros_like(z), torch.zeros_like(w))
    (wz, ww), (bz, bw) = S.bwd_reference(x['g'], x['z'], x['w'], x['u'], x['v'], x['r'], False, task_route=route == 'task')
    if bad != 'g_overflow':
        assert not bool(torch.isfinite(wz).all()), 'the case has no non-finite element'
    tag = 'nonfinite.%s.%s' % (route, bad)
    S.check(g_z, wz, bz, tag, 'd_z', finite_inside=route != 'task')
    S.check(g_w, ww, bw, tag, 'd_w')
    if route == 'task' and bad == 'g_overflow':              # its bound overflows: the rule of tipk.h poisons all of d z
        assert bool(torch.isnan(g_z).all())
