"""CPU checks of `tests/distmult_cases.py` (no GPU: `tipk_distmult_route` is a pure host query):
  - every route, variant and boundary the table must cover has a case, and every case takes the route written next to it;
  - every case holds what its layout promises, and the exact variant's premise (`distmult_spec.exact_ok`) holds;
  - the bound of `tests/distmult_spec.py` admits the plain fp32 emulation on EVERY element of every random case, in three
    seeded orders of the triples; the largest share is printed."""
import pytest
import torch

import distmult_cases as T
import distmult_spec as S

ORDERS = (1, 2, 3)


route_code, route_name, route_of, resolved, case_route = T.route_code, T.route_name, T.route_of, T.resolved, T.case_route


def test_route_query_contract():
    from tip_amd import _lib
    EINVAL, EUNSUPPORTED = _lib._CONSTANTS['EINVAL'], _lib._CONSTANTS['EUNSUPPORTED']
    assert [route_code(r) for r in T.ROUTES] == [0, 1, 2, 3]
    assert route_name(645, 16, 1, True, True, 8, True) == 'objective'            # BioSNAP: the fused objective
    assert route_name(645, 16, 1, True, True, 2, True) == 'objective'
    assert route_name(645, 16, 1, True, False, 8, True) == 'task'                # no workspace: the task kernel, float atomics
    assert route_name(300, 32, 1, True, True, 8, True) == 'task'                 # k = 32: no objective kernel
    assert route_name(645, 16, 0, True, False, 8, True) == 'task'
    assert route_name(645, 16, 0, False, False, 8, True) == 'generic_lds'
    assert route_name(645, 16, 0, True, False, 8, False) == 'generic_lds'        # misaligned z / rel_w
    assert route_name(645, 6, 0, True, False, 4, True) == 'generic_lds'
    assert route_name(645, 16, 2, False, False, 8, True) == 'generic_global'     # objective only: no d z image
    assert route_name(645, 16, 1, False, False, 2, True) == EUNSUPPORTED         # packed pairs: the objective kernel only
    assert route_name(300, 32, 1, True, True, 2, True) == EUNSUPPORTED
    assert route_name(T.resolve(('task_next', 16), route_of), 16, 1, True, True, 2, True) == EUNSUPPORTED
    assert route_name(645, 16, 0, True, False, 2, True) == EINVAL
    assert route_name(645, 16, 3, True, False, 8, True) == EINVAL
    assert route_name(645, 0, 0, True, False, 8, True) == EINVAL
    assert route_name(645, 16, 0, True, False, 5, True) == EINVAL


def test_route_boundaries_come_from_the_library():
    """the boundaries move with k as the LDS budget says, and sit where include/tipk.h section 4 puts them."""
    last = {k: T.resolve(('task_last', k), route_of) for k in (4, 8, 16, 32, 64)}
    assert last[4] > last[8] > last[16] > last[32] > last[64] > 64
    lds = lambda n, k: ((n * (k + 1) + 1) // 2 * 2) * 8 + ((n * (k + 4) + 3) // 4 * 4 + 16 * k + 16) * 4 + 16 * 1024
    for k, n in last.items():
        assert lds(n, k) <= 158 * 1024 < lds(n + 1, k), (k, n, lds(n, k))
    assert (last[4], last[16], last[64]) == (2015, 668, 178)                     # the three the header quotes
    for k in (6, 16):
        n = T.resolve(('lds_last', k), route_of)
        assert n * k * 4 <= 96 * 1024 < (n + 1) * k * 4


def test_table_covers_every_route_variant_and_boundary():
    have = set()
    for c in T.CASES:
        n = resolved(c)
        if c['route'] is not None:
            assert case_route(c, n) == c['route'], (c['id'], n, case_route(c, n))
        have.update(T.tags(c, n))
    missing = [t for t in T.REQUIRED if t not in have]
    assert not missing, missing
    for route in T.NONFINITE_ROUTES:
        spec = T.NONFINITE_ROUTES[route]
        assert route_of(T.resolve(spec['n'], route_of), 16, spec['tasks']) == route
    assert set(T.NONFINITE_ROUTES) == {'task', 'generic_lds', 'generic_global'}
    assert set(T.NONFINITE_BAD) == {'g_nan', 'g_pinf', 'g_ninf', 'z_nan', 'w_nan', 'g_overflow'}


@pytest.mark.parametrize('cid', [c['id'] for c in T.CASES])
def test_case_promises_and_exact_premise(cid):
    c = T.BY_ID[cid]
    n = resolved(c)
    x = T.inputs(cid, n, True)
    E = x['u'].numel()
    assert E == sum(c['runs']) and int(x['u'].max()) < n and int(x['v'].max()) < n and int(x['r'].max()) < x['R']
    assert E == 1 or (E >= 8 and n >= 4), 'a layout too small for its promises'
    if E >= 8:
        p = T.promises(x['u'], x['v'], x['r'], n, x['R'])
        assert all(p.values()), (cid, p)
    if c['layout'] == 'grouped':
        assert bool((x['r'][1:] >= x['r'][:-1]).all())
        assert all(run <= 2049 for run in c['runs']) or not c['tasks']
    else:
        rels = torch.unique_consecutive(x['r'])
        assert torch.unique(rels).numel() < rels.numel(), 'a shuffled list that is still grouped by relation'
    if c['kind'] == 'bwd':
        S.exact_ok(x['g'], x['z'], x['w'], x['u'], x['v'], x['r'], x.get('prefill'), unit=1.0)
    if c['band'] is not None:
        y = T.inputs(cid, n, False)
        z, w = y['z'].double(), y['w'].double()
        top = float((z[y['u']] * z[y['v']] * w[y['r']]).sum(1).abs().max())
        if c['kind'] == 'loss':
            top = max(top, float((z[y['nu']] * z[y['nv']] * w[y['r']]).sum(1).abs().max()))
        assert abs(top - c['band']) < 1e-3 * c['band']


@pytest.mark.parametrize('cid', [c['id'] for c in T.CASES if c['special'] is None])
def test_bound_admits_fp32_emulation(cid):
    c = T.BY_ID[cid]
    n = resolved(c)
    x = T.inputs(cid, n, False)
    z, w, u, v, r = (x[a] for a in 'zwuvr')
    shares = {}

    def hold(got, want, bound, what):
        shares[what] = max(shares.get(what, 0.0), S.check(got, want, bound, cid, what, out=lambda s: None))
    if c['kind'] == 'fwd':
        for sig in (False, True):
            want, bound = S.fwd_reference(z, w, u, v, r, sig)
            hold(S.emulate_fwd(z, w, u, v, r, sig), want, bound, 'score' if sig else 'logit')
    elif c['kind'] == 'bwd':
        for sig in ((False, True) if c['sig'] else (False,)):
            (wz, ww), (bz, bw) = S.bwd_reference(x['g'], z, w, u, v, r, sig, task_route=False)     # (the tighter of the two bounds)
            for seed in ORDERS:
                gz, gw = S.emulate_bwd(x['g'], z, w, u, v, r, sig, seed)
                hold(gz, wz, bz, 'd_z' + '.sig' * sig)
                hold(gw, ww, bw, 'd_w' + '.sig' * sig)
    else:
        (wl, wz, ww), (bl, bz, bw) = S.loss_reference(z, w, u, v, x['nu'], x['nv'], r)
        for seed in ORDERS:
            l, gz, gw = S.emulate_loss(z, w, u, v, x['nu'], x['nv'], r, seed)
            hold(l, wl.reshape(1), bl, 'loss')
            hold(gz, wz, bz, 'd_z')
            hold(gw, ww, bw, 'd_w')
    print('DMSHARE %s %s' % (cid, ' '.join('%s=%.3f' % kv for kv in sorted(shares.items()))))
    assert shares and max(shares.values()) <= 1.0
