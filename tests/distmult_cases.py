"""The case table of the DistMult decoder outside its fused fast path: `tipk_distmult_fwd`, the three routes of `tipk_distmult_bwd`
and `tipk_distmult_loss` on the generic kernel.  `tests/test_host_distmult_cases.py` checks the table on the CPU (coverage, what
every case promises, the bound of `tests/distmult_spec.py` against the fp32 emulation), `tests/test_gpu_distmult_routes.py` runs it.

A case names n, k, the triple layout (run lengths per relation; relation ids are 1, 3, 5, ... so that every even relation is
EMPTY), the id widths, how it is called and the route it must take.  No boundary is written down: a size given as a tuple is
resolved from `tipk_distmult_route` by bisection (`resolve`).  The 48 KB step is not a route boundary (it is where the generic
kernel's LDS image first needs the attribute call): 48 * 1024 / (4 k) rows, and one more.

What every layout with at least 8 triples and 4 nodes promises (`promises`): node 0 and node n - 1 are used, self-pairs u = v are
present, node 0 is in EVERY triple of the longest relation (2 049 adds into one row of the LDS image), node n // 2 is never touched,
and every even relation is empty."""
import functools

import torch

import distmult_spec as S

ROUTES = ('generic_global', 'generic_lds', 'task', 'objective')
TASK_RUNS = (1, 1023, 1024, 1025, 2047, 2048, 2049)          # the last one splits 2 048 + 1
WAVE_RUNS = (64, 128, 37, 91, 700, 5)                        # waves of one relation, of several, and one partly past the end
BIG = 4096 * 1024 + 257                                      # where per_block of the generic kernel starts to grow


def _c(cid, kind, n, k, runs, route=None, layout='grouped', idx=8, et=8, tasks=False, entry='c', offset=None, sig=False,
       prefill=False, band=None, packed=False, special=None):
    return dict(id=cid, kind=kind, n=n, k=k, runs=tuple(runs), route=route, layout=layout, idx=idx, et=et, tasks=tasks, entry=entry,
                offset=offset, sig=sig, prefill=prefill, band=band, packed=packed, special=special)


CASES = [
    # ---- forward: k, V = 1 by k and by a 4-byte-offset base, the four width pairs, the block edge of 256 triples
    _c('f_k4_e1', 'fwd', 37, 4, (1,), idx=4, et=4),
    _c('f_k6_e255', 'fwd', 37, 6, (200, 55), idx=8, et=8),
    _c('f_k16_e256', 'fwd', 37, 16, (100, 156), idx=4, et=8),
    _c('f_k64_e257', 'fwd', 37, 64, (257,), idx=8, et=4),
    _c('f_k16_zoff', 'fwd', 37, 16, (257,), idx=4, et=4, offset='z'),
    _c('f_k4_woff', 'fwd', 37, 4, (257,), idx=8, et=8, offset='w'),
    _c('f_band8', 'fwd', 37, 16, (257,), band=8.0),
    _c('f_band20', 'fwd', 37, 16, (257,), band=20.0),
    _c('f_band40', 'fwd', 37, 16, (257,), band=40.0),
    _c('f_band88', 'fwd', 37, 16, (257,), band=88.0),
    _c('f_band104', 'fwd', 37, 16, (257,), band=104.0),
    _c('f_nonfinite', 'fwd', 37, 16, (257,), special='rows'),
    # ---- backward, task route: 1 .. 16 lanes per position, both id widths, the task lengths, more tasks than workgroups
    _c('t_k4', 'bwd', 61, 4, TASK_RUNS, 'task', idx=4, et=4, tasks=True),
    _c('t_k8', 'bwd', 61, 8, TASK_RUNS, 'task', idx=8, et=8, tasks=True, prefill=True),
    _c('t_k16', 'bwd', 61, 16, TASK_RUNS, 'task', idx=4, et=8, tasks=True, sig=True),
    _c('t_k32', 'bwd', 61, 32, TASK_RUNS, 'task', idx=8, et=4, tasks=True),
    _c('t_k64', 'bwd', 61, 64, TASK_RUNS, 'task', idx=4, et=4, tasks=True),
    _c('t_300rel', 'bwd', 61, 16, tuple(1 + i % 5 for i in range(300)), 'task', tasks=True),
    _c('t_ops', 'bwd', 61, 16, WAVE_RUNS, 'task', tasks=True, entry='ops'),
] + [
    _c('t_last_k%d' % k, 'bwd', ('task_last', k), k, (700, 300), 'task', idx=4 if k in (4, 16, 64) else 8, tasks=True)
    for k in (4, 8, 16, 32, 64)
] + [
    _c('g_next_k%d' % k, 'bwd', ('task_next', k), k, (700, 300), 'generic_lds', idx=4 if k in (4, 16, 64) else 8, tasks=True)
    for k in (4, 8, 16, 32, 64)
] + [
    # ---- backward, generic routes (tasks = NULL through the C entry; a shuffled list through ops)
    _c('g_lds48', 'bwd', ('bytes', 48 * 1024, 16, 0), 16, WAVE_RUNS, 'generic_lds', idx=4, et=4, prefill=True),
    _c('g_lds48p', 'bwd', ('bytes', 48 * 1024, 16, 1), 16, WAVE_RUNS, 'generic_lds', idx=8, et=4, sig=True),
    _c('g_lds96', 'bwd', ('lds_last', 16), 16, WAVE_RUNS, 'generic_lds', idx=4, et=8),
    _c('g_glob96', 'bwd', ('lds_next', 16), 16, WAVE_RUNS, 'generic_global', idx=8, et=8, sig=True),
    _c('g_k6_lds', 'bwd', 50, 6, WAVE_RUNS, 'generic_lds', idx=4, et=4, tasks=True),            # tasks given: k = 6 has no task route
    _c('g_k6_lds96', 'bwd', ('lds_last', 6), 6, WAVE_RUNS, 'generic_lds', idx=8, et=8),
    _c('g_k6_glob', 'bwd', ('lds_next', 6), 6, WAVE_RUNS, 'generic_global', idx=4, et=8, prefill=True),
    _c('g_k16_zoff', 'bwd', 61, 16, WAVE_RUNS, 'generic_lds', idx=8, et=4, tasks=True, offset='z'),   # misaligned: no task route, V = 1
    _c('g_shuffled_ops', 'bwd', 61, 16, WAVE_RUNS, 'generic_lds', layout='shuffled', entry='ops'),
    _c('g_e1', 'bwd', 33, 4, (1,), 'generic_lds', idx=4, et=4),
    _c('g_e4095', 'bwd', 33, 4, (4000, 95), 'generic_lds', idx=4, et=4),
    _c('g_e4096', 'bwd', 33, 4, (4000, 96), 'generic_lds', idx=4, et=4),
    _c('g_e4097', 'bwd', 33, 4, (4000, 97), 'generic_lds', idx=4, et=4),
    _c('g_e8193', 'bwd', 33, 4, (4000, 4193), 'generic_lds', idx=4, et=4),
    _c('g_big', 'bwd', 40, 4, (1400000, 64, BIG - 1400064), 'generic_lds', idx=4, et=4),
    # ---- the objective on the generic kernel, through ops.distmult_loss: k = 6, an ungrouped list, n past the task limit
    _c('l_k6_lds', 'loss', 100, 6, WAVE_RUNS, 'generic_lds', layout='shuffled', entry='ops'),
    _c('l_k6_lds48p', 'loss', ('bytes', 48 * 1024, 6, 52), 6, WAVE_RUNS, 'generic_lds', layout='shuffled', entry='ops'),
    _c('l_k6_glob', 'loss', ('lds_next', 6), 6, WAVE_RUNS, 'generic_global', layout='shuffled', entry='ops'),
    _c('l_k16_past', 'loss', ('task_next', 16), 16, WAVE_RUNS, 'generic_lds', tasks=True, entry='ops'),
    _c('l_k16_packed', 'loss', ('task_next', 16), 16, WAVE_RUNS, 'generic_lds', tasks=True, entry='ops', packed=True),
    _c('l_band20', 'loss', 100, 6, WAVE_RUNS, 'generic_lds', layout='shuffled', entry='ops', band=20.0),
    _c('l_band40', 'loss', 100, 6, WAVE_RUNS, 'generic_lds', layout='shuffled', entry='ops', band=40.0),
]
BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the non-finite policy: every route x every way an input can be non-finite
NONFINITE_ROUTES = {'task': dict(n=61, tasks=True), 'generic_lds': dict(n=61, tasks=False), 'generic_global': dict(n=('lds_next', 16), tasks=False)}
NONFINITE_BAD = ('g_nan', 'g_pinf', 'g_ninf', 'z_nan', 'w_nan', 'g_overflow')

# what the table must cover (tests/test_host_distmult_cases.py: `tags` derives them from the case's fields)
REQUIRED = (
    ['fwd:k%d' % k for k in (4, 6, 16, 64)] + ['fwd:offset_z', 'fwd:offset_w'] + ['fwd:i%de%d' % p for p in ((4, 4), (4, 8), (8, 4), (8, 8))]
    + ['fwd:e%d' % e for e in (1, 255, 256, 257)] + ['fwd:band%d' % b for b in (8, 20, 40, 88, 104)] + ['fwd:nonfinite_rows']
    + ['task:k%d' % k for k in (4, 8, 16, 32, 64)] + ['task:i4', 'task:i8'] + ['task:run%d' % r for r in TASK_RUNS]
    + ['task:more_tasks_than_workgroups', 'task:ops', 'task:sig', 'task:prefill']
    + ['task:last_k%d' % k for k in (4, 8, 16, 32, 64)] + ['generic:next_k%d' % k for k in (4, 8, 16, 32, 64)]
    + ['generic:lds48', 'generic:lds48+row', 'generic:lds96', 'generic:global96+row', 'generic:V1_k6', 'generic:V1_offset', 'generic:V4']
    + ['generic:i%de%d' % p for p in ((4, 4), (4, 8), (8, 4), (8, 8))] + ['generic:waves_uniform_mixed_tail', 'generic:shuffled_ops']
    + ['generic:e%d' % e for e in (1, 4095, 4096, 4097, 8193)] + ['generic:per_block_grows']
    + ['generic_lds:sig', 'generic_global:sig', 'generic_lds:prefill', 'generic_global:prefill']
    + ['loss:generic_lds', 'loss:generic_lds_over_48k', 'loss:generic_global', 'loss:k6', 'loss:ungrouped', 'loss:past_task_limit',
       'loss:packed_fallback', 'loss:band20', 'loss:band40']
)


def first(pred, lo, hi):
    """the smallest v in [lo, hi) with pred(v) (pred monotone: False ... False True ... True)."""
    assert pred(hi - 1) and not pred(lo)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def resolve(n, route_of):
    """a node count of the table: an int, or a boundary found from `route_of(n, k, tasks)` (the library's route name)."""
    if isinstance(n, int):
        return n
    if n[0] == 'bytes':
        _, nbytes, k, more = n
        assert nbytes % (4 * k) == 0
        return nbytes // (4 * k) + more
    kind, k = n
    if kind in ('task_last', 'task_next'):
        nxt = first(lambda m: route_of(m, k, True) != 'task', 1, 1 << 17)
        assert route_of(nxt - 1, k, True) == 'task'
        return nxt - 1 if kind == 'task_last' else nxt
    nxt = first(lambda m: route_of(m, k, False) != 'generic_lds', 1, 1 << 17)
    assert route_of(nxt - 1, k, False) == 'generic_lds' and route_of(nxt, k, False) == 'generic_global'
    return nxt - 1 if kind == 'lds_last' else nxt


# ---------------------------------------------------------------------------------------------------------------------
# the library's route query (imported on first use: this module itself needs no tip_amd)
# ---------------------------------------------------------------------------------------------------------------------
def route_code(name):
    from tip_amd import _lib
    return _lib._CONSTANTS['DM_ROUTE_' + name.upper()]


def route_name(n, k, mode, tasks, ws, idx, aligned):
    """tipk_distmult_route -> its name in ROUTES, or the negative status."""
    from tip_amd import _lib
    code = _lib.lib().tipk_distmult_route(n, k, mode, int(tasks), int(ws), idx, int(aligned))
    return ROUTES[code] if code >= 0 else code


def route_of(n, k, tasks):
    return route_name(n, k, 0, tasks, False, 8, True)


def resolved(c):
    return resolve(c['n'], route_of)


def case_route(c, n):
    """the route the library reports for the call the case makes."""
    if c['kind'] == 'loss':                                # (ops passes tasks only for a grouped list, and then a workspace too)
        return route_name(n, c['k'], 1, c['tasks'], c['tasks'], c['idx'], True)
    return route_name(n, c['k'], 0, c['tasks'], False, c['idx'], c['offset'] is None)


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors; built once per (case, variant) and shared)
# ---------------------------------------------------------------------------------------------------------------------
def triples(n, runs, layout, seed):
    """-> (u, v, r int64 [E], R).  Relation of run i is 2 i + 1."""
    g = torch.Generator().manual_seed(seed)
    E, R = sum(runs), 2 * len(runs) + 1
    cold = n // 2 if n >= 4 else -1

    def draw():
        x = torch.randint(0, n, (E,), generator=g)
        return torch.where(x == cold, x - 1, x)
    u, v = draw(), draw()
    r = torch.repeat_interleave(2 * torch.arange(len(runs)) + 1, torch.tensor(runs))
    if E >= 8 and n >= 4:
        i = max(range(len(runs)), key=lambda j: runs[j])
        b = sum(runs[:i])
        u[b:b + runs[i]] = 0                                    # the hot node
        p = torch.arange(3, E, 7)
        v[p] = u[p]                                             # self-pairs (some on the hot node)
        v[b] = n - 1
    if layout == 'shuffled':
        perm = torch.randperm(E, generator=g)
        u, v, r = u[perm], v[perm], r[perm]
    return u, v, r, R


def promises(u, v, r, n, R):
    """what `triples` promises for E >= 8, n >= 4 -> dict of booleans."""
    used = torch.zeros(n, dtype=torch.bool)
    used[u], used[v] = True, True
    rels, cnt = torch.unique(r, return_counts=True)
    top = rels[torch.argmax(cnt)]
    return dict(node0=bool(used[0]), last_node=bool(used[n - 1]), self_pairs=bool((u == v).any()),
                hot_node=bool(((u == 0) | (v == 0))[r == top].all()), cold_node=not bool(used[n // 2]),
                empty_relations=rels.numel() < R and not bool((rels % 2 == 0).any()))


def _ints(shape, g):
    return torch.tensor([-1.0, 0.0, 0.0, 1.0])[torch.randint(0, 4, shape, generator=g)]


def _pow2(shape, g):
    return torch.tensor([-1.0, 1.0])[torch.randint(0, 2, shape, generator=g)] * 2.0 ** torch.randint(0, 3, shape, generator=g).float()


@functools.lru_cache(maxsize=4)
def inputs(cid, n, exact):
    """The inputs of a case at its resolved n -> dict(z, w, u, v, r, R, g [, nu, nv, prefill])."""
    c = BY_ID[cid]
    seed = CASES.index(c) * 10 + int(exact)
    g = torch.Generator().manual_seed(1000 + seed)
    u, v, r, R = triples(n, c['runs'], c['layout'], seed)
    k, E = c['k'], u.numel()
    if exact:
        z, w, gs = _ints((n, k), g), _ints((R, k), g), _pow2((E,), g)
    else:
        z, w, gs = torch.randn((n, k), generator=g), torch.randn((R, k), generator=g), torch.randn((E,), generator=g)
        gs[::11] = 0.0
    out = dict(u=u, v=v, r=r, R=R)
    if c['kind'] == 'loss':
        nu = torch.randint(0, n, (E,), generator=g)
        nv = torch.randint(0, n, (E,), generator=g)
        out.update(nu=nu, nv=nv)
    if c['band'] is not None:                                   # scale z: the largest |logit| of the case becomes the band
        z64, w64 = z.double(), w.double()
        top = float((z64[u] * z64[v] * w64[r]).sum(1).abs().max())
        if c['kind'] == 'loss':
            top = max(top, float((z64[out['nu']] * z64[out['nv']] * w64[r]).sum(1).abs().max()))
        z = (z64 * (c['band'] / top) ** 0.5).float()
    if c['special'] == 'rows':
        z[3, 0], z[3, 1], z[3, 2], z[3, 3] = 0.0, -0.0, float('inf'), float('-inf')
        z[5, 7] = float('nan')
        z[7, 2], z[7, 3] = -0.0, 0.0
    if c['prefill'] and exact:
        out['prefill'] = (torch.randint(-7, 8, (n, k), generator=g).float(), torch.randint(-7, 8, (R, k), generator=g).float())
    out.update(z=z, w=w, g=gs)
    return out


def nonfinite_inputs(n, bad, tasks):
    """k = 16, the grouped WAVE_RUNS layout; `bad` puts one non-finite value (or the overflowing g_score) into it."""
    g = torch.Generator().manual_seed(77)
    u, v, r, R = triples(n, WAVE_RUNS, 'grouped', 77)
    z, w = 0.25 * torch.randn((n, 16), generator=g), 0.25 * torch.randn((R, 16), generator=g)
    gs = torch.randn((u.numel(),), generator=g)
    if bad == 'g_nan':
        gs[70] = float('nan')
    elif bad == 'g_pinf':
        gs[70] = float('inf')
    elif bad == 'g_ninf':
        gs[70] = float('-inf')
    elif bad == 'z_nan':
        z[int(u[70]), 5] = float('nan')
    elif bad == 'w_nan':
        w[int(r[70]), 5] = float('nan')
    else:                                                       # finite, but sum |g| > FLT_MAX; |z w| <= ~1: every term fits fp32
        gs[70], gs[71], gs[300] = 1.5e38, -1.5e38, 1.5e38
        assert float(gs.double().abs().sum()) > S.F32_MAX
    return dict(z=z, w=w, u=u, v=v, r=r, R=R, g=gs)


def tags(c, n):
    """what a case covers, derived from its fields and its resolved n (not written next to it)."""
    t, k, runs, E = [], c['k'], c['runs'], sum(c['runs'])
    wp = 'i%de%d' % (c['idx'], c['et'])
    if c['kind'] == 'fwd':
        plain = c['band'] is None and c['special'] is None
        if plain and c['offset'] is None:
            t += ['fwd:k%d' % k, 'fwd:' + wp, 'fwd:e%d' % E]
        if c['offset'] and k % 4 == 0:
            t.append('fwd:offset_' + c['offset'])
        if c['band'] is not None:
            t.append('fwd:band%d' % c['band'])
        if c['special'] == 'rows':
            t.append('fwd:nonfinite_rows')
    elif c['kind'] == 'bwd' and c['route'] == 'task':
        t += ['task:k%d' % k, 'task:i%d' % c['idx']] + ['task:run%d' % x for x in runs if x in TASK_RUNS]
        if len(runs) > 256:
            t.append('task:more_tasks_than_workgroups')
        t += ['task:ops'] * (c['entry'] == 'ops') + ['task:sig'] * c['sig'] + ['task:prefill'] * c['prefill']
        if c['n'] == ('task_last', k):
            t.append('task:last_k%d' % k)
    elif c['kind'] == 'bwd':
        if c['n'] == ('task_next', k) and c['tasks']:
            t.append('generic:next_k%d' % k)
        nbytes = n * k * 4
        if c['route'] == 'generic_lds' and k == 16:
            t += ['generic:lds48'] * (nbytes == 48 * 1024) + ['generic:lds48+row'] * (nbytes == 48 * 1024 + 4 * k)
            t += ['generic:lds96'] * (c['n'] == ('lds_last', k))
        if c['route'] == 'generic_global' and c['n'] == ('lds_next', k):
            t.append('generic:global96+row')
        t.append('generic:V1_k6' if k % 4 else ('generic:V1_offset' if c['offset'] else 'generic:V4'))
        t.append('generic:' + wp)
        if runs == WAVE_RUNS and c['layout'] == 'grouped' and 64 in runs and E % 64 and not c['tasks']:
            t.append('generic:waves_uniform_mixed_tail')
        if c['layout'] == 'shuffled' and c['entry'] == 'ops':
            t.append('generic:shuffled_ops')
        t.append('generic:e%d' % E)
        if E > 4096 * 1024:
            t.append('generic:per_block_grows')
        t += [c['route'] + ':sig'] * c['sig'] + [c['route'] + ':prefill'] * c['prefill']
    else:
        t.append('loss:' + c['route'])
        t += ['loss:generic_lds_over_48k'] * (c['route'] == 'generic_lds' and n * k * 4 > 48 * 1024)
        t += ['loss:k6'] * (k == 6) + ['loss:ungrouped'] * (c['layout'] == 'shuffled')
        t += ['loss:past_task_limit'] * (c['n'] == ('task_next', k) and not c['packed'])
        t += ['loss:packed_fallback'] * (c['n'] == ('task_next', k) and c['packed'])
        if c['band'] is not None:
            t.append('loss:band%d' % c['band'])
    return t
