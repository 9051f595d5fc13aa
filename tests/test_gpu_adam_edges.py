"""tipk_adam_step (include/tipk.h section 9) against the fp64 rule and rounding bound of tests/adam_spec.py, at its rule,
launch, list and count edges.

Every case cuts its tensors out of ONE arena that is otherwise filled with a sentinel word (at least 8 before and after each
tensor).  After every launch: every arena word outside the parameters and moments (sentinels, gaps, the gradients) is
bitwise what it was, all 528 ticket words are 0, every step word moved by exactly what the case expects.  Values are always
compared ONE step from the kernel's own fp32 state: a multi-step case reads the state back and feeds it to the spec."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_spec as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = np.int32(0x7FA5C3C3)                       # a NaN: a kernel that reads one shows it
GUARD = -7777                                         # around the step words
EINVAL = -1
SHARES = {'dP': 0.0, 'dM': 0.0, 'dV': 0.0}


@pytest.fixture(scope='module', autouse=True)
def _report_shares():
    yield
    print('\nadam edges, largest share of each bound used on the GPU: dP %.3f dM %.3f dV %.3f'
          % (SHARES['dP'], SHARES['dM'], SHARES['dV']))


def _note(used):
    for k in SHARES:
        SHARES[k] = max(SHARES[k], used[k])


class Case:
    """tensors: list of (numel, steps_done) or (numel, steps_done, (off_p, off_g, off_m, off_v)); offsets in floats from
    a 16-byte boundary.  numel 0: null data pointers, a step word of its own."""

    def __init__(self, tensors, seed, zero_g=True, state=None):
        self.spec = [(t[0], t[1], t[2] if len(t) > 2 else (0, 0, 0, 0)) for t in tensors]
        self.n = len(self.spec)
        self.where, parts, cursor = [], [], 0                                  # where[i] = 4 starts (p, g, m, v) or None
        for i, (numel, done, offs) in enumerate(self.spec):
            if numel == 0:
                self.where.append(None)
                continue
            data = state[i] if state is not None else A.rule_state(numel, done, seed + i, zero_g=zero_g)
            starts = []
            for arr, off in zip(data, offs):
                start = (cursor + 3) // 4 * 4 + 8 + off
                parts.append((start, np.ascontiguousarray(arr, dtype=np.float32)))
                starts.append(start)
                cursor = start + numel + 8
            self.where.append(starts)
        self.host = np.full((cursor + 3) // 4 * 4 + 8, SENTINEL, dtype=np.int32)
        for start, arr in parts:
            self.host[start:start + arr.size] = arr.view(np.int32)
        self.written = np.zeros(self.host.size, dtype=bool)                   # the words a launch may change
        for i, w in enumerate(self.where):
            if w is not None:
                for k in (0, 2, 3):
                    self.written[w[k]:w[k] + self.spec[i][0]] = True
        self.reset()

    def reset(self):
        self.arena = torch.from_numpy(self.host.copy()).to(DEV)
        assert self.arena.data_ptr() % 16 == 0
        steps = [GUARD] + [s[1] for s in self.spec] + [GUARD]
        self.steps = torch.tensor(steps, dtype=torch.int64, device=DEV)

    def state(self, words, i):
        """(p, g, m, v) float32 of tensor i from a copy of the arena."""
        return tuple(words[s:s + self.spec[i][0]].view(np.float32) for s in self.where[i])

    def args(self, numel=None, null=None):
        base, sbase = self.arena.data_ptr(), self.steps.data_ptr()
        cols = []
        for k in range(4):
            ptrs = [None if w is None else base + 4 * w[k] for w in self.where]
            if null is not None and null[0] == k:
                ptrs[null[1]] = None
            cols.append((C.c_void_p * self.n)(*ptrs))
        steps = [sbase + 8 * (1 + i) for i in range(self.n)]
        if null is not None and null[0] == 4:
            steps[null[1]] = None
        numel = [s[0] for s in self.spec] if numel is None else numel
        return [self.n] + cols + [(C.c_int64 * self.n)(*numel), (C.c_void_p * self.n)(*steps)]


def _ticket():
    return torch.zeros(528, dtype=torch.int64, device=DEV)


def _call(case, ticket, hyper, **kw):
    from tip_amd._lib import lib, stream_ptr
    a = case.args(**kw)
    status = lib().tipk_adam_step(*a, C.c_void_p(ticket.data_ptr()) if ticket is not None else None, hyper['lr'],
                                  hyper['beta1'], hyper['beta2'], hyper['eps'], hyper['weight_decay'], stream_ptr(DEV))
    torch.cuda.synchronize()
    return status


def _step(case, ticket, hyper, what='', values=True):
    """One launch, everything checked -> the arena after it (int32 words).  values=False: all but the comparison with the
    spec (for a run that is then compared bitwise with one that was)."""
    before = case.arena.cpu().numpy()
    counts = case.steps.cpu().tolist()
    assert _call(case, ticket, hyper) == 0, what
    after = case.arena.cpu().numpy()
    assert np.array_equal(after[~case.written], before[~case.written]), (what, 'a word outside parameters and moments changed',
                                                                         np.flatnonzero((after != before) & ~case.written)[:8])
    assert not bool(ticket.any()), (what, 'ticket left non-zero', torch.nonzero(ticket).flatten()[:8].tolist())
    expect = [GUARD] + [c + (1 if case.spec[i][0] > 0 else 0) for i, c in enumerate(counts[1:-1])] + [GUARD]
    assert case.steps.cpu().tolist() == expect, (what, 'step words')
    for i, (numel, _, _) in enumerate(case.spec):
        if numel == 0 or not values:
            continue
        t = counts[1 + i] + 1
        st = case.state(before, i)
        got = case.state(after, i)
        _note(A.check((got[0], got[2], got[3]), st, t, hyper, what=(what, 'tensor %d' % i, 'numel %d' % numel, 't %d' % t)))
        if hyper['weight_decay'] == 0.0:                                        # (with decay g' = wd p moves such an element)
            p, g, m, v = st
            still = (g == 0) & (m == 0) & (v == 0)
            assert np.array_equal(got[0][still].view(np.int32), p[still].view(np.int32)), (what, i, 'g = m = v = 0 moved p')
        if hyper['lr'] == 0.0:
            assert np.array_equal(got[0].view(np.int32), st[0].view(np.int32)), (what, i, 'lr = 0 moved p')
    return after


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('done', A.STEPS_DONE)
@pytest.mark.parametrize('name', list(A.HYPER))
def test_rule(name, done):
    """n = 5000 (vector path, 5 workgroups, a tail); 2^33 + 4 steps done catches a count read as 32 bits."""
    case = Case([(5000, done)], seed=1000 + 17 * A.STEPS_DONE.index(done), zero_g=name != 'eps_0')
    p, g, m, v = case.state(case.host, 0)
    if name != 'eps_0':
        assert ((g == 0) & (m == 0) & (v == 0)).sum() >= 5000 // 14
    _step(case, _ticket(), A.HYPER[name], what=(name, done))


# ------------------------------------------------------------------------------------------------ grid and ticket
def _grid_list(w):
    if w == 1:
        return [700]
    if w == 2:
        return [1, 1023]
    if w <= 33:
        return [3] * (w - 3) + [1, 2047]                                       # one workgroup each, the last one two
    if w <= 65:
        return [7] * 40 + [(w - 40) * 1024 - 5]
    return [1, (w - 2) * 1024 - 3, 1023]


@pytest.mark.parametrize('w', [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025])
def test_grid_and_ticket(w):
    """Workgroup totals around the ticket's group size (wg mod 32) and its multiples: three launches in a row on one
    ticket (a ticket left non-zero corrupts the NEXT launch's count), each inside the bounds; a second run is bitwise equal."""
    numels = _grid_list(w)
    assert sum(-(-n // 1024) for n in numels) == w and len(numels) <= 48
    case = Case([(n, 2 * i) for i, n in enumerate(numels)], seed=w)
    ticket, hyper = _ticket(), A.HYPER['default']
    runs = []
    for run in range(2):
        case.reset()
        runs.append([_step(case, ticket, hyper, what=('grid', w, 'run', run, 'launch', k), values=run == 0) for k in range(3)])
        assert case.steps.cpu().tolist()[1:-1] == [2 * i + 3 for i in range(len(numels))]
    for a, b in zip(*runs):
        assert np.array_equal(a, b), ('grid', w, 'two runs differ')


# ------------------------------------------------------------------------------------------------ tensor boundaries
def test_tensor_boundaries_each_tensor_its_own_step_count():
    numels = [1, 1024, 1025, 3, 2048, 1, 4097, 2, 4, 5, 1023]
    case = Case([(n, 3 * i) for i, n in enumerate(numels)], seed=77)
    _step(case, _ticket(), A.HYPER['default'], what='boundaries')
    # the bias corrections of neighbouring tensors differ by far more than the bound: a workgroup that took its
    # neighbour's count cannot pass (tensor 1: t = 4 against t = 1 or 7)
    st = case.state(case.host, 1)
    a, b = (A.adam_step64(*st, t, **A.HYPER['default'])[0] for t in (4, 7))
    assert (np.abs(a - b) > 100 * A.adam_bounds(*st, 4, **A.HYPER['default'])[0]).mean() > 0.5


# ------------------------------------------------------------------------------------------------ list length
@pytest.mark.parametrize('count_empties', [False, True], ids=['live', 'total'])
@pytest.mark.parametrize('length', [47, 48, 49, 96, 97])
def test_list_length_and_empty_tensors(length, count_empties):
    """47 / 48 / 49 / 96 / 97 tensors (48 per launch), numels cycling 1 ... 9, with numel == 0 entries (null data
    pointers) first, in the middle, at position 48 and last.  `length` counts the tensors that have elements ('live') or
    all entries ('total')."""
    def empties(total):
        return {0, total // 2, total - 1} | ({48} if total > 48 else set())
    total = length if count_empties else next(t for t in range(length, length + 5) if t - len(empties(t)) == length)
    live = iter(range(total))
    numels = [0 if i in empties(total) else 1 + next(live) % 9 for i in range(total)]
    assert len(numels) == total and sum(n > 0 for n in numels) == (length if not count_empties else total - len(empties(total)))
    case = Case([(n, i % 5) for i, n in enumerate(numels)], seed=length)
    ticket = _ticket()
    for k in range(2):                                                         # (_step: empties stay, all others +1)
        _step(case, ticket, A.HYPER['decay'], what=('list', length, count_empties, k))


def test_list_of_only_empty_tensors():
    case = Case([(0, 5), (0, 0), (0, 9)], seed=1)
    extra = Case([(5, 3)], seed=2)                                             # something to be left untouched
    ticket = _ticket()
    before, counts = extra.arena.cpu().numpy(), case.steps.cpu().tolist()
    assert _call(case, ticket, A.HYPER['default']) == 0
    assert case.steps.cpu().tolist() == counts and not bool(ticket.any())
    assert np.array_equal(extra.arena.cpu().numpy(), before)


# ------------------------------------------------------------------------------------------------ alignment
def test_misaligned_pointers_take_the_scalar_path():
    """torch never hands out a pointer that is not 16-byte aligned: here each of p, g, m, v in turn starts 1, 2, 3 floats
    past a 16-byte boundary while the other three stay aligned, then all four start 1 past."""
    variants = [tuple(off if k == which else 0 for k in range(4)) for which in range(4) for off in (1, 2, 3)] + [(1, 1, 1, 1)]
    ticket = _ticket()
    for offs in variants:
        case = Case([(n, 6, offs) for n in (1, 3, 4, 5, 1027)], seed=sum(o << (2 * k) for k, o in enumerate(offs)))
        for i, w in enumerate(case.where):
            assert tuple((case.arena.data_ptr() + 4 * s) % 16 // 4 for s in w) == offs
        _step(case, ticket, A.HYPER['decay'], what=('offsets', offs))


# ------------------------------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize('name', ['default', 'decay'])
def test_non_finite_gradients_stay_where_they_are(name):
    """inf, -inf and NaN at isolated positions -- 1 and 2 of a float4, the last element of a tensor, one of a scalar-path
    tail: the NaN / inf masks of p, m, v are the rule's (adam_spec.check) and every neighbour stays inside its bound."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    plan = [(2051, (0, 0, 0, 0), {1: inf, 2: -inf, 9: nan, 14: -inf, 1030: nan, 2049: inf, 2050: nan}),
            (1027, (0, 0, 0, 0), {1: nan, 6: inf, 1026: -inf}),
            (9, (0, 1, 0, 0), {2: inf, 8: nan})]
    state = []
    for i, (n, _, where) in enumerate(plan):
        p, g, m, v = A.rule_state(n, 6, 500 + i)
        assert np.abs(g).max() < 1e15
        for pos, val in where.items():
            g[pos] = val
        state.append((p, g, m, v))
    case = Case([(n, 6, offs) for n, offs, _ in plan], seed=0, state=state)
    after = _step(case, _ticket(), A.HYPER[name], what=('non-finite', name))
    for i, (n, _, where) in enumerate(plan):
        got = case.state(after, i)
        hit = np.zeros(n, dtype=bool)
        hit[list(where)] = True
        for arr in (got[0], got[2], got[3]):
            assert np.array_equal(~np.isfinite(arr), hit)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_untouched():
    case = Case([(5, 3), (1030, 4)], seed=3)
    ticket = _ticket()
    ticket[7] = 5                                                              # (any change of the ticket would show)
    before, counts, tk = case.arena.cpu().numpy(), case.steps.cpu().tolist(), ticket.cpu().tolist()
    ok = A.HYPER['decay']
    calls = [('beta1 = 1', dict(ok, beta1=1.0), {}), ('beta2 = 1', dict(ok, beta2=1.0), {}),
             ('beta1 < 0', dict(ok, beta1=-0.1), {}), ('beta2 < 0', dict(ok, beta2=-1e-9), {}),
             ('lr < 0', dict(ok, lr=-0.01), {}), ('lr = NaN', dict(ok, lr=float('nan')), {}),
             ('eps < 0', dict(ok, eps=-1e-8), {}), ('null ticket', ok, {'ticket': None}),
             ('negative numel', ok, {'numel': [5, -1]}), ('negative numel first', ok, {'numel': [-5, 1030]})]
    calls += [('null pointer %d of tensor %d' % (k, i), ok, {'null': (k, i)}) for k in range(5) for i in range(2)]
    for what, hyper, kw in calls:
        tkt = kw.pop('ticket', ticket)
        assert _call(case, tkt, hyper, **kw) == EINVAL, what
        assert np.array_equal(case.arena.cpu().numpy(), before), what
        assert case.steps.cpu().tolist() == counts and ticket.cpu().tolist() == tk, what


# ------------------------------------------------------------------------------------------------ through tip_amd.optim.Adam
def _host(t):
    return t.detach().cpu().numpy().copy()


def _optim_state(opt, p):
    """(p, g, m, v) on the host and the steps done, before a step (no state yet: zeros, 0)."""
    st = opt.state.get(p)
    if not st:
        z = np.zeros(p.numel(), dtype=np.float32)
        return (_host(p).ravel(), _host(p.grad).ravel(), z, z.copy()), 0
    return (_host(p).ravel(), _host(p.grad).ravel(), _host(st['exp_avg']).ravel(), _host(st['exp_avg_sq']).ravel()), int(st['step'])


def _optim_check(opt, p, before, done, hyper, what):
    st = opt.state[p]
    assert int(st['step']) == done + 1, what
    got = (_host(p).ravel(), _host(st['exp_avg']).ravel(), _host(st['exp_avg_sq']).ravel())
    _note(A.check(got, before, done + 1, hyper, what=what))


def _params(numels, seed):
    ps = []
    for i, n in enumerate(numels):
        ps.append(torch.nn.Parameter(torch.from_numpy(A.rule_state(n, 0, seed + i)[0]).to(DEV)))
    return ps


def _feed(ps, seed, skip=lambda i: False):
    for i, p in enumerate(ps):
        p.grad = None if skip(i) else torch.from_numpy(A.rule_state(p.numel(), 0, seed + i)[1]).to(DEV)


def _hyper_of(group):
    return dict(lr=group['lr'], beta1=group['betas'][0], beta2=group['betas'][1], eps=group['eps'],
                weight_decay=group['weight_decay'])


def test_optim_two_param_groups_share_the_ticket():
    from tip_amd.optim import Adam
    a, b = _params([1030, 3, 2048], 10), _params([5, 1025], 20)
    opt = Adam([dict(params=a, lr=0.01), dict(params=b, lr=0.003, betas=(0.8, 0.99), weight_decay=0.01, eps=1e-6)])
    for k in range(3):
        _feed(a + b, 100 * k)
        before = {p: _optim_state(opt, p) for p in a + b}
        opt.step()
        torch.cuda.synchronize()
        for group in opt.param_groups:
            for p in group['params']:
                _optim_check(opt, p, *before[p], _hyper_of(group), ('groups', k, p.numel()))
    assert len(opt._tickets) == 1 and not bool(opt._tickets[torch.device(DEV)].any())


def test_optim_300_parameters_second_counter_block():
    """More than 256 parameters: the counters of the last 44 live in a second block.  Every third parameter has no gradient
    on the second step: counts 1 or 2, values with the right t."""
    from tip_amd.optim import Adam
    ps = _params([1 + i % 5 for i in range(300)], 3000)
    opt = Adam(ps, lr=0.02, weight_decay=0.01)
    hyper = _hyper_of(opt.param_groups[0])
    for k in range(2):
        skip = (lambda i: i % 3 == 0) if k == 1 else (lambda i: False)
        _feed(ps, 5000 + 1000 * k, skip)
        before = {p: _optim_state(opt, p) for i, p in enumerate(ps) if not skip(i)}
        frozen = {p: (_host(p), _host(opt.state[p]['exp_avg']), _host(opt.state[p]['exp_avg_sq']))
                  for i, p in enumerate(ps) if skip(i)}
        opt.step()
        torch.cuda.synchronize()
        for p, (st, done) in before.items():
            _optim_check(opt, p, st, done, hyper, ('300', k))
        for p, (p0, m0, v0) in frozen.items():
            assert int(opt.state[p]['step']) == 1
            assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in
                       ((_host(p), p0), (_host(opt.state[p]['exp_avg']), m0), (_host(opt.state[p]['exp_avg_sq']), v0)))
    assert [int(opt.state[p]['step']) for p in ps] == [1 if i % 3 == 0 else 2 for i in range(300)]
    blocks = {opt.state[p]['step'].untyped_storage().data_ptr() for p in ps}
    assert len(blocks) == 2
    assert not bool(opt._tickets[torch.device(DEV)].any())


def test_optim_graph_of_61_tensors_replayed():
    """61 tensors: two launches in one captured graph (a side stream, as the graph test of test_gpu_optim.py captures);
    three replays with new gradients in the same storage: counts + 3, every replay inside the bounds."""
    from tip_amd.optim import Adam
    ps = _params([17 + i for i in range(60)] + [5000], 7000)
    opt = Adam(ps, lr=0.01)
    hyper = _hyper_of(opt.param_groups[0])
    _feed(ps, 8000)
    grads = [p.grad for p in ps]
    opt.step()                                                                 # allocates the state, outside the graph
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    assert all(int(opt.state[p]['step']) == 1 for p in ps)                     # capture executes nothing
    for k in range(3):
        for i, gr in enumerate(grads):
            gr.copy_(torch.from_numpy(A.rule_state(gr.numel(), 0, 9000 + 100 * k + i)[1]))
        before = {p: _optim_state(opt, p) for p in ps}
        graph.replay()
        torch.cuda.synchronize()
        for p in ps:
            assert before[p][1] == 1 + k
            _optim_check(opt, p, *before[p], hyper, ('graph', k, p.numel()))
    assert all(int(opt.state[p]['step']) == 4 for p in ps)
    assert not bool(opt._tickets[torch.device(DEV)].any())
