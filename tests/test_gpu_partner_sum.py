"""-m gpu: the partner sum (include/tipk.h section 4l, tip_amd/csrc/tipk_partner_sum.hip) against the fp64 spec and the
acceptance rule of tests/partner_sum_spec.py -- every result of every test is held to the rule.  The kernel's contract is
tested through the C entries themselves (`_raw`: the lists as given, forward keys only); `ops.*_partner_sum` (which mirrors
the lists) and `TIP.drug_profile` on top."""
import os

import pytest
import torch

import partner_sum_cases as cases
from partner_rank_cases import known_from_dict
from partner_sum_spec import check_partner_sum, expected_top
from tip_amd import _lib, ops
from tip_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(c):
    """A case of partner_sum_cases on the device."""
    known = None if c['known'] is None else tuple(t.to(DEV) for t in c['known'])
    m = c['model']
    out = dict(c, model=(m[0], m[1].to(DEV), m[2].to(DEV)), known=known)
    for name in ('q_drug', 'rel_ids', 'partner_w'):
        out[name] = None if c[name] is None else c[name].to(DEV)
    return out


def _raw(model, q_drug, k, rel_ids=None, partner_w=None, known=None):
    """The C entry on device tensors, the known lists exactly as given -> (sum, count, top_val, top_pos)."""
    kind, a, b = model
    L = _lib.lib()
    qd = q_drug.to(torch.int32).contiguous()
    rel = None if rel_ids is None else rel_ids.to(torch.int32).contiguous()
    pw = None if partner_w is None else partner_w.to(torch.float32).contiguous()
    keys = kptr = None
    if known is not None and known[0].numel():
        keys, kptr = known[0].to(torch.int64).contiguous(), known[1].to(torch.int64).contiguous()
    n_rel = b.shape[0]
    n_q, n_sel = qd.numel(), (n_rel if rel is None else rel.numel())
    out_sum = torch.full((n_q, n_sel), -7.0, dtype=torch.float32, device=DEV)
    out_cnt = torch.full((n_q, n_sel), -7, dtype=torch.int32, device=DEV)
    top_v = torch.full((n_q, k), -7.0, dtype=torch.float32, device=DEV)
    top_p = torch.full((n_q, k), -7, dtype=torch.int32, device=DEV)
    if kind == 'distmult':
        a, b = a.contiguous(), b.contiguous()
        st = L.tipk_distmult_partner_sum(ptr(a), a.shape[0], a.shape[1], ptr(b), n_rel, ptr(qd), n_q, ptr(rel), n_sel, ptr(pw),
                                         ptr(keys), ptr(kptr), k, ptr(out_sum), ptr(out_cnt), ptr(top_v), ptr(top_p),
                                         stream_ptr(DEV))
    else:
        assert a.stride(0) == b.stride(0) and a.stride(1) == 1
        st = L.tipk_pair_table_partner_sum(ptr(a), ptr(b), a.stride(0), a.shape[1], n_rel, ptr(qd), n_q, ptr(rel), n_sel,
                                           ptr(pw), ptr(keys), ptr(kptr), k, ptr(out_sum), ptr(out_cnt), ptr(top_v),
                                           ptr(top_p), stream_ptr(DEV))
    _lib.check(st, 'partner sum')
    torch.cuda.synchronize()
    return out_sum, out_cnt, top_v, top_p


def _run_case(c, k, what):
    c = _dev(c)
    got = _raw(c['model'], c['q_drug'], k, c['rel_ids'], c['partner_w'], c['known'])
    t = check_partner_sum(c['model'], c['q_drug'], k, got, c['rel_ids'], c['partner_w'], c['known'], what=what)
    return c, got, t


def _same(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('n', cases.SMALL_N)
@pytest.mark.parametrize('kind,dim', [('distmult', d) for d in cases.SMALL_DIM] + [('table', 0)])
def test_small_shapes(kind, dim, n):
    for col_mode in ('all', 'subset', 'repeats'):
        c, got, t = _run_case(cases.small_case(kind, n, dim, col_mode), 10, 'small %s n%d dim%d %s' % (kind, n, dim, col_mode))
        q = c['q_drug']
        outside = (q < 0) | (q >= n)
        assert bool(torch.isnan(got[0][outside]).all()) and bool((got[1][outside] == 0).all())
        assert bool((got[3][outside] == -1).all())                        # a row of NaN cells selects nothing
        if n == 1:
            assert bool((got[0][~outside] == 0).all() | torch.isnan(got[0][~outside]).any())


@pytest.mark.parametrize('kind', cases.KINDS)
def test_every_column_count(kind):
    """Every n_sel around the kernel's block of columns, and 63, 64, 65, 257; k walks through 0, 1, 10, 128 and n_sel + 3."""
    for i, n_sel in enumerate(cases.SEL_COUNTS):
        k = (0, 1, 10, 128, n_sel + 3)[i % 5]
        c, got, t = _run_case(cases.sel_case(kind, n_sel), min(k, 128), 'columns %s S%d k%d' % (kind, n_sel, k))
        assert got[0].shape == (9, n_sel)
        if n_sel >= 4:                                                    # the column out of range: NaN, 0, never selected
            assert bool(torch.isnan(got[0][:, 2]).all()) and bool((got[1][:, 2] == 0).all()) and not bool((got[3] == 2).any())


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('n_q', cases.QUERY_COUNTS)
def test_query_counts_and_k(kind, n_q):
    for k in (0, 1, 10, 128, cases.R + 3):
        c = cases.small_case(kind, 65, 16, 'all', 'zeros', n_q=n_q)
        c, got, t = _run_case(c, k, 'queries %s Q%d k%d' % (kind, n_q, k))
        assert got[0].shape == (n_q, cases.R) and got[2].shape == (n_q, k)
        if k > cases.R and n_q:
            assert bool((got[3][:, cases.R:] == -1).all()) and bool(torch.isinf(got[2][:, cases.R:]).all())


# ------------------------------------------------------------------ known lists and weights
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('how', ['none', 'symmetric', 'one_way', 'every', 'self'])
def test_known_lists(kind, how):
    c, got, t = _run_case(cases.known_case(kind, how), 5, 'known %s %s' % (kind, how))
    n = 130
    if how == 'none':
        assert bool((got[1] == n - 1).all())
    if how == 'every':
        assert float(got[0][5, 1]) == 0.0 and int(got[1][5, 1]) == 0      # no candidates: exactly 0
        assert int(got[1][6, 2]) == n - 1                                 # reverse keys alone drop nothing
    if how == 'one_way':                                                  # only the listed direction is dropped ...
        keys, kptr = c['known']
        dropped = ((n - 1) - got[1][:n].long()).sum()                      # every key u*n+v takes one candidate off one cell
        assert int(dropped) == keys.numel() and int(got[1][int(keys[0]) // n, 0]) < n - 1
        # ... and the ops drop both: their lists are mirrored
        args = (c['model'][1], c['model'][2], c['q_drug'], 5, None, None, c['known'])
        both = ops.distmult_partner_sum(*args) if kind == 'distmult' else ops.pair_table_partner_sum(*args)
        torch.cuda.synchronize()
        mirrored = ops.symmetric_known(c['known'], n)
        check_partner_sum(c['model'], c['q_drug'], 5, both, known=mirrored, what='ops mirrored %s' % kind)
        assert int(((n - 1) - both[1][:n].long()).sum()) == mirrored[0].numel() == 2 * keys.numel()
    if how == 'self':
        bare = cases.known_case(kind, 'self')
        keys, kptr = bare['known']
        d = {}
        for r in range(kptr.numel() - 1):
            d[r] = [(int(x) // n, int(x) % n) for x in keys[kptr[r]:kptr[r + 1]] if int(x) // n != int(x) % n]
        no_self = _dev(dict(bare, known=known_from_dict(d, n, kptr.numel() - 1)))
        assert _same(got, _raw(no_self['model'], no_self['q_drug'], 5, None, None, no_self['known']))


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('w_mode', ['none', 'zeros', 'all_zero'])
def test_weights(kind, w_mode):
    c, got, t = _run_case(cases.small_case(kind, 130, 16, 'all', w_mode, n_q=40), 3, 'weights %s %s' % (kind, w_mode))
    if w_mode == 'all_zero':
        inside = (c['q_drug'] >= 0) & (c['q_drug'] < 130)
        assert bool((got[0][inside] == 0).all()) and bool((got[1] == 0).all())
        assert got[3][inside][0].tolist() == [0, 1, 2]                    # exact ties: by position


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize('kind', cases.KINDS)
def test_nan_row_poisons_exactly_its_cells(kind):
    """Drug 9 has a NaN embedding (table: NaN partner scores).  It poisons every cell where it is a candidate -- not where its
    weight is 0, not where it is recorded, not its own row's other partners' sums beyond what the contract says."""
    n, n_rel = 65, 5
    c = cases.small_case(kind, n, 16, 'all', 'none', n_q=0, n_rel=n_rel)
    m = c['model']
    if kind == 'distmult':
        z = m[1].clone()
        z[9] = float('nan')
        m = (kind, z, m[2])
    else:
        s2 = m[2].clone()
        s2[:, 9] = float('nan')
        m = (kind, m[1], s2)
    q = torch.arange(n)
    d = {0: [(u, 9) for u in range(0, n, 2)], 3: [(9, u) for u in range(n)]}   # relation 0: recorded for even u; 3: reverse only
    known = known_from_dict(d, n, n_rel)
    c = _dev(dict(model=m, q_drug=q, rel_ids=None, partner_w=None, known=known))
    got = _raw(c['model'], c['q_drug'], 5, None, None, c['known'])
    check_partner_sum(c['model'], c['q_drug'], 5, got, known=c['known'], what='nan row %s' % kind)
    nan = torch.isnan(got[0])
    rows = torch.arange(n, device=DEV)
    odd, others = rows % 2 == 1, rows != 9
    assert torch.equal(nan[others][:, 0], odd[others])                    # relation 0: recorded for the even drugs
    assert bool(nan[others][:, 1:].all())                                 # relation 3's reverse keys do not take it out
    if kind == 'distmult':                                                # its own logits are all NaN; relation 3 has no candidate
        assert bool(nan[9, [0, 1, 2, 4]].all()) and float(got[0][9, 3]) == 0.0 and int(got[1][9, 3]) == 0
    else:
        assert not bool(nan[9].any())                                     # the table's NaN is the partner's score only
    even = others & ~odd                                                  # NaN cells are never selected
    assert bool((got[3][even][:, 0] == 0).all()) and bool((got[3][even][:, 1:] == -1).all())
    assert bool((got[3][others & odd] == -1).all())
    pw = torch.ones(n, device=DEV)
    pw[9] = 0.0
    got = _raw(c['model'], c['q_drug'], 5, None, pw, c['known'])
    check_partner_sum(c['model'], c['q_drug'], 5, got, partner_w=pw, known=c['known'], what='nan row w0 %s' % kind)
    assert not bool(torch.isnan(got[0][others]).any())                    # weight 0: skipped, not multiplied


def test_infinite_logits():
    """Table scores of +-inf: sigma is exactly 1 or 0, the cell exactly the weights of the +inf partners plus the rest."""
    g = torch.Generator().manual_seed(8)
    n, n_rel = 70, 3
    s1 = torch.randn(n_rel, n, generator=g)
    s2 = torch.randn(n_rel, n, generator=g)
    s2[0, 5::7] = float('inf')
    s2[1, 3::5] = float('-inf')
    s2[2, :] = float('inf')
    s2[2, 1::2] = float('-inf')
    pw = cases.weights(n, 'zeros', g)
    m = ('table', s1.to(DEV), s2.to(DEV))
    q = torch.arange(n, device=DEV)
    got = _raw(m, q, 3, None, pw.to(DEV))
    check_partner_sum(m, q, 3, got, partner_w=pw.to(DEV), what='inf table')
    want = torch.stack([pw[0::2].sum() - (pw[u] if u % 2 == 0 else 0) for u in range(n)])    # exact only up to the sum order
    assert bool(((got[0][:, 2].cpu() - want).abs() <= 1e-5 * want.abs()).all())
    one = torch.zeros(n)
    one[4] = 2.5
    got = _raw(m, q, 0, None, one.to(DEV))
    assert got[0][:, 2].cpu().tolist() == [0.0 if u == 4 else 2.5 for u in range(n)]   # +inf contributes exactly the weight
    # DistMult: products that overflow to +-inf in fp32
    z = torch.randn(20, 4, generator=g)
    z[3] = 3e19
    z[4] = -3e19
    w = torch.rand(2, 4, generator=g) + 0.5
    m = ('distmult', z.to(DEV), w.to(DEV))
    q = torch.tensor([3, 4, 0], device=DEV)
    got = _raw(m, q, 2)
    check_partner_sum(m, q, 2, got, what='inf distmult')


@pytest.mark.parametrize('kind', cases.KINDS)
def test_exact_ties_by_position(kind):
    """Repeated columns are the same cell bit for bit: the selection lists them by position."""
    c = _dev(cases.small_case(kind, 65, 16, 'all', 'none', n_q=12, n_rel=4))
    rel = torch.tensor([2, 0, 2, 3, 2, 0, 1, 2], device=DEV)
    got = _raw(c['model'], c['q_drug'], 8, rel, None, c['known'])
    check_partner_sum(c['model'], c['q_drug'], 8, got, rel_ids=rel, known=c['known'], what='ties %s' % kind)
    inside = (c['q_drug'] >= 0) & (c['q_drug'] < 65)
    S = got[0][inside]
    assert torch.equal(S[:, 0], S[:, 2]) and torch.equal(S[:, 2], S[:, 4]) and torch.equal(S[:, 4], S[:, 7])
    for row in got[3][inside].tolist():
        twos = [p for p in row if p in (0, 2, 4, 7)]
        assert twos == [0, 2, 4, 7] and [p for p in row if p in (1, 5)] == [1, 5]


# ------------------------------------------------------------------ routes, repeatability
@pytest.mark.parametrize('n,dim', cases.ROUTES)
def test_routes(n, dim):
    route = _lib.lib().tipk_distmult_partner_sum_lds_route
    assert route(n, dim) == (0 if n == 2600 else 1)
    c, got, t = _run_case(cases.routes_case(n, dim), 3, 'route n%d dim%d' % (n, dim))
    again = _raw(c['model'], c['q_drug'], 3, c['rel_ids'], c['partner_w'], c['known'])
    assert _same(got, again)                                              # two calls give equal bits
    if (n, dim) == (700, 16):
        assert _lib.get_option('partner_sum_global') == 0
        _lib.set_option('partner_sum_global', 1)
        try:
            assert route(n, dim) == 0
            forced = _raw(c['model'], c['q_drug'], 3, c['rel_ids'], c['partner_w'], c['known'])
        finally:
            _lib.set_option('partner_sum_global', 0)
        assert _same(got, forced)                                         # the two routes agree to the bit
        check_partner_sum(c['model'], c['q_drug'], 3, forced, c['rel_ids'], c['partner_w'], c['known'], what='route global')


@pytest.mark.parametrize('kind', cases.KINDS)
def test_repeatable(kind):
    c = _dev(cases.small_case(kind, 130, 16, 'repeats', 'zeros', n_q=300))
    a = _raw(c['model'], c['q_drug'], 10, c['rel_ids'], c['partner_w'], c['known'])
    b = _raw(c['model'], c['q_drug'], 10, c['rel_ids'], c['partner_w'], c['known'])
    assert _same(a, b)
    args = (c['model'][1], c['model'][2], c['q_drug'], 10, c['rel_ids'], c['partner_w'], c['known'])
    via_ops = ops.distmult_partner_sum(*args) if kind == 'distmult' else ops.pair_table_partner_sum(*args)
    torch.cuda.synchronize()
    assert _same(a, via_ops)                                              # symmetric lists: the ops pass them on as they are


# ------------------------------------------------------------------ BioSNAP size
@pytest.mark.parametrize('kind', cases.KINDS)
def test_biosnap_size(kind):
    c, got, t = _run_case(cases.biosnap_case(kind), 10, 'biosnap %s' % kind)
    assert got[0].shape == (64, 1097) and int(got[1].min()) > 600 and int(got[1].max()) <= 644
    assert not bool(torch.isnan(got[0]).any())


# ------------------------------------------------------------------ TIP.drug_profile
def _model_of(model, z):
    dec = model.decoder
    if model.decoder_kind == 'distmult':
        return ('distmult', z, dec.weight.detach())
    with torch.no_grad():                                                 # the tables as NNDecoder.objective forms them
        s1t = ops.matmul(dec.w1_l2, torch.relu(ops.matmul(z, dec.w1_l1)).t())
        s2t = ops.matmul(dec.w2_l2, torch.relu(ops.matmul(z, dec.w2_l1)).t())
    return ('table', s1t, s2t)


def _pairs_of(idx, rng, d=None):
    d = {} if d is None else d
    idx = idx.cpu().tolist()
    for r, (a, b) in enumerate(torch.as_tensor(rng).long().tolist()):
        d.setdefault(r, [])
        d[r] += [(u, v) for u, v in zip(idx[0][a:b], idx[1][a:b])] + [(v, u) for u, v in zip(idx[0][a:b], idx[1][a:b])]
    return d


@pytest.mark.parametrize('decoder', ['distmult', 'nn'])
def test_tip_drug_profile(decoder):
    from conftest import GOLDEN
    from tip_amd.layers import TIP, DrugProfile, Setting
    torch.manual_seed(0)
    st = Setting(sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32)
    model = TIP(st, torch.device(DEV), data_path=os.path.join(GOLDEN, 'data_dict_small.pkl'), decoder=decoder)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z = model.embeddings.detach()
    m = _model_of(model, z)
    train = _pairs_of(d.dd_train_idx, d.dd_train_range)
    both = _pairs_of(d.dd_test_idx, d.dd_test_range, _pairs_of(d.dd_train_idx, d.dd_train_range))
    lists = {None: None, 'train': known_from_dict(train, n, R), 'all': known_from_dict(both, n, R)}
    all_drugs = torch.arange(n, device=DEV)
    g = torch.Generator().manual_seed(6)
    k = 4

    def held(res, model_t, q, rel, pw, known, what):
        assert isinstance(res, DrugProfile) and res.candidates.dtype == torch.int64 and res.top_relation.dtype == torch.int64
        rel_t = None if rel is None else torch.as_tensor(rel, device=DEV)
        known = None if known is None else tuple(t.to(DEV) for t in known)
        kk = res.top_expected.shape[1]
        want_p = expected_top(res.expected, kk)[1]                        # positions; the method returns global ids
        ids = want_p if rel is None else torch.where(want_p >= 0, rel_t[want_p.clamp(min=0)], want_p)
        assert torch.equal(res.top_relation, ids), 'top_relation is not relations[position]'
        check_partner_sum(model_t, q, kk, (res.expected, res.candidates, res.top_expected, want_p), rel_t, pw, known, what=what)
        assert res.expected.shape == (q.numel(), R if rel is None else len(rel))

    for exclude in (None, 'train', 'all'):
        res = model.drug_profile(k=k, exclude=exclude)                     # drugs None: all training drugs
        held(res, m, all_drugs, None, None, lists[exclude], 'TIP %s %s' % (decoder, exclude))
    assert int(model.drug_profile(exclude='all').candidates.sum()) < int(model.drug_profile(exclude=None).candidates.sum())
    # against the composition from the decoder's own scores: every (u, c, r) triple, the mask, the sum
    res = model.drug_profile(k=0, exclude='all')
    assert res.top_expected.shape == (n, 0) and res.top_relation.shape == (n, 0)
    u = all_drugs.repeat_interleave(n * R)
    c = all_drugs.repeat_interleave(R).repeat(n)
    et = torch.arange(R, device=DEV).repeat(n * n)
    with torch.no_grad():
        score = model.decoder(z, torch.stack([u, c]), et).view(n, n, R).double()
    keys, kptr = (t.to(DEV) for t in lists['all'])
    rel_of = torch.repeat_interleave(torch.arange(R, device=DEV), kptr[1:] - kptr[:-1])
    free = torch.ones((n, n, R), dtype=torch.bool, device=DEV)
    free[torch.div(keys, n, rounding_mode='floor'), keys % n, rel_of] = False
    free[all_drugs, all_drugs] = False
    comp = (score * free).sum(1)
    assert torch.equal(free.sum(1), res.candidates)
    assert bool(((res.expected.double() - comp).abs() <= 1e-5 * comp.abs() + 1e-6).all())   # two fp32 routes of one model
    # relations (repeats, any order) and partner weights
    sub = [4, 1, 5, 1]
    pw = cases.weights(n, 'zeros', g)
    q = [3, 0, 3, n - 1]
    res = model.drug_profile(q, k=6, exclude='train', relations=sub, partner_weights=pw.tolist())
    held(res, m, torch.tensor(q, device=DEV), sub, pw.to(DEV), lists['train'], 'TIP %s subset' % decoder)
    assert bool((res.top_relation[:, 4:] == -1).all()) and set(res.top_relation[:, :4].reshape(-1).tolist()) <= set(sub)
    # new drugs: ids n + i query the folded-in rows; they are never partners
    targets = [[0, 1, 2], [], [5]]
    inter = [[(0, 1), (3, 2)], [(1, 0)], []]
    new = model.embed_new_drugs(targets, inter)
    z_ext = torch.cat([z, new.z])
    m_ext = _model_of(model, z_ext)
    q = [n + 1, 2, n, n + 2, 0]
    res = model.drug_profile(q, k=k, exclude='all', new=new, partner_weights=pw.tolist())
    wide = {r: [(a, b) for a, b in uv] for r, uv in both.items()}
    pw_ext = torch.cat([pw, torch.zeros(3)]).to(DEV)
    held(res, m_ext, torch.tensor(q, device=DEV), None, pw_ext, known_from_dict(wide, n + 3, R), 'TIP %s new' % decoder)
    res1 = model.drug_profile(q, k=k, exclude='all', new=new)
    ones_ext = torch.cat([torch.ones(n), torch.zeros(3)]).to(DEV)
    held(res1, m_ext, torch.tensor(q, device=DEV), None, ones_ext, known_from_dict(wide, n + 3, R), 'TIP %s new w1' % decoder)
    assert bool((res1.candidates[[0, 2, 3]] == n).all())                  # a new drug: every training drug, nothing recorded
    assert bool((res1.candidates[[1, 4]] <= n - 1).all())                 # a training drug: new drugs are no partners
    old = model.drug_profile([2, 0], k=k, exclude='all')
    assert _same((old.expected, old.candidates), (res1.expected[[1, 4]], res1.candidates[[1, 4]]))
