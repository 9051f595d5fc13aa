"""CPU checks of `tests/dense_cases.py`: every product takes the route written next to it (`tipk_gemm_route`, a pure host query), the
tables reach every body, buffer count and operand walk, the limits of the workgroup-split kernel are where the header puts them,
correct fp32 arithmetic stays inside every case's bound (so the reference alone does not consume it), and the operand builder's
guards and sentinels are really there."""
import ctypes

import pytest
import torch

import dense_cases as D
from tip_amd import _lib

ALL_GEMM = D.GEMM_CASES + D.GROUP_CASES + D.GROUP_SINGLES


def _route(desc, grouped=0):
    return _lib.lib().tipk_gemm_route(desc, int(grouped))


def test_abi_version_and_route_codes():
    assert _lib.ABI_VERSION == 30 and _lib.lib().tipk_abi_version() == 30
    codes = [D.BODY[k] for k in D.BODY]
    assert sorted(codes) == list(range(9)), 'nine distinct body codes'
    mask = D._C['ROUTE_BODY_MASK']
    flags = [D._C['ROUTE_TWO_BUFFERS'], D._C['ROUTE_A_KFAST'], D._C['ROUTE_B_KFAST']]
    assert all(c & mask == c for c in codes) and all(f & mask == 0 for f in flags) and len({*flags}) == 3


def test_case_ids_are_unique():
    ids = [c.cid for c in ALL_GEMM] + [c.cid for c in D.WG_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize('case', ALL_GEMM, ids=lambda c: c.cid)
def test_every_gemm_case_takes_its_route(case):
    t = D.build_gemm(case, 'cpu')
    with D.options(**case.opts):
        got = _route(t.job.desc, case.grouped)
    assert got == case.code, '%s: %s, written down: %s' % (case.cid, D.route_name(got), D.route_name(case.code))
    if case.k == 0 and case.m > 0:
        assert not t.job.desc.a and not t.job.desc.b, 'an empty-K operand is handed over as NULL'


def test_cases_cover_every_body_buffer_count_and_operand_walk():
    missing = []
    seen = {c.route for c in D.GEMM_CASES}
    for body in D.BODY:
        if body in D.TILED:
            for nbuf in ((1,) if body == 't128x128' else (1, 2)):            # 128 x 128 never has two buffers
                for akf in (0, 1):
                    for bkf in (0, 1):
                        if (body, nbuf, akf, bkf) not in seen:
                            missing.append((body, nbuf, akf, bkf))
        elif body != 'none' and (body,) not in seen:
            missing.append(body)
    assert ('none',) in {c.route for c in D.GROUP_CASES}
    assert not missing, missing
    # every k of the list under every tiled body that can have it, and the multi-tile single-buffer loop of 128 x 128
    for body in D.TILED:
        ks = {c.k for c in D.GEMM_CASES if c.route[0] == body}
        assert ks >= {0, 1, 31, 32, 33, 64, 70}, (body, sorted(ks))
    for body in D.BODY:
        if body != 'none':
            assert any(c.inf for c in D.GEMM_CASES if c.route[0] == body), 'no +inf case for ' + body
            assert any(c.integer for c in D.GEMM_CASES if c.route[0] == body), 'no integer case for ' + body
    # the bodies that load the last valid k again for the lanes past the end of k: a +inf exactly there, with a k tail
    for body in ('thin_k', 'thin_k4', 'thin_m', 'kk'):
        assert any(c.inf and D.inf_k(c.inf, c.k) == c.k - 1 and c.k % 32 for c in D.GEMM_CASES if c.route[0] == body), body
    assert any(c.inf == 'last' and c.k % 32 and c.k % 4 == 0 for c in D.WG_CASES) and any(c.inf == 'last' and c.k % 4 for c in D.WG_CASES)
    assert any(c.inf and c.ksplit > 1 for c in D.GEMM_CASES)


def test_route_honours_each_option():
    k4 = D.build_gemm(D.gemm_case('thin_k4_m256_n4096_k32'), 'cpu').job.desc
    kk = D.build_gemm(D.gemm_case('kk_m256_n1_k4096'), 'cpu').job.desc
    tm = D.build_gemm(D.gemm_case('thin_m_m32_n1024_k1024'), 'cpu').job.desc
    assert _route(k4) == D.BODY['thin_k4'] and _route(tm) == D.BODY['thin_m']
    assert _route(kk) == D.route_code(('t128x32', 2, 1, 1))
    with D.options(gemm_thin_k_narrow=1):
        assert _route(k4) == D.BODY['thin_k'] and _route(tm) == D.BODY['thin_m']
    with D.options(gemm_stream_kk=1):
        assert _route(kk) == D.BODY['kk'] and _route(k4) == D.BODY['thin_k4']
    with D.options(gemm_no_stream=1, gemm_stream_kk=1, gemm_thin_k_narrow=1):
        assert _route(k4) == D.route_code(('t64x64', 1, 1, 0))
        assert _route(kk) == D.route_code(('t128x32', 2, 1, 1))
        assert _route(tm) == D.route_code(('t32x128', 2, 1, 0))
    assert all(_lib.get_option(o) == 0 for o in D.OPTIONS), 'options restored'
    # a member of a grouped launch: thin-k runs tiled, 128 x 128 becomes 64 x 64, always two buffers
    assert _route(k4, 1) == D.route_code(('t64x64', 2, 1, 0)) and _route(tm, 1) == D.BODY['thin_m']
    big = D.build_gemm(D.gemm_case('t128x128_512_k32'), 'cpu').job.desc
    assert _route(big) == D.route_code(('t128x128', 1, 0, 1)) and _route(big, 1) == D.route_code(('t64x64', 2, 0, 1))


def test_route_returns_the_status_of_the_launch():
    d = D.build_gemm(D.gemm_case('t64x64_m64_n64_k32'), 'cpu').job.desc
    EINVAL, EUNSUPPORTED = -1, -2
    assert _route(None) == EINVAL

    def changed(**kw):
        c = _lib.GemmDesc()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for bad in (dict(m=-1), dict(k=-1), dict(batch=-1), dict(kbatch=0), dict(ksplit=0), dict(a=None), dict(b=None), dict(c=None),
                dict(ksplit=2, relu=1), dict(a_sm=-1), dict(b_sn=-1)):
        assert _route(changed(**bad)) == EINVAL, bad
    assert _route(changed(a_sm=1 << 24)) == EUNSUPPORTED
    assert _route(changed(batch=70000)) == EUNSUPPORTED                      # grid z
    assert _route(changed(k=0, a=None, b=None)) == D.route_code(('t64x64', 1, 1, 0)), 'k == 0 reads neither a nor b'
    assert _route(changed(k=0, c=None)) == EINVAL
    for empty in (dict(m=0), dict(n=0), dict(batch=0), dict(m=0, a=None, b=None, c=None)):
        assert _route(changed(**empty)) == D.BODY['none'], empty
    # the launch itself answers the same without touching a device where it refuses
    assert _lib.lib().tipk_gemm_f32(changed(ksplit=2, relu=1), None) == EINVAL
    assert _lib.lib().tipk_gemm_f32(changed(m=0), None) == 0


@pytest.mark.parametrize('case', D.WG_CASES, ids=lambda c: c.cid)
def test_workgroup_split_limits(case):
    """64 K tiles and 4096 output tiles are taken, 65 and 4097 are not (tipk_gemm_wg_group_supported: a host query)."""
    t = D.build_wg(case, 'cpu')
    assert (t.job is not None) == case.supported
    tiles = -(-case.m // 32) * -(-case.n // 32) * (1 if case.reduce else case.z)
    assert case.supported == (case.n_kt <= 64 and tiles <= 4096)


def test_workgroup_split_table_reaches_its_edges():
    assert {c.n_kt for c in D.WG_CASES if c.k2 == 0 and not c.reduce and c.z == 1} >= {1, 15, 16, 17, 32, 33, 63, 64, 65}
    assert {c.m for c in D.WG_CASES} >= {1, 31, 32, 33} and {c.n for c in D.WG_CASES} >= {1, 31, 32, 33}
    assert {c.k % 32 for c in D.WG_CASES if c.la == 'r' and c.lb == 'c' and c.k % 4 == 0} >= {4, 28}
    tiles = sorted(-(-c.m // 32) * -(-c.n // 32) for c in D.WG_CASES)[-2:]
    assert tiles == [4096, 4097]


@pytest.mark.parametrize('case', ALL_GEMM, ids=lambda c: c.cid)
def test_fp32_on_the_host_stays_inside_the_bound(case):
    t = D.build_gemm(case, 'cpu')
    want, mag = case.reference()
    assert t.kr == case.total_k() + t.job.n_slabs + 3
    if case.m == 0:
        return
    used = D.ratio(D.gemm_fp32(t), want, mag) / t.kr
    assert used <= 1.0, used
    if case.integer:
        assert torch.equal(D.gemm_fp32(t).double(), want)
    if case.inf:
        bad = ~torch.isfinite(want)
        expect = torch.zeros_like(bad)
        expect[case.m // 2, :] = True
        expect[:, case.n // 3] = True
        assert torch.equal(bad, expect), 'exactly one row and one column are non-finite'
        assert bool(torch.isinf(want[bad]).all()), 'the reference holds infinities there, no NaN'


@pytest.mark.parametrize('case', [c for c in D.WG_CASES if c.supported and c.m * c.n < 10000], ids=lambda c: c.cid)
def test_workgroup_split_fp32_on_the_host(case):
    v = case.values()
    want, mag = case.reference()
    p = torch.matmul(v['a'], v['b'])
    if case.reduce:
        p = p.sum(0)
    if case.k2:
        p = p + v['a2'] @ v['b2']
    p = case.alpha * p + (v['c_in'] if case.cin else 0.0)
    if case.relu:
        p = torch.relu(p)
    if case.gate:
        p = p * (v['gate'] > 0)
        closed = ~(v['gate'] > 0)
        assert bool(closed.any()) and bool((want[closed] == 0).all()) and bool((mag[closed] == 0).all())
    assert D.ratio(p, want, mag) / case.kr <= 1.0


def test_gate_values_hold_every_closed_kind():
    g = D.gate_values([33, 33], D._gen('gate'))
    flat = g.view(-1)
    assert bool(torch.isnan(flat).any()) and bool((flat == float('-inf')).any()) and bool((flat == float('inf')).any())
    zeros = flat[flat == 0]
    assert bool(torch.signbit(zeros).any()) and bool((~torch.signbit(zeros)).any()), '+0 and -0'
    assert bool((flat < 0).any()) and bool(((flat > 0) & (flat < 1e-20)).any())


@pytest.mark.parametrize('epi', range(len(D.EPILOGUES)))
@pytest.mark.parametrize('n_slabs', D.SLAB_COUNTS)
def test_slab_sum_fp32_on_the_host(n_slabs, epi):
    epi = D.EPILOGUES[epi]
    v = D.slab_values(n_slabs, 5, 13, epi, 'slab%d' % n_slabs)
    want, mag, kr = D.slab_reference(v, epi)
    assert kr == n_slabs + 4
    assert D.ratio(D.slab_fp32(v, epi), want, mag) / kr <= 1.0
    vi = D.slab_values(n_slabs, 5, 13, dict(epi, row_scale=False, alpha=2.0), 'slabi%d' % n_slabs, integer=True)
    assert torch.equal(D.slab_fp32(vi, dict(epi, alpha=2.0)).double(), D.slab_reference(vi, dict(epi, alpha=2.0))[0])


@pytest.mark.parametrize('lay', ['r', 'r1', 'ro', 'c', 'c1', 'co', 'g', 'k'])
@pytest.mark.parametrize('shape', [(5, 7), (2, 5, 7), (5, 0), (0, 7), (1, 1)])
def test_operand_builder(shape, lay):
    vals = torch.arange(1, 1 + max(1, torch.Size(shape).numel()), dtype=torch.float32)[:torch.Size(shape).numel()].view(shape)
    big, view = D.place(vals, lay)
    assert torch.equal(view, vals)
    assert big.numel() > view.numel() and D.guards_intact(big, shape, lay, D.NAN)
    assert int(torch.isnan(big).sum()) == big.numel() - view.numel(), 'everything around the view is NaN'
    if view.numel():
        off = (view.data_ptr() - big.data_ptr()) // 4
        assert off >= (8 if lay == 'k' else 2)
        aligned = view.data_ptr() % 16 == 0
        assert aligned == ('1' not in lay and lay != 'g'), 'base alignment'
        assert big.data_ptr() % 64 == 0
        if lay[0] in 'rc' and min(shape[-2:]) > 1:
            ld = max(view.stride(-1), view.stride(-2))
            assert (ld % 4 == 0) == ('o' not in lay) and ld > shape[-1 if lay[0] == 'r' else -2]
        if lay == 'g':
            assert view.stride(-1) == 3 and view.stride(-2) == 2 * big.stride(-2)
        if lay[0] == 'c':
            assert view.stride(-2) == 1
        if lay == 'k':
            assert view.is_contiguous()
    # a write just outside the view is noticed, on every side
    out, oview = D.place(None, lay, D.SENT, shape=shape)
    assert bool((out == D.SENT).all()) and D.guards_intact(out, shape, lay, D.SENT)
    flat = out.view(-1)
    inside = torch.zeros(out.shape, dtype=torch.bool)
    D.layout(shape, lay)[1](inside)[...] = True
    outside = torch.nonzero(~inside.view(-1)).view(-1)
    for i in (outside[0], outside[-1], outside[outside.numel() // 2]):
        keep = float(flat[i])
        flat[i] = 0.0
        assert not D.guards_intact(out, shape, lay, D.SENT)
        flat[i] = keep
    if oview.numel():
        oview.fill_(1.0)
        assert D.guards_intact(out, shape, lay, D.SENT)


def test_rowwise_tables():
    assert set(D.TRANSPOSE_SIZES) == {1, 31, 32, 33, 65}
    for rows, cols, lx, lg, lo, *_ in D.AFFINE_CASES:
        lds = {D.place(None, l, shape=(rows, cols))[1].stride(0) for l in (lx, lg, lo)}
        assert len(lds) == 3 or rows == 1, 'three different leading dimensions'
    assert any(r * c % 256 for r, c, *_ in D.AFFINE_CASES)
    assert set(D.COLSUM_COLS) == {1, 3, 48, 255, 256, 257, 700} and set(D.GATE_COLSUM_COLS) == {1, 5, 48, 255, 256}
    L = _lib.lib()
    for cols in D.GATE_COLSUM_COLS:
        few, many = D.gate_colsum_rows(cols)
        assert L.tipk_gate_colsum_groups(few, cols) == 1
        assert L.tipk_gate_colsum_groups(many - 1, cols) == 256 and L.tipk_gate_colsum_groups(many, cols) == 256
        assert L.tipk_gate_colsum_groups(many - 1 - (256 // cols) * 4, cols) == 255
    assert L.tipk_gate_colsum_groups(5, 257) == 0
