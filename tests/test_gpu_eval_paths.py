"""-m gpu: what the evaluation reports.  `tipk_rank_metrics` (and its wrapper `utils.auprc_auroc_ap_by_range`) against
sklearn at the kernel's size steps, tie patterns and score edges, and the NNDecoder's table kernels
(`tipk_pair_table_fwd/_bwd/_loss`) against the literal formula in float64.

Metrics: the reference is sklearn as the reference project calls it (`oracle.tip_oracle.auprc_auroc_ap`) on float64 copies
of the fp32 scores, rtol 1e-9 / atol 1e-12 (the kernel's sums are fp64).  +-inf enter sklearn as +-FLT_MAX.  NaN and empty
relations are checked against the policy of include/tipk.h section 6 (NaN in all three metrics), not against sklearn, which
raises.  The C entry is never given a `max_pairs` below the largest range.

Table decoder: the reference is score = sigma(S1[u, r] + S2[v, r]) and the loss of src/layers.py:335-340 in torch float64
on the CPU.  No tolerance is a constant: for every compared quantity the same formula is evaluated in torch float32 on the
CPU, its largest deviation from float64 is what fp32 costs without the kernel, and the kernel gets 8 x that (it uses
__expf / __logf and another summation order), never less than 4 fp32 ulps of the reference's largest magnitude.  The fused
table gradients get, per cell, count(cell) * 2^-37 / n_positions on top (2^36 fixed point: half a unit per term).
The gradients of `tipk_pair_table_bwd` are sums of float atomics, which arrive in no particular order; what such a sum costs
in fp32 depends on the order (1 000 terms on one cell: 7e-6 to 1.4e-4 over a few orders on the CPU, the kernel 2e-5 and 1.4e-4
in two runs), so for those the fp32 cost is the largest over ORDERS (8) seeded permutations of the triples, not that of the
one order the test happens to build them in.
Every comparison prints "EVALERR <quantity> err=<seen> bound=<allowed>"; profiles/eval_paths_errors.md holds the table.
"""
import time

import numpy as np
import pytest
import torch

import eval_cases as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS = 1e-13                                          # src/layers.py:15
SENTINEL = -7.0                                      # no metric is negative
ORDERS = 8                                           # orders of the triples the fp32 cost of an atomic sum is taken over
SIZES = [1, 2, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192]


# ------------------------------------------------------------------------------------------------ rank metrics
def device_metrics(blocks):
    """One launch of `tipk_rank_metrics` over the relations `blocks` = [(pos, neg), ...] (fp32 arrays, possibly empty)
    into an output pre-filled with a sentinel -> float64 [3, R]."""
    from tip_amd import _lib
    sizes = [int(p.size) for p, _ in blocks]
    assert all(p.size == q.size and p.dtype == np.float32 and q.dtype == np.float32 for p, q in blocks)
    ptr = torch.from_numpy(np.r_[0, np.cumsum(sizes)].astype(np.int64)).to(DEV)
    pos = torch.from_numpy(np.concatenate([p for p, _ in blocks])).to(DEV)
    neg = torch.from_numpy(np.concatenate([q for _, q in blocks])).to(DEV)
    out = torch.full((3, len(blocks)), SENTINEL, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().tipk_rank_metrics(_lib.ptr(pos), _lib.ptr(neg), _lib.ptr(ptr), len(blocks), max(sizes),
                                            _lib.ptr(out), _lib.stream_ptr(pos.device)), 'tipk_rank_metrics')
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any(), 'cells left unwritten: %s' % np.argwhere(got == SENTINEL).tolist()
    return got


def assert_metrics(got, blocks, nan_relations=(), label=''):
    for r, (p, q) in enumerate(blocks):
        if p.size == 0 or r in nan_relations:
            assert np.isnan(got[:, r]).all(), '%s relation %d (n = %d): want NaN, got %s' % (label, r, p.size, got[:, r])
            continue
        want = E.sklearn_metrics(p, q)
        print('EVALMETRIC %s rel=%d n=%d got=%s sklearn=%s' % (label, r, p.size, got[:, r].tolist(), want.tolist()))
        np.testing.assert_allclose(got[:, r], want, rtol=1e-9, atol=1e-12, err_msg='%s relation %d (n = %d)' % (label, r, p.size))


FAMILIES = [E.continuous, E.one_decimal, E.sigmoid_logits, E.saturated_sigmoid]


@pytest.mark.parametrize('n', SIZES)
def test_rank_metrics_sizes_and_families(n):
    """Every step of the padded sort size and of the ranks per thread (1 -> 2 -> ... -> 16), each with continuous scores,
    scores rounded to one decimal (tie groups that cross thread chunks), fp32 sigmoids of N(+-2, 3) logits, and the same
    logits times 8 (many scores exactly 1.0, the low end down to denormals and 0)."""
    blocks = [f(n, 100 + n) for f in FAMILIES]
    if n >= 512:
        assert (blocks[3][0] == 1.0).sum() > n // 4 and (blocks[3][1] == 1.0).any()
    assert_metrics(device_metrics(blocks), blocks, label='n=%d' % n)


def test_rank_metrics_one_tie_group_over_all_threads():
    """16 384 equal scores: one operating point, owned by the last thread; the carry scan runs over 1 023 empty threads."""
    blocks = [E.all_equal(8192), E.all_equal(8192, 0.0), E.all_equal(8192, 1.0)]
    got = device_metrics(blocks)
    assert_metrics(got, blocks, label='all equal')
    assert (got[1] == 0.5).all(), got[1]


@pytest.mark.parametrize('n', [513, 8192])
def test_rank_metrics_perfect_and_inverted_separation(n):
    blocks = [E.separated(n, n), E.separated(n, n, inverted=True)]
    got = device_metrics(blocks)
    print('EVALMETRIC separated n=%d got=%s' % (n, got.tolist()))
    assert_metrics(got, blocks, label='separated')
    assert got[1, 0] == 1.0 and got[2, 0] == 1.0 and got[1, 1] == 0.0, got


def test_rank_metrics_saturation_at_zero_and_one():
    """Scores that are exactly 0.0 and 1.0 in both classes, with a few values in between."""
    rng = np.random.RandomState(4)
    blocks = []
    for n in (513, 8192):
        p = rng.choice(np.array([0.0, 1.0, 1.0, 1.0, 0.5, 0.999999], np.float32), n)
        q = rng.choice(np.array([0.0, 0.0, 0.0, 1.0, 0.5, 1e-7], np.float32), n)
        blocks.append((p, q))
    assert_metrics(device_metrics(blocks), blocks, label='saturated 0/1')


@pytest.mark.parametrize('n', [2, 513, 4097, 8192])
def test_rank_metrics_logits_negative_and_denormal(n):
    blocks = [E.logits(n, n), tuple(-a for a in E.continuous(n, n))]
    assert_metrics(device_metrics(blocks), blocks, label='logits')


@pytest.mark.parametrize('n', [4, 500, 8192])
def test_rank_metrics_signed_zeros_tie(n):
    """-0.0 and +0.0 in both classes, next to small values of both signs: sklearn (and numpy) compare them equal, so they
    are one threshold.  (Keyed on their bits, +0.0 ranks above -0.0: AUROC 0.4104 instead of 0.4820 at n = 500.)"""
    blocks = [E.signed_zeros(n, 0)]
    for p, q in blocks:
        for a in (p, q):
            assert (a[a == 0].view(np.uint32) == 0).any() and (a[a == 0].view(np.uint32) == 0x80000000).any()
    assert_metrics(device_metrics(blocks), blocks, label='signed zeros')


@pytest.mark.parametrize('n', [16, 513, 8192])
def test_rank_metrics_infinities_are_ordinary_scores(n):
    blocks = [E.infinities(n, n)]
    for a in blocks[0]:
        assert np.isposinf(a).sum() >= 1 and np.isneginf(a).sum() >= 1
    assert_metrics(device_metrics(blocks), blocks, label='infinities')


def test_rank_metrics_mixed_launch_with_empty_relations():
    """Sizes [0, 1, 8192, 0, 3, 0]: empty relations first, in the middle and last report NaN, the others equal sklearn, and
    every cell of the sentinel-filled output is written."""
    sizes = [0, 1, 8192, 0, 3, 0]
    blocks = [E.one_decimal(n, 7 + i) for i, n in enumerate(sizes)]
    assert_metrics(device_metrics(blocks), blocks, label='mixed')


def test_rank_metrics_nan_scores_poison_their_relation_only():
    sizes = [40, 700, 5, 8192, 1, 513]
    blocks = [E.continuous(n, 20 + i) for i, n in enumerate(sizes)]
    clean = device_metrics(blocks)
    dirty = [(p.copy(), q.copy()) for p, q in blocks]
    dirty[1][0][699] = np.nan                                          # a positive of relation 1
    dirty[3][1][4242] = -np.nan                                        # a negative of relation 3 (sign bit set)
    got = device_metrics(dirty)
    assert_metrics(got, blocks, nan_relations=(1, 3), label='nan')
    keep = [0, 2, 4, 5]
    assert np.array_equal(got[:, keep], clean[:, keep])


def test_rank_metrics_full_size_test_ranges(monkeypatch):
    """The 1 097 test ranges of the BioSNAP split with saturated fp32 sigmoids: the wrapper takes the device route (largest
    range <= 8 192), every relation equals sklearn, and a second run is bit-identical."""
    from tip_amd import ops, utils
    from tip_amd.data import build_data_dict
    rg = build_data_dict()['dd_test_range']
    sizes = (rg[:, 1] - rg[:, 0]).numpy()
    assert rg.shape[0] == 1097 and 5000 < sizes.max() <= 8192 and sizes.min() >= 1
    pos, neg = E.saturated_sigmoid(int(rg[-1, 1]), 31)
    routes = []
    real = ops.rank_metrics

    def spy(*a, **kw):
        rec = real(*a, **kw)
        routes.append(rec is not None)
        return rec
    monkeypatch.setattr(ops, 'rank_metrics', spy)
    pt, nt = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)
    got = utils.auprc_auroc_ap_by_range(pt, nt, rg)
    again = utils.auprc_auroc_ap_by_range(pt, nt, rg)
    assert routes == [True, True]
    assert got.shape == (3, 1097) and got.dtype == np.float64 and np.array_equal(got, again)
    t0 = time.time()
    want = np.stack([E.sklearn_metrics(pos[a:b], neg[a:b]) for a, b in rg.tolist()], 1)
    print('EVALMETRIC full size: 1097 sklearn calls %.1f s; max |diff| %.3g' % (time.time() - t0, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the wrapper
def _ranges(sizes):
    ptr = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    return ptr, torch.from_numpy(np.stack([ptr[:-1], ptr[1:]], 1))


def _spy_routes(monkeypatch):
    from tip_amd import ops
    routes, real = [], ops.rank_metrics

    def spy(*a, **kw):
        rec = real(*a, **kw)
        routes.append('device' if rec is not None else 'too large')
        return rec
    monkeypatch.setattr(ops, 'rank_metrics', spy)
    return routes


def test_wrapper_accepts_fp64_fp16_and_strided_scores(monkeypatch):
    from tip_amd.utils import auprc_auroc_ap_by_range
    routes = _spy_routes(monkeypatch)
    sizes = [3, 700, 1, 1025]
    ptr, rg = _ranges(sizes)
    tot = int(ptr[-1])

    def verify(got, pos, neg):
        assert got.shape == (3, len(sizes)) and got.dtype == np.float64
        for r in range(len(sizes)):
            want = E.sklearn_metrics(pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]])
            np.testing.assert_allclose(got[:, r], want, rtol=1e-9, atol=1e-12)
    # fp64 scores that differ below fp32 resolution: ranked as they are (the host path; the kernel ranks fp32)
    rng = np.random.RandomState(8)
    p64, n64 = 0.5 + rng.rand(tot) * 1e-9, 0.5 + rng.rand(tot) * 1e-9
    got = auprc_auroc_ap_by_range(torch.from_numpy(p64).to(DEV), torch.from_numpy(n64).to(DEV), rg)
    verify(got, p64, n64)
    assert routes == []
    # fp16 scores: exact in fp32, device route
    p16, n16 = (a.astype(np.float16) for a in E.continuous(tot, 9))
    got = auprc_auroc_ap_by_range(torch.from_numpy(p16).to(DEV), torch.from_numpy(n16).to(DEV), rg)
    verify(got, p16.astype(np.float32), n16.astype(np.float32))
    assert routes == ['device']
    # every second element of a wider buffer
    p32, n32 = E.one_decimal(tot, 10)
    wide_p, wide_n = torch.full((2 * tot,), 9.0, device=DEV), torch.full((tot, 3), -9.0, device=DEV)
    wide_p[::2] = torch.from_numpy(p32).to(DEV)
    wide_n[:, 1] = torch.from_numpy(n32).to(DEV)
    assert not wide_p[::2].is_contiguous() and not wide_n[:, 1].is_contiguous()
    got = auprc_auroc_ap_by_range(wide_p[::2], wide_n[:, 1], rg)
    verify(got, p32, n32)
    assert routes == ['device', 'device']


def test_wrapper_host_path_for_gaps_and_oversized_relations(monkeypatch):
    """Non-consecutive ranges and a launch with one 8 193-pair relation are evaluated on the host with the same policy: the
    same numbers as sklearn, NaN (no exception) for empty and NaN-holding relations, and the same [3, R] float64 record."""
    from tip_amd.utils import auprc_auroc_ap_by_range
    routes = _spy_routes(monkeypatch)
    # gaps between the ranges, one of them empty, one with a NaN
    rg = torch.tensor([[0, 5], [10, 40], [40, 41], [50, 50], [60, 100]])
    pos, neg = E.one_decimal(100, 12)
    pos[70] = np.nan
    got = auprc_auroc_ap_by_range(torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), rg)
    assert routes == [] and got.shape == (3, 5) and got.dtype == np.float64
    for r, (a, b) in enumerate(rg.tolist()):
        if r in (3, 4):
            assert np.isnan(got[:, r]).all(), got[:, r]
        else:
            np.testing.assert_allclose(got[:, r], E.sklearn_metrics(pos[a:b], neg[a:b]), rtol=1e-9, atol=1e-12)
    # one relation beyond the single-workgroup sort among small ones (an empty one and a NaN among them)
    sizes = [4, 0, 8193, 30, 2]
    ptr, rg = _ranges(sizes)
    pos, neg = E.saturated_sigmoid(int(ptr[-1]), 13)
    pos[ptr[3] + 7] = np.nan
    got = auprc_auroc_ap_by_range(torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), rg)
    assert routes == ['too large'] and got.shape == (3, 5) and got.dtype == np.float64
    for r in range(5):
        if r in (1, 3):
            assert np.isnan(got[:, r]).all(), got[:, r]
        else:
            want = E.sklearn_metrics(pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]])
            np.testing.assert_allclose(got[:, r], want, rtol=1e-9, atol=1e-12)
    # the same launch without the large relation takes the device route: same record for the relations they share
    keep = [0, 1, 3, 4]
    ptr2, rg2 = _ranges([sizes[r] for r in keep])
    sel = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in keep])
    dev = auprc_auroc_ap_by_range(torch.from_numpy(pos[sel]).to(DEV), torch.from_numpy(neg[sel]).to(DEV), rg2)
    assert routes == ['too large', 'device'] and dev.shape == (3, 4) and dev.dtype == got.dtype
    np.testing.assert_allclose(dev, got[:, keep], rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.array_equal(np.isnan(dev), np.isnan(got[:, keep]))


# ------------------------------------------------------------------------------------------------ table decoder
def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def check(name, got, ref64, cpu32, extra=None):
    """got (device fp32) against ref64 within max(8 x the cost of fp32 on the CPU, 4 fp32 ulps of max |ref64|), plus the
    per-element `extra` where given.  Prints the error seen next to the bound."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    cost = max(float((c.detach().double().reshape(ref64.shape) - ref64).abs().max())
               for c in (cpu32 if isinstance(cpu32, (list, tuple)) else [cpu32]))       # (several orders of one sum)
    floor = 4 * ulp32(ref64.abs().max())
    bound = max(8 * cost, floor)
    err = (got - ref64).abs()
    tol = torch.full_like(ref64, bound) if extra is None else bound + extra.double().reshape(ref64.shape)
    worst = float((err / tol).max())
    print('EVALERR %-34s err=%.3e bound=%.3e (8 x fp32 cost %.3e, 4 ulp %.3e%s) used=%.3f max|ref|=%.3e'
          % (name, float(err.max()), bound, 8 * cost, floor,
             '' if extra is None else ', fixed point <= %.3e' % float(extra.max()), worst, float(ref64.abs().max())))
    assert torch.isfinite(got).all(), name
    assert worst <= 1.0, '%s: error %.3e exceeds its bound %.3e' % (name, float(err.max()), float(tol.min()))
    if extra is None:
        torch.testing.assert_close(got, ref64, rtol=0.0, atol=bound)     # (seen by TIPK_ERRLOG)


def table_reference(s1, s2, u, v, et, sigmoid, g, dtype):
    """score and d S1 / d S2 of sum(g * score), score = sigma(S1[u, r] + S2[v, r]), by autograd in `dtype` on the CPU."""
    a = s1.to(dtype).clone().requires_grad_(True)
    b = s2.to(dtype).clone().requires_grad_(True)
    x = a[u, et] + b[v, et]
    score = torch.sigmoid(x) if sigmoid else x
    (score * g.to(dtype)).sum().backward()
    return score.detach(), a.grad, b.grad


def table_kernels(s1, s2, u, v, et, sigmoid, g, pad):
    """`tipk_pair_table_fwd` then `_bwd` through the C entries on tables whose row stride is R + pad; the padding columns
    hold NaN on the way in and must stay zero in the gradients."""
    from tip_amd import _lib
    N, R = s1.shape
    ld = R + pad

    def padded(t, fill):
        w = torch.full((N, ld), fill, dtype=torch.float32, device=DEV)
        w[:, :R] = t.to(DEV)
        return w
    w1, w2 = padded(s1, float('nan')), padded(s2, float('nan'))
    ud, vd, etd, gd = u.to(DEV).contiguous(), v.to(DEV).contiguous(), et.to(DEV).contiguous(), g.to(DEV)
    ib, eb = ud.element_size(), etd.element_size()
    n = ud.numel()
    score = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV)
    g1 = torch.zeros((N, ld), dtype=torch.float32, device=DEV)
    g2 = torch.zeros((N, ld), dtype=torch.float32, device=DEV)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(torch.device(DEV))
    _lib.check(L.tipk_pair_table_fwd(p(w1), p(w2), ld, p(ud), p(vd), ib, p(etd), eb, n, int(sigmoid), p(score), st),
               'tipk_pair_table_fwd')
    _lib.check(L.tipk_pair_table_bwd(p(gd), p(score), ld, p(ud), p(vd), ib, p(etd), eb, n, int(sigmoid), p(g1), p(g2), st),
               'tipk_pair_table_bwd')
    torch.cuda.synchronize()
    assert not g1[:, R:].any() and not g2[:, R:].any(), 'gradient written into the padding columns'
    return score, g1[:, :R], g2[:, :R]


def check_table(label, s1, s2, u, v, et, sigmoid, g, pad):
    got = table_kernels(s1, s2, u, v, et, sigmoid, g, pad)
    ul, vl, el = u.long(), v.long(), et.long()
    ref = table_reference(s1, s2, ul, vl, el, sigmoid, g, torch.float64)
    c32 = table_reference(s1, s2, ul, vl, el, sigmoid, g, torch.float32)
    check('table %s score' % label, got[0], ref[0], c32[0])
    gen = torch.Generator().manual_seed(ul.numel())
    orders = [c32]
    for _ in range(ORDERS - 1):
        o = torch.randperm(ul.numel(), generator=gen)
        orders.append(table_reference(s1, s2, ul[o], vl[o], el[o], sigmoid, g[o], torch.float32))
    for k, what in ((1, 'd S1'), (2, 'd S2')):
        check('table %s %s' % (label, what), got[k], ref[k], [c[k] for c in orders])
    return got


@pytest.mark.parametrize('sigmoid', [0, 1])
@pytest.mark.parametrize('et_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('idx_dtype', [torch.int32, torch.int64])
def test_pair_table_widths_counts_and_padded_tables(idx_dtype, et_dtype, sigmoid):
    """All four index / type widths of the dispatch, with and without the sigmoid, at triple counts around the 256-thread
    workgroup, on tables with ld > R."""
    gen = torch.Generator().manual_seed(5)
    N, R = 37, 11
    s1, s2 = torch.randn(N, R, generator=gen) * 2, torch.randn(N, R, generator=gen) * 2
    for n, pad in ((1, 5), (255, 1), (256, 5), (257, 21)):
        u = torch.randint(0, N, (n,), generator=gen).to(idx_dtype)
        v = torch.randint(0, N, (n,), generator=gen).to(idx_dtype)
        et = torch.randint(0, R, (n,), generator=gen).to(et_dtype)
        g = torch.randn(n, generator=gen)
        check_table('%s/%s sig=%d n=%d' % (str(idx_dtype)[-5:], str(et_dtype)[-5:], sigmoid, n), s1, s2, u, v, et,
                    sigmoid, g, pad)


@pytest.mark.parametrize('sigmoid', [0, 1])
def test_pair_table_repeated_triple_and_self_pair(sigmoid):
    """One triple 1 000 times with u = v among 300 others: 1 000 atomic adds land on one cell of each gradient table."""
    gen = torch.Generator().manual_seed(6)
    N, R = 20, 4
    s1, s2 = torch.randn(N, R, generator=gen), torch.randn(N, R, generator=gen)
    u = torch.cat([torch.full((1000,), 7), torch.randint(0, N, (300,), generator=gen)])
    v = torch.cat([torch.full((1000,), 7), torch.randint(0, N, (300,), generator=gen)])
    et = torch.cat([torch.full((1000,), 2), torch.randint(0, R, (300,), generator=gen)])
    perm = torch.randperm(1300, generator=gen)
    g = torch.rand(1300, generator=gen) + 0.5                          # one sign: the 1 000 terms add up
    check_table('repeated sig=%d' % sigmoid, s1, s2, u[perm], v[perm], et[perm], sigmoid, g, pad=3)


def test_pair_table_saturated_logits():
    """Logits of +-100: the fp32 sigmoid is 1 or (nearly) 0, both finite, and d sigma = s (1 - s) vanishes."""
    gen = torch.Generator().manual_seed(7)
    N, R, n = 16, 3, 600
    s1 = torch.where(torch.rand(N, R, generator=gen) < 0.5, 50.0, -50.0)
    s2 = s1.clone()                                                    # u = v -> exactly +-100; else 0 or +-100
    u = torch.randint(0, N, (n,), generator=gen)
    v = torch.where(torch.rand(n, generator=gen) < 0.7, u, torch.randint(0, N, (n,), generator=gen))
    et = torch.randint(0, R, (n,), generator=gen)
    g = torch.randn(n, generator=gen)
    for sigmoid in (0, 1):
        score, g1, g2 = check_table('+-100 sig=%d' % sigmoid, s1, s2, u, v, et, sigmoid, g, pad=1)
        x = (s1[u, et] + s2[v, et])
        assert set(x.tolist()) == {-100.0, 0.0, 100.0}
        if sigmoid:
            s = score.cpu()
            assert bool((s[x == 100] == 1).all()) and bool((s[x == -100] < 1e-40).all()) and bool((s[x == 0] == 0.5).all())


# ---- the fused objective on the transposed tables
def objective_reference(s1t, s2t, pos, neg, et, dtype):
    """loss of src/layers.py:335-340 with score = sigma(S1[u, r] + S2[v, r]) and its table gradients, autograd in `dtype`."""
    a = s1t.to(dtype).clone().requires_grad_(True)
    b = s2t.to(dtype).clone().requires_grad_(True)
    ps = torch.sigmoid(a[et, pos[0]] + b[et, pos[1]])
    ns = torch.sigmoid(a[et, neg[0]] + b[et, neg[1]])
    loss = -torch.log(ps + EPS).mean() - torch.log(1 - ns + EPS).mean()
    loss.backward()
    return loss.detach().view(1), a.grad, b.grad


def fixed_point_term(shape, pos, neg, et):
    """Per cell of d S1^T / d S2^T: (terms added to the cell) * 2^-37 / n_positions."""
    R, n = shape
    E_ = et.numel()
    c1 = torch.bincount(et * n + pos[0], minlength=R * n) + torch.bincount(et * n + neg[0], minlength=R * n)
    c2 = torch.bincount(et * n + pos[1], minlength=R * n) + torch.bincount(et * n + neg[1], minlength=R * n)
    return c1.view(R, n).double() * 2.0 ** -37 / E_, c2.view(R, n).double() * 2.0 ** -37 / E_


def fused_objective(s1t, s2t, pos, neg, et, grad=True):
    from tip_amd import ops
    a = s1t.to(DEV).requires_grad_(grad)
    b = s2t.to(DEV).requires_grad_(grad)
    loss = ops.pair_table_objective(a, b, pos.to(DEV), neg.to(DEV), et.to(DEV))
    if not grad:
        return loss.detach(), None, None
    loss.backward()
    return loss.detach(), a.grad, b.grad


def check_objective(label, s1t, s2t, pos, neg, et):
    loss, g1, g2 = fused_objective(s1t, s2t, pos, neg, et)
    ref = objective_reference(s1t, s2t, pos, neg, et, torch.float64)
    c32 = objective_reference(s1t, s2t, pos, neg, et, torch.float32)
    fx = fixed_point_term(s1t.shape, pos, neg, et)
    check('fused %s loss' % label, loss, ref[0], c32[0])
    check('fused %s d S1t' % label, g1, ref[1], c32[1], extra=fx[0])
    check('fused %s d S2t' % label, g2, ref[2], c32[2], extra=fx[1])
    # loss-only mode and a second run: the same bits
    only, _, _ = fused_objective(s1t, s2t, pos, neg, et, grad=False)
    loss2, h1, h2 = fused_objective(s1t, s2t, pos, neg, et)
    assert torch.equal(only, loss) and torch.equal(loss2, loss) and torch.equal(h1, g1) and torch.equal(h2, g2), label
    return loss, g1, g2


def triples(counts, n, gen):
    et = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    tot = int(et.numel())
    return torch.randint(0, n, (2, tot), generator=gen), torch.randint(0, n, (2, tot), generator=gen), et


def test_fused_objective_empty_and_one_position_relations():
    """Relations without a triple first, in the middle and last (their gradient rows must be written as zeros), a
    one-position relation, and blocks around the 1 024-thread stride."""
    gen = torch.Generator().manual_seed(8)
    counts, n = [0, 1, 300, 0, 1025, 5, 1024, 0], 50
    pos, neg, et = triples(counts, n, gen)
    s1t, s2t = torch.randn(len(counts), n, generator=gen) * 2, torch.randn(len(counts), n, generator=gen) * 2
    _, g1, g2 = check_objective('empty relations', s1t, s2t, pos, neg, et)
    for r in (0, 3, 7):
        assert not g1[r].any() and not g2[r].any()


@pytest.mark.parametrize('n', [1, 2, 1024, 1025, 6400])
def test_fused_objective_node_counts(n):
    """Node counts around the 1 024-thread staging loop up to the largest the kernel takes (6 400: two table rows and two
    64-bit gradient rows in 150 KB of LDS)."""
    from tip_amd import ops
    assert ops.pair_table_loss_supported(n)
    gen = torch.Generator().manual_seed(9 + n)
    counts = [700, 0, 2500, 1]
    pos, neg, et = triples(counts, n, gen)
    if n > 2:
        pos[:, -1], neg[:, -1] = n - 1, n - 1                          # the last node, on both sides
    s1t, s2t = torch.randn(4, n, generator=gen) * 2, torch.randn(4, n, generator=gen) * 2
    check_objective('n=%d' % n, s1t, s2t, pos, neg, et)


def test_fused_objective_saturated_logits():
    """Relations 0 / 1 score every pair at +100 / -100: the eps = 1e-13 floor keeps the loss finite and equal to float64
    with the same eps, and the gradient is exactly 0 where the fp32 sigmoid saturates."""
    gen = torch.Generator().manual_seed(10)
    counts, n = [600, 600, 900], 40
    pos, neg, et = triples(counts, n, gen)
    s1t, s2t = torch.randn(3, n, generator=gen), torch.randn(3, n, generator=gen)
    s1t[0], s2t[0], s1t[1], s2t[1] = 50.0, 50.0, -50.0, -50.0
    loss, g1, g2 = check_objective('+-100', s1t, s2t, pos, neg, et)
    assert torch.isfinite(loss).all()
    assert not g1[:2].any() and not g2[:2].any()
    assert g1[2].abs().max() > 0
    # the floor is what the saturated relations contribute: 600 negatives of relation 0 and 600 positives of relation 1 at
    # log(eps) each, the other 1 200 at log(1 + eps) = 0; relation 2 adds 900 ordinary terms on either side
    floor_part = -1200 * np.log(EPS) / 2100
    assert floor_part < float(loss) < floor_part + 2 * 900 / 2100 * 3


def test_fused_objective_all_positions_on_one_cell():
    """Every position of relation 1 is the pair (3, 7), positive and negative: 2 x 3 000 fixed-point adds on one LDS cell of
    each gradient row."""
    gen = torch.Generator().manual_seed(11)
    counts, n = [200, 3000, 10], 12
    pos, neg, et = triples(counts, n, gen)
    pos[0, 200:3200], pos[1, 200:3200], neg[0, 200:3200], neg[1, 200:3200] = 3, 7, 3, 7
    s1t, s2t = torch.randn(3, n, generator=gen), torch.randn(3, n, generator=gen)
    check_objective('one cell', s1t, s2t, pos, neg, et)


# ---- through the module: the fused route up to 6 400 nodes, the table kernels beyond
def module_reference(z, w, pos, neg, et, dtype):
    """NNDecoder (src/layers.py:598-637) under the loss of src/layers.py:335-340, autograd in `dtype` on the CPU."""
    z = z.to(dtype).clone().requires_grad_(True)
    w = [t.to(dtype).clone().requires_grad_(True) for t in w]
    s1 = torch.relu(z @ w[0]) @ w[1].t()
    s2 = torch.relu(z @ w[2]) @ w[3].t()
    ps = torch.sigmoid(s1[pos[0], et] + s2[pos[1], et])
    ns = torch.sigmoid(s1[neg[0], et] + s2[neg[1], et])
    loss = -torch.log(ps + EPS).mean() - torch.log(1 - ns + EPS).mean()
    loss.backward()
    return [loss.detach().view(1), z.grad] + [t.grad for t in w]


@pytest.mark.parametrize('n', [1, 2, 1024, 1025, 6400, 6401])
def test_nn_decoder_objective_routes(n, monkeypatch):
    """`NNDecoder.objective` against float64 autograd of the module's formula: loss, d z and the four weight gradients.
    Up to 6 400 nodes it runs the fused kernel, and repeats bit for bit; 6 401 nodes must take the table kernels (forward
    and backward, float atomics) and agree within the same kind of bound."""
    from tip_amd import ops
    from tip_amd.layers import NNDecoder
    calls = {'fused': 0, 'tables': 0}
    real_fused, real_tables = ops.pair_table_objective, ops.pair_table_score

    def fused(*a, **kw):
        calls['fused'] += 1
        return real_fused(*a, **kw)

    def tables(*a, **kw):
        calls['tables'] += 1
        return real_tables(*a, **kw)
    monkeypatch.setattr(ops, 'pair_table_objective', fused)
    monkeypatch.setattr(ops, 'pair_table_score', tables)
    gen = torch.Generator().manual_seed(12 + n)
    R, counts = 5, [900, 0, 1, 2100, 64]
    pos, neg, et = triples(counts, n, gen)
    if n > 2:
        pos[:, -1], neg[:, -1] = n - 1, n - 1
    z_c = torch.randn(n, 16, generator=gen) * 0.5
    m = NNDecoder(16, R, l1_dim=16)
    names = ('w1_l1', 'w1_l2', 'w2_l1', 'w2_l2')
    for k in names:
        getattr(m, k).data = torch.randn(getattr(m, k).shape, generator=gen) * 0.4
    w = [getattr(m, k).detach().clone() for k in names]
    m = m.to(DEV)

    def run():
        m.zero_grad()
        z = z_c.to(DEV).requires_grad_(True)
        loss = m.objective(z, pos.to(DEV), neg.to(DEV), et.to(DEV))
        loss.backward()
        return [loss.detach(), z.grad.clone()] + [getattr(m, k).grad.clone() for k in names]
    got = run()
    fused_route = n <= 6400
    assert ops.pair_table_loss_supported(n) == fused_route
    assert calls == ({'fused': 1, 'tables': 0} if fused_route else {'fused': 0, 'tables': 2}), calls
    ref = module_reference(z_c, w, pos, neg, et, torch.float64)
    c32 = [module_reference(z_c, w, pos, neg, et, torch.float32)]
    if not fused_route:                                               # float atomics: the fp32 cost over several orders
        for _ in range(ORDERS - 1):
            o = torch.randperm(et.numel(), generator=gen)
            c32.append(module_reference(z_c, w, pos[:, o], neg[:, o], et[o], torch.float32))
    c32 = list(zip(*c32))
    route = 'fused' if fused_route else 'unfused'
    for what, a, b, c in zip(('loss', 'd z') + tuple('d ' + k for k in names), got, ref, c32):
        check('module %s n=%d %s' % (route, n, what), a, b, c)
    if fused_route:
        again = run()
        assert all(torch.equal(a, b) for a, b in zip(got, again))
