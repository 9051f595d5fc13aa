"""-m gpu: the negative sampler against its bit-exact spec on every launch path, and the fused objective across the
values it meets in training (saturated scores, wide dynamic range, non-finite inputs, full BioSNAP size against fp64).

Sampler cases compare every output form the case uses (int64 [2, E], int32 [2, E], packed int32 [E]) with
`typed_negative_sampling_spec` bit for bit, into outputs pre-filled with a sentinel (-1 is no pair of any form: a packed
word 0xffffffff would be node 65535 of a graph of at most 65535 nodes), so an unwritten position fails too.
Each launch runs once.
"""
import math

import numpy as np
import pytest
import torch

from oracle import tip_oracle as O
from oracle.philox_sampler import typed_negative_sampling_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SEED = 0x5DEECE66D1234567
FORMS_ALL = ('int64', 'int32', 'packed')


@pytest.fixture(autouse=True)
def _fresh_key_cache():
    from tip_amd import neg_sampling as NS
    NS._key_cache.clear()            # (every case builds its own keys; an entry pins its tensors, so emptying also frees them)
    yield
    NS._key_cache.clear()


def _rg(rel_ptr):
    rel_ptr = np.asarray(rel_ptr, dtype=np.int64)
    return torch.from_numpy(np.stack([rel_ptr[:-1], rel_ptr[1:]], 1))


def draw(pos_t, n, rel_ptr, seed, form, wg=None, pos_offset=None, no_keys32=False, out=None):
    """One launch of `tipk_typed_negative_sampling` into a sentinel-filled output -> (int64 [2, E] numpy, out)."""
    from tip_amd import neg_sampling as NS, ops
    keys, rp, n_rel, wg0, (_, keys32) = NS._cached_keys(pos_t, n, _rg(rel_ptr))
    E = pos_t.shape[1]
    wg = wg0 if wg is None else (wg[0].to(DEV), wg[1].to(DEV))
    packed = form == 'packed'
    dtype = torch.int32 if form != 'int64' else torch.int64
    if out is None:
        out = torch.full((E,) if packed else (2, E), -1, dtype=dtype, device=DEV)
    po = None if pos_offset is None else torch.as_tensor(pos_offset, dtype=torch.int64).to(DEV)
    ops.typed_negative_sampling_device(keys, rp, n_rel, n, seed, E, dtype=dtype, wg=wg, pos_offset=po, packed=packed,
                                       keys32=None if no_keys32 else keys32, out=out)
    o = out.cpu().numpy().astype(np.int64)
    unwritten = int((o == -1).sum())
    assert unwritten == 0, '%d positions left unwritten (%s)' % (unwritten, form)
    if packed:
        o = o & 0xffffffff
        o = np.stack([o & 0xffff, o >> 16])
    return o, out


def check_forms(pos_np, n, rel_ptr, seed, forms, want=None, **kw):
    if want is None:
        want = typed_negative_sampling_spec(pos_np, n, rel_ptr, seed, pos_offset=kw.get('pos_offset'))
    pos_t = torch.from_numpy(pos_np).to(DEV)
    for form in forms:
        got, _ = draw(pos_t, n, rel_ptr, seed, form, **kw)
        bad = np.nonzero((got != want).any(0))[0]
        assert bad.size == 0, '%s: %d positions differ from the spec, first %s' % (form, bad.size, bad[:8].tolist())
    return want


def force_rejections(pos_np, n, rel_ptr, seed, frac=0.5):
    """Positives that make the first draw of many positions a positive of their relation (the draws do not depend on the
    positives, only the rejections do): the last positives of every relation become the first draws of its first
    positions -- so the retry paths run at node counts where random positives almost never collide."""
    first = typed_negative_sampling_spec(pos_np, n, rel_ptr, seed)
    pos = pos_np.copy()
    for a, b in zip(rel_ptr[:-1], rel_ptr[1:]):
        m = int((b - a) * frac) // 2
        if m:
            pos[:, b - m:b] = first[:, a:a + m]
    return pos


# ------------------------------------------------------------------ A.1 full BioSNAP, as training calls it
@pytest.fixture(scope='module')
def biosnap():
    from tip_amd.data import build_data_dict
    dd = build_data_dict()
    rg = dd['dd_train_range']
    return {'pos_np': dd['dd_train_idx'].numpy(), 'n': int(dd['n_drug']), 'rg': rg,
            'rel_ptr': np.r_[0, rg[:, 1].numpy()].astype(np.int64)}


@pytest.mark.timeout(600)
def test_sampler_full_biosnap_matches_spec(biosnap):
    """645 drugs, 1 097 relations, 8.3 M positions, the default deal, two seeds; int64 and packed through
    `typed_negative_sampling`, and one sentinel-filled launch of each form; a relation-sharded rank (every third
    relation with its global offsets) draws the matching slice."""
    from tip_amd import neg_sampling as NS, ops
    pos_np, n, rg, rel_ptr = biosnap['pos_np'], biosnap['n'], biosnap['rg'], biosnap['rel_ptr']
    assert n == 645 and rel_ptr.size - 1 == 1097 and rel_ptr[-1] == 8326508
    pos_t = torch.from_numpy(pos_np).to(DEV)
    for seed in (SEED, 0x0BADC0FFEE):
        want = typed_negative_sampling_spec(pos_np, n, rel_ptr, seed)
        got = NS.typed_negative_sampling(pos_t, n, rg, seed=seed)
        assert np.array_equal(got.cpu().numpy(), want)
        got_p = NS.typed_negative_sampling(pos_t, n, rg, seed=seed, packed=True)
        assert np.array_equal(ops.unpack_pairs(got_p).cpu().numpy(), want)
        check_forms(pos_np, n, rel_ptr, seed, ('int64', 'packed'), want=want)
        keep = list(range(0, rel_ptr.size - 1, 3))
        loc = np.concatenate([pos_np[:, rel_ptr[r]:rel_ptr[r + 1]] for r in keep], axis=1)
        sizes = [rel_ptr[r + 1] - rel_ptr[r] for r in keep]
        loc_ptr = np.r_[0, np.cumsum(sizes)].astype(np.int64)
        off = torch.tensor([rel_ptr[r] - loc_ptr[i] for i, r in enumerate(keep)])
        want_l = np.concatenate([want[:, rel_ptr[r]:rel_ptr[r + 1]] for r in keep], axis=1)
        loc_t = torch.from_numpy(loc).to(DEV)
        got_l = NS.typed_negative_sampling(loc_t, n, _rg(loc_ptr), seed=seed, pos_offset=off)
        assert np.array_equal(got_l.cpu().numpy(), want_l)
        got_lp = NS.typed_negative_sampling(loc_t, n, _rg(loc_ptr), seed=seed, pos_offset=off, packed=True)
        assert np.array_equal(ops.unpack_pairs(got_lp).cpu().numpy(), want_l)


# ------------------------------------------------------------------ A.2 consecutive units of one relation
def _consecutive_same_relation(wg):
    ptr, units = wg
    return sum(int(units[i, 0] == units[i + 1, 0]) for w in range(ptr.numel() - 1)
               for i in range(int(ptr[w]), int(ptr[w + 1]) - 1))


@pytest.mark.timeout(300)
@pytest.mark.parametrize('E,n_wg', [(20000, 1), (4_000_000, 512)])
def test_sampler_consecutive_units_of_one_relation(E, n_wg):
    """A workgroup whose next unit belongs to the relation whose bitmap it holds skips the rebuild and its barriers (the
    `rel == have` path): the retry queue of the previous unit must be empty before the next unit parks a position."""
    from tip_amd.neg_sampling import sampler_units
    rng = np.random.RandomState(E % 1000 + n_wg)
    n = 645
    cells = rng.choice(n * n, int(0.4 * n * n), replace=False)            # 40 % of the cells positive
    key = cells[rng.randint(0, cells.size, E)]
    pos = np.stack([key // n, key % n]).astype(np.int64)
    rel_ptr = np.array([0, E], dtype=np.int64)
    wg = sampler_units(torch.from_numpy(rel_ptr), n_wg)
    assert _consecutive_same_relation(wg) >= 1
    check_forms(pos, n, rel_ptr, SEED, FORMS_ALL, wg=wg)


# ------------------------------------------------------------------ A.3 retry-queue overflow
@pytest.mark.timeout(300)
def test_sampler_retry_queue_overflow():
    """n = 41 with 1 200 of the 1 681 cells positive (71 % first-draw rejections) in units of 10 000 positions: ~7 000
    parked positions per unit, more than the queue's 4 096 -- the rest is drawn again in place."""
    from tip_amd.neg_sampling import sampler_units
    rng = np.random.RandomState(3)
    n, E = 41, 40000
    cells = rng.choice(n * n, 1200, replace=False)
    key = cells[rng.randint(0, cells.size, E)]
    pos = np.stack([key // n, key % n]).astype(np.int64)
    rel_ptr = np.array([0, E], dtype=np.int64)
    wg = sampler_units(torch.from_numpy(rel_ptr), 3)
    sizes = (wg[1][:, 2] - wg[1][:, 1]).tolist()
    assert sizes == [10000] * 4
    check_forms(pos, n, rel_ptr, SEED, FORMS_ALL, wg=wg)


# ------------------------------------------------------------------ A.4 saturated relations
@pytest.mark.timeout(300)
@pytest.mark.parametrize('n', [4, 1])
def test_sampler_saturated_relation_keeps_the_64th_draw(n):
    """Every cell positive: every attempt is rejected and the 64th draw is kept -- by the parked retry loop and by the
    in-place loop alike (two units of 6 000 on one workgroup: 4 096 parked, 1 904 in place, and `rel == have`)."""
    from tip_amd.neg_sampling import sampler_units
    E = 12000
    cells = np.arange(n * n)
    key = np.resize(cells, E)
    pos = np.stack([key // n, key % n]).astype(np.int64)
    rel_ptr = np.array([0, E], dtype=np.int64)
    wg = sampler_units(torch.from_numpy(rel_ptr), 1)
    assert (wg[1][:, 2] - wg[1][:, 1]).tolist() == [6000, 6000]
    check_forms(pos, n, rel_ptr, SEED, FORMS_ALL, wg=wg)


# ------------------------------------------------------------------ A.5 node-count boundaries of the launch choice
@pytest.mark.timeout(300)
@pytest.mark.parametrize('n,wgs_per_cu', [(712, 2), (713, 1), (1078, 1), (1079, 0), (65535, 0), (65536, 0), (70001, 0)])
def test_sampler_node_count_boundaries(n, wgs_per_cu):
    """712 / 713: two 512-thread workgroups per CU / one of 1 024; 1 078 / 1 079: the last LDS bitmap / the first
    binary-search launch; 65 535: the largest packed output; 65 536: n^2 = 2^32, the 64-bit-candidate branch; 70 001."""
    from tip_amd import ops
    assert ops.lib().tipk_negsample_wgs_per_cu(n) == wgs_per_cu
    rng = np.random.RandomState(n)
    rel_ptr = np.r_[0, np.cumsum([9000, 0, 20000, 5])].astype(np.int64)
    pos = rng.randint(0, n, (2, int(rel_ptr[-1]))).astype(np.int64)
    pos = force_rejections(pos, n, rel_ptr, SEED)
    forms = FORMS_ALL if n <= 65535 else ('int64', 'int32')
    check_forms(pos, n, rel_ptr, SEED, forms)


# ------------------------------------------------------------------ A.6 relations longer than the key prefetch
@pytest.mark.timeout(300)
@pytest.mark.parametrize('n,E,no_keys32', [(645, 9000, False), (800, 20000, False), (645, 9000, True)])
def test_sampler_relations_longer_than_the_key_prefetch(n, E, no_keys32):
    """Bitmap builds beyond NS_PRE x threads keys (4 096 at 512 threads, 8 192 at 1 024) take the tail loop; without
    32-bit keys the build reads the int64 keys."""
    from tip_amd import ops
    assert ops.lib().tipk_negsample_wgs_per_cu(n) == (2 if n <= 712 else 1)
    rng = np.random.RandomState(E)
    rel_ptr = np.array([0, 37, 37 + E], dtype=np.int64)
    pos = rng.randint(0, n, (2, int(rel_ptr[-1]))).astype(np.int64)
    pos = force_rejections(pos, n, rel_ptr, SEED)
    check_forms(pos, n, rel_ptr, SEED, ('int64', 'packed'), no_keys32=no_keys32)


# ------------------------------------------------------------------ A.7 unaligned starts
@pytest.mark.timeout(300)
def test_sampler_unaligned_offsets_and_output():
    """pos_offset with off & 3 != 0 and a packed output whose base is 4 bytes past a 16-byte boundary: the four words of
    a Philox call go out as scalar stores next to the 16-byte store; the word in front of the view stays untouched."""
    rng = np.random.RandomState(17)
    n = 645
    rel_ptr = np.r_[0, np.cumsum([5001, 0, 12003, 77])].astype(np.int64)
    E = int(rel_ptr[-1])
    pos = force_rejections(rng.randint(0, n, (2, E)).astype(np.int64), n, rel_ptr, SEED)
    off = [5, 0, 1001, 3]
    want = check_forms(pos, n, rel_ptr, SEED, FORMS_ALL, pos_offset=off)
    for o in (None, off):
        buf = torch.full((E + 5,), -1, dtype=torch.int32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:E + 1]
        w = want if o is not None else typed_negative_sampling_spec(pos, n, rel_ptr, SEED)
        got, _ = draw(torch.from_numpy(pos).to(DEV), n, rel_ptr, SEED, 'packed', pos_offset=o, out=view)
        assert np.array_equal(got, w)
        rest = buf.cpu()
        assert int(rest[0]) == -1 and bool((rest[E + 1:] == -1).all())


# ------------------------------------------------------------------ C. the objective
ROUTES = ('fused', 'task_kernel', 'float_atomics')
ROUTE_K = [('fused', 16), ('fused', 8), ('fused', 4), ('task_kernel', 16), ('float_atomics', 16)]
U = 2.0 ** -24                                                          # fp32 spacing in [0.5, 1)


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops as o
    return o


def close(got, want, rtol=1e-4, atol=None):
    want = want.to(torch.float64).cpu()
    got = got.detach().to('cpu', torch.float64)
    if atol is None:
        atol = 2e-5 * max(1.0, float(want.abs().max()))
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol)


def objective(ops, route, z, w, pos, neg, et, monkeypatch, need_grad=True):
    """ops.distmult_loss on one route: the fused objective kernel, the task kernel (dm_task_kernel = 1) or the task kernel
    with float atomics (TIPK_FLOAT_ATOMICS = 1)."""
    from tip_amd import _lib
    if route == 'float_atomics':
        monkeypatch.setenv('TIPK_FLOAT_ATOMICS', '1')
    if route == 'task_kernel':
        _lib.set_option('dm_task_kernel', 1)
    try:
        return ops.distmult_loss(z, w, pos, neg, et, need_grad=need_grad)
    finally:
        _lib.set_option('dm_task_kernel', 0)
        monkeypatch.delenv('TIPK_FLOAT_ATOMICS', raising=False)


def reference(z, w, pos, neg, et, dtype):
    """The oracle's objective (loss, d z, d w, positive and negative sigma) evaluated in `dtype`: float64 is the exact
    value, float32 the reference's own arithmetic (src/layers.py:338-340, EPS = 1e-13)."""
    z, w = z.to(dtype), w.to(dtype)
    ps, ns = O.distmult_fwd(z, pos, et, w), O.distmult_fwd(z, neg, et, w)
    gp, gn = O.tip_loss_bwd(ps, ns)
    a1, b1 = O.distmult_bwd(gp, z, pos, et, w)
    a2, b2 = O.distmult_bwd(gn, z, neg, et, w)
    return O.tip_loss(ps, ns), a1 + a2, b1 + b2, ps, ns


def abs_terms(cp, cn, z64, w64, pos, neg, et):
    """Per element of d z and of d w: sum over the terms that reach it of |c| |z| |w| (c: per-triple coefficient bounds)."""
    za, wa = z64.abs(), w64.abs()
    a, b = O.distmult_bwd(cp, za, pos, et, wa, sigmoid=False)
    c, d = O.distmult_bwd(cn, za, neg, et, wa, sigmoid=False)
    return a + c, b + d


def fp32_bounds(z64, w64, pos, neg, et, ps, ns):
    """What fp32 evaluation may change in the objective, per triple, derived from the fp32 spacing (ps, ns: the fp64
    sigma of the positives and the negatives).  Negatives: the kernel's sigma = rcp(1 + exp(-s)); in [0.5, 1) the fp32
    spacing is U = 2^-24, the add rounds by <= U / 2, v_rcp_f32 errs by <= 1 ulp, forming 1 - sigma rounds by <= U / 2
    (exact there: Sterbenz), and the fp32 dot product moves s by at most ds = 2 k U sum_j |z_u z_v w|; so
    |(1 - sigma)_kernel - (1 - sigma)| <= D = 4 U + sigma (1 - sigma) ds.  With x = 1 - sigma + 1e-13 the term -log(x)
    is off by at most max(log(x + D) - log(x), log(x) - log(max(x - D, 1e-13))): about D e^s, large once 1 - sigma
    nears D (s ~ 17; above 17.3 fp32 rounds sigma to 1 and the term is -log(1e-13)).  Positives: x = sigma + 1e-13,
    sigma with relative error <= 4 U + ds (no cancellation).  Gradient coefficients (divided by n):
    sigma (1 - sigma) / (1 - sigma + 1e-13) of a negative is off by <= D + 4 U, except where 1 - sigma <= D (1 - sigma
    may round to 0): there by up to 1; (1 - sigma) sigma / (sigma + 1e-13) of a positive by <= D_pos + 4 U with
    D_pos = 4 U + sigma (4 U + ds) (the 1 - sigma of a positive cancels the same way).
    -> (bound on |loss error| before summation, coefficient bounds of the positives, of the negatives)."""
    k, m = z64.shape[1], ns.numel()
    dsp = 2 * k * U * (z64[pos[0]] * z64[pos[1]] * w64[et]).abs().sum(1)
    dsn = 2 * k * U * (z64[neg[0]] * z64[neg[1]] * w64[et]).abs().sum(1)
    xp, xn = ps + 1e-13, 1 - ns + 1e-13
    Dp, Dn = ps * (4 * U + dsp), 4 * U + ns * (1 - ns) * dsn
    tp = torch.maximum(torch.log(xp + Dp) - torch.log(xp), torch.log(xp) - torch.log((xp - Dp).clamp(min=1e-13)))
    tn = torch.maximum(torch.log(xn + Dn) - torch.log(xn), torch.log(xn) - torch.log((xn - Dn).clamp(min=1e-13)))
    cp = (4 * U + Dp + 4 * U) / m
    cn = torch.where(1 - ns <= Dn, torch.ones_like(ns), Dn + 4 * U) / m
    return float((tp + tn).sum()) / m, cp, cn


def objective_bounds(z, w, pos, neg, et, l64, ps, ns):
    """Derived bounds on |loss - fp64| and on |d z - fp64|, |d w - fp64| elementwise: fp32_bounds, plus the suite's 2e-5 of
    the loss and 1e-5 of each element's sum of |terms| for fp32 summation and products, plus the d z fixed point."""
    z64, w64 = z.double(), w.double()
    lb, cp, cn = fp32_bounds(z64, w64, pos, neg, et, ps, ns)
    gp, gn = O.tip_loss_bwd(ps, ns)
    az, aw = abs_terms((gp * ps * (1 - ps)).abs(), (gn * ns * (1 - ns)).abs(), z64, w64, pos, neg, et)
    bz, bw = abs_terms(cp, cn, z64, w64, pos, neg, et)
    return (lb + 2e-5 * abs(float(l64)), bz + 1e-5 * az + fixed_point_bound(z, w, pos, neg, ns.numel()),
            bw + 1e-5 * aw + 1e-12)


def fixed_point_bound(z, w, pos, neg, m):
    """What the 64-bit fixed point of d z can lose: a term is rounded to 2^-30 of tb = 4 zmax wmax / n_total (the scale is
    2^(30 - ilogb(tb) - 1) >= 2^29 / tb, round to nearest: <= 2^-30 tb per term), times the terms an element receives."""
    tb = 4 * float(z.abs().max()) * float(w.abs().max()) / m
    counts = torch.bincount(torch.cat([pos.flatten(), neg.flatten()]), minlength=z.shape[0]).double()
    return counts.unsqueeze(1) * (2.0 ** -30 * tb)


def band_inputs(k, pos_band, neg_band, seed=0):
    """z, w and triples whose positive scores s = sum z_u z_v w_r lie in -pos_band and negative scores in neg_band:
    positives pair a node of A (z > 0) with one of B (z < 0), negatives two nodes of C (z > 0), w > 0; a row is a
    constant times (1 + 2 % jitter), the constants drawn so that every score falls inside its band."""
    g = torch.Generator().manual_seed(seed)
    n_a, r, m = 200, 17, 30000
    n = 3 * n_a
    w = (0.7 + 0.3 * torch.rand(r, 1, generator=g)) * (1 + 0.02 * torch.rand(r, k, generator=g))
    et = torch.sort(torch.randint(0, r, (m,), generator=g)).values
    pos = torch.stack([torch.randint(0, n_a, (m,), generator=g), torch.randint(n_a, 2 * n_a, (m,), generator=g)])
    neg = torch.randint(2 * n_a, n, (2, m), generator=g)
    z = torch.empty(n, k)

    def fill(lo_row, lo, hi, sign):
        # |s| in [k a_lo^2 0.7, k a_hi^2 1.02^3]
        a_lo, a_hi = math.sqrt(lo / (0.7 * k)), math.sqrt(hi / (1.0613 * k))
        a = a_lo + (a_hi - a_lo) * torch.rand(n_a, 1, generator=g)
        z[lo_row:lo_row + n_a] = sign * a * (1 + 0.02 * torch.rand(n_a, k, generator=g))

    fill(0, pos_band[0], pos_band[1], 1.0)
    fill(n_a, pos_band[0], pos_band[1], -1.0)
    fill(2 * n_a, neg_band[0], neg_band[1], 1.0)
    ps = (z[pos[0]] * z[pos[1]] * w[et]).sum(1)
    ns = (z[neg[0]] * z[neg[1]] * w[et]).sum(1)
    assert pos_band[0] <= float(-ps.max()) and float(-ps.min()) <= pos_band[1]
    assert neg_band[0] <= float(ns.min()) and float(ns.max()) <= neg_band[1]
    return z, w, pos, neg, et


@pytest.mark.timeout(300)
@pytest.mark.parametrize('route,k', ROUTE_K)
def test_objective_score_bands(ops, route, k, monkeypatch):
    dev = lambda *t: [x.to(DEV) for x in t]                                       # noqa: E731
    # normal range |s| <= 8: fp64 at the suite's tolerances
    z, w, pos, neg, et = band_inputs(k, (0.5, 8.0), (0.5, 8.0))
    loss, gz, gw = objective(ops, route, *dev(z, w, pos, neg, et), monkeypatch)
    l64, gz64, gw64, _, _ = reference(z, w, pos, neg, et, torch.float64)
    close(loss, l64.view(1), rtol=2e-5)
    close(gz, gz64, atol=2e-6)
    close(gw, gw64, atol=2e-6)

    # full saturation: negatives s >= 18 (sigma rounds to 1 in fp32: the term is -log(1e-13), its coefficient 0) and
    # positives s <= -90 (sigma < 1e-39 << 1e-13: the same term, coefficient < 1e-26 / n): the float32 oracle, tightly.
    # (fp64 gives another loss here -- -log sigma(-90) = 90 -- that is the reference's arithmetic, not a kernel error.)
    z, w, pos, neg, et = band_inputs(k, (90.0, 400.0), (18.0, 60.0), seed=1)
    loss, gz, gw = objective(ops, route, *dev(z, w, pos, neg, et), monkeypatch)
    l32, gz32, gw32, _, _ = reference(z, w, pos, neg, et, torch.float32)
    assert abs(float(l32) + 2 * math.log(float(np.float32(1e-13)))) < 1e-5 * float(l32)
    close(loss, l32.view(1), rtol=1e-5)
    assert float(gz32.abs().max()) < 1e-20 and float(gw32.abs().max()) < 1e-20
    close(gz, gz32, rtol=0, atol=1e-20)
    close(gw, gw32, rtol=0, atol=1e-20)

    # partial band 8 < |s| < 18: fp32 keeps only a few bits of 1 - sigma here, so per-term disagreement is large and
    # legitimate; the kernel must stay within the bound derived from the fp32 spacing (fp32_bounds)
    z, w, pos, neg, et = band_inputs(k, (8.0, 18.0), (8.0, 18.0), seed=2)
    loss, gz, gw = objective(ops, route, *dev(z, w, pos, neg, et), monkeypatch)
    l64, gz64, gw64, ps, ns = reference(z, w, pos, neg, et, torch.float64)
    lb, bz, bw = objective_bounds(z, w, pos, neg, et, l64, ps, ns)
    err = abs(float(loss) - float(l64))
    dz, dw = (gz.cpu().double() - gz64).abs(), (gw.cpu().double() - gw64).abs()
    print('score band 8..18, %s k=%d: loss error %.3g (derived bound %.3g); d z, d w error / bound: max %.3g, %.3g'
          % (route, k, err, lb, float((dz / bz).max()), float((dw / bw).max())))
    assert err <= lb
    assert bool((dz <= bz).all()) and bool((dw <= bw).all())


def wide_range_inputs():
    """z rows from 1e-3 to 1 with one hub row at 1e2 (1e4 x the median row); w rows from 1e-3 to 1 with one at 1e2; every
    triple redrawn until |s| <= 8 (the test is about the d z accumulator, not about saturation)."""
    g = torch.Generator().manual_seed(5)
    n, r, k, m = 645, 40, 16, 60000
    z = torch.randn(n, k, generator=g) / math.sqrt(k) * torch.exp(torch.empty(n, 1).uniform_(math.log(1e-3), 0, generator=g))
    z[7] *= 1e2 / float(z[7].abs().max())
    w = torch.randn(r, k, generator=g) * torch.exp(torch.empty(r, 1).uniform_(math.log(1e-3), 0, generator=g))
    w[11] *= 1e2 / float(w[11].abs().max())
    et = torch.sort(torch.randint(0, r, (m,), generator=g)).values
    pairs = []
    for _ in range(2):
        p = torch.randint(0, n, (2, m), generator=g)
        for _ in range(50):
            bad = ((z[p[0]] * z[p[1]] * w[et]).sum(1).abs() > 8).nonzero().flatten()
            if bad.numel() == 0:
                break
            p[:, bad] = torch.randint(0, n, (2, bad.numel()), generator=g)
        assert bad.numel() == 0
        pairs.append(p)
    assert bool((pairs[0] == 7).any()) and bool((et == 11).any())
    return z, w, pairs[0], pairs[1], et


@pytest.mark.timeout(300)
def test_objective_wide_dynamic_range(ops, monkeypatch):
    """One large row of z or w coarsens the fixed-point d z of every row: every element stays within the derived bound
    (fixed_point_bound + 1e-5 of the element's sum of |terms| for the fp32 products); the float-atomic path, whose d z
    image has a 2^60 scale for the whole workgroup's sum, is reported next to it."""
    z, w, pos, neg, et = wide_range_inputs()
    m = pos.shape[1]
    l64, gz64, gw64, ps, ns = reference(z, w, pos, neg, et, torch.float64)
    z64, w64 = z.double(), w.double()
    gp, gn = O.tip_loss_bwd(ps, ns)
    az = abs_terms((gp * ps * (1 - ps)).abs(), (gn * ns * (1 - ns)).abs(), z64, w64, pos, neg, et)[0]
    fx = fixed_point_bound(z, w, pos, neg, m)
    bound = fx + 1e-5 * az
    small = z.abs().max(1).values < 1e-2                                          # the rows the hub coarsens
    assert int(small.sum()) > 100
    errs = {}
    for route in ROUTES:
        loss, gz, gw = objective(ops, route, z.to(DEV), w.to(DEV), pos.to(DEV), neg.to(DEV), et.to(DEV), monkeypatch)
        close(loss, l64.view(1), rtol=2e-5)
        close(gw, gw64, atol=2e-6 * max(1.0, float(gw64.abs().max())))
        dz = (gz.cpu().double() - gz64).abs()
        errs[route] = float(dz[small].max())
        if route != 'float_atomics':
            assert bool((dz <= bound).all()), float((dz / bound).max())
    print('wide range, small rows: max |d z - fp64| %s; derived bound there %.3g (fixed point %.3g); max |d z| %.3g'
          % (errs, float(bound[small].max()), float(fx[small].max()), float(gz64[small].abs().max())))


@pytest.mark.timeout(300)
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('where', ['z', 'w', 'z_unreferenced'])
def test_objective_non_finite_inputs(ops, bad, where, monkeypatch):
    """A NaN or an infinity in z or w makes the objective's loss NaN on every route, and d z non-finite: the fixed-point
    sums cannot carry a NaN, so the kernels flag non-finite values while they stage z and w and the conversion back
    yields NaN.  torch at fp32 gives a NaN loss for a NaN; for an infinity its loss stays finite (the scores saturate)
    but its gradients do not.  A z row that no pair references is flagged all the same (the kernels stage all of z):
    the loss is NaN where torch's is finite."""
    g = torch.Generator().manual_seed(9)
    n, r, m = 645, 20, 30000
    z = torch.randn(n, 16, generator=g) * 0.7
    w = torch.randn(r, 16, generator=g) * 0.5
    et = torch.sort(torch.randint(0, r, (m,), generator=g)).values
    pos = torch.randint(0, n - 1, (2, m), generator=g)
    neg = torch.randint(0, n - 1, (2, m), generator=g)                           # row n - 1: referenced by no pair
    if where == 'z':
        z[int(pos[0, 123]), 1] = bad
    elif where == 'w':
        w[int(et[m // 2]), 3] = bad
    else:
        z[n - 1, 2] = bad
    l32, gz32, _, _, _ = reference(z, w, pos, neg, et, torch.float32)
    if where == 'z_unreferenced':
        assert math.isfinite(float(l32))
    elif math.isnan(bad):
        assert math.isnan(float(l32))
    else:
        assert not bool(torch.isfinite(gz32).all())
    for route, k in ROUTE_K:
        args = (z[:, :k].contiguous().to(DEV), w[:, :k].contiguous().to(DEV), pos.to(DEV), neg.to(DEV), et.to(DEV))
        loss, gz, gw = objective(ops, route, *args, monkeypatch)
        assert math.isnan(float(loss)), (route, k, float(loss))
        assert not bool(torch.isfinite(gz).all()), (route, k)
        loss_only = objective(ops, route, *args, monkeypatch, need_grad=False)[0]
        assert math.isnan(float(loss_only)), (route, k, float(loss_only))


# ------------------------------------------------------------------ C.4 full BioSNAP against fp64
# max-norm relative error of d z / d w against fp64 at full size and the training test's scales, measured on an MI355X:
# 3.0e-7 / 7.5e-8 (loss: 6e-8 relative); the tolerances are 20 x / 27 x those
GZ_ATOL, GW_ATOL = 6e-6, 2e-6


@pytest.mark.timeout(600)
@pytest.mark.parametrize('scale', [1.0, 3.0])
def test_objective_full_biosnap_vs_fp64(ops, biosnap, scale, monkeypatch):
    """8.3 M triples, device-sampled negatives (fixed seed), k = 16, z and w at the training test's scales (0.5, 0.25)
    and 3 x those; int64 and packed negatives; mirrored positives on and off.  The fp64 oracle runs on the device (plain
    torch ops in float64: only the checker).  At 3 x the scores reach |s| ~ 30 and the fp32 objective saturates (the
    float32 oracle is 2 % off the fp64 loss there): loss and gradients are held to the bounds derived in fp32_bounds.
    (d w uses nearly all of its bound by construction: every negative above s = 17.3 has coefficient 0 in fp32 and just
    below 1 / n in fp64, and the bound allows 1 / n for each.)"""
    from tip_amd import neg_sampling as NS
    pos_np, n, rg = biosnap['pos_np'], biosnap['n'], biosnap['rg']
    pos = torch.from_numpy(pos_np).to(DEV)
    R = rg.shape[0]
    et = torch.repeat_interleave(torch.arange(R), rg[:, 1] - rg[:, 0]).to(DEV)
    neg = NS.typed_negative_sampling(pos, n, rg, seed=31)
    neg_p = NS.typed_negative_sampling(pos, n, rg, seed=31, packed=True)
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(n, 16, generator=g) * 0.5 * scale).to(DEV)
    w = (torch.randn(R, 16, generator=g) * 0.25 * scale).to(DEV)
    l64, gz64, gw64, ps, ns = reference(z, w, pos, neg, et, torch.float64)
    if scale != 1.0:
        lb, bz, bw = objective_bounds(z, w, pos, neg, et, l64, ps, ns)
        del ps, ns
    for sym in (True, False):
        if not sym:
            monkeypatch.setenv('TIPK_NO_SYMMETRIC_POS', '1')
        p = pos.clone()                                                 # a new tensor: a new task table
        assert bool((ops.relation_tasks(et, p)[:, 3] == 1).all()) != sym
        for ng in (neg, neg_p):
            loss, gz, gw = ops.distmult_loss(z, w, p, ng, et)
            if scale == 1.0:
                close(loss, l64.view(1), rtol=2e-5)
                close(gz, gz64, rtol=0, atol=GZ_ATOL * float(gz64.abs().max()))
                close(gw, gw64, rtol=0, atol=GW_ATOL * float(gw64.abs().max()))
            else:
                err = abs(float(loss) - float(l64))
                dz, dw = (gz.double() - gz64).abs(), (gw.double() - gw64).abs()
                print('full size x3 (sym %s, %s): loss error %.3g of %.4g (bound %.3g); d z, d w error / bound: %.3g, %.3g'
                      % (sym, ng.dtype, err, float(l64), lb, float((dz / bz).max()), float((dw / bw).max())))
                assert err <= lb
                assert bool((dz <= bz).all()) and bool((dw <= bw).all())
        monkeypatch.delenv('TIPK_NO_SYMMETRIC_POS', raising=False)
