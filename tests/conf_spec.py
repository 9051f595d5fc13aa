"""fp64 specification of the decoder-row posterior and the confidence top-k (include/tipk.h section 4p) and the acceptance
rules their results are held to.  Everything here works from the DEFINITION:

    row b:  posterior N(w_b, (P_b H_b)^-1),  H_b = L L^T,  W_b = P_b^(-1/2) L^-1 (lower triangular)
    triple: phi = z[u] * z[v],  s = phi . w_b,  var = phi^T (P_b H_b)^-1 phi = |W_b phi|^2
    key:    mode 0  s / sqrt(1 + pi/8 var)        mode 1  s + c sqrt(var)

FACTOR (`check_factor`).  The device's L and W, cast to fp64, are held entrywise to the classical backward bounds of Cholesky
and of forward substitution, which do not depend on the conditioning of H:
    |L L^T - H|   <= (dim + 1 + C_F) U (|L| |L^T|)
    |L W - r_b I| <= (dim + C_F) U (|L| |W|) + U r_b
with H the symmetric matrix of the LOWER triangle given (the entry reads nothing else), r_b = row_scale[b].  The strict upper
triangles are exact zeros; a row with status 0 is all zeros.

QUERY (`conf_tables`, `check_pair_conf`).  From (z, rel_w, W) in fp64 the rounding bounds of the arithmetic the header states
(phi rounded once, fma chains over j, the squares summed in a chain of at most dim / 4 + 2 <= dim + 2 roundings):
    tau_s   = (dim + 2) U sum_j |z_u z_v w|                                 (the tau of tests/pair_topk_spec.py)
    e_i     = (dim + 2) U sum_j |W_ij phi_j|
    tau_var = sum_i (2 |y_i| e_i + e_i^2) + (dim + 2) U sum_i y_i^2
    tau_key = tau_s and tau_var taken through the key function, with
              |sqrt a - sqrt b| <= min(|a - b| / (2 sqrt min(a, b)), sqrt |a - b|)   -- finite at var = 0:
      mode 0: d = sqrt(1 + a var), a = pi/8;  dd = the sqrt bound of a tau_var at min(.) >= 1 + a max(var - tau_var, 0);
              tau_key = tau_s / d_lo + |s| dd / (d d_lo),  d_lo = max(d - dd, 1)
      mode 1: tau_key = tau_s + |c| * (the sqrt bound of tau_var at min(.) >= max(var - tau_var, 0))
Every returned logit, variance and key lies within its tau + C_Q U |value| (the sqrt, the division, the last fma).
Selection: the five rules of tests/pair_topk_spec.py with the key in place of the logit and that bound in place of tau; the
padding is (-inf, -1, -inf, +inf).  A pair with an id outside [0, n) has a fully padded row and a dense row of (-inf, +inf).

END TO END (`check_end_to_end`).  The fp64 pipeline starts from the device's Hessian cast to fp64 (the statistics kernel has
its own tests): |var32 - var64| <= tau_var + C_E dim U kappa_2(H) var64, kappa_2 from torch.linalg.eigvalsh.  The spec asserts
dim U kappa_2 <= 2^-10 for every case it is given, so the bound never goes vacuous.

C_F, C_Q, C_E follow the project's rule: at most 30 x the largest excess measured on an MI355X and not below 4; with
TIPK_ERRLOG set every check prints and logs the excess it saw.  Measured (profiles/pair_confidence.md): the largest excess
was -0.05 for the factor (in units of U |L||.| beyond the dim terms), -2.7 for the query (units of U |value| beyond tau) and
-0.06 for the end-to-end rule (units of dim U kappa_2 var) -- every error stayed inside the tau and dim terms alone -- so all
three constants are the floor of the rule.
"""
import json
import math
import os

import torch

from pair_topk_spec import U, known_mask

C_F = 4.0
C_Q = 4.0
C_E = 4.0
PI8 = math.pi / 8
KAPPA_CAP = 2.0 ** -10


def _log(what, case, observed, c):
    if os.environ.get('TIPK_ERRLOG') and observed > float('-inf'):
        line = {'what': what, 'case': case, 'observed_c': observed, 'c': c}
        print('ERR %s' % json.dumps(line))
        with open(os.environ['TIPK_ERRLOG'], 'a') as f:
            f.write(json.dumps(line) + '\n')


def logical(w_phys):
    """The lower-triangular W [B, dim, dim] of the physical (transposed) layout of `ops.spd_factor`."""
    return w_phys.transpose(-1, -2)


def sym_lower(h):
    """The symmetric matrix whose lower triangle is that of h [..., dim, dim]."""
    lo = torch.tril(h)
    return lo + torch.tril(h, -1).transpose(-1, -2)


def posterior64(hess, n_pairs):
    """(L, W logical) in fp64 of hess [B, dim, dim] (lower triangle) and P_b = n_pairs [B]: W = P^(-1/2) chol(H)^-1."""
    h = sym_lower(hess.double())
    chol = torch.linalg.cholesky(h)
    eye = torch.eye(h.shape[-1], dtype=torch.float64, device=h.device).expand_as(h)
    inv = torch.linalg.solve_triangular(chol, eye, upper=False)
    return chol, inv * n_pairs.double().reshape(-1, 1, 1).rsqrt()


def check_factor(hess, row_scale, got, c_f=C_F, what=''):
    """Assert the factor rules for got = (L, W physical, status) of `ops.spd_factor` -> the largest excess over the dim
    terms that a good row needed (in units of U |L||.|; -inf without a good row)."""
    out_l, out_w, status = got
    dev = hess.device
    b, dim = hess.shape[0], hess.shape[-1]
    assert out_l.dtype == torch.float32 and out_w.dtype == torch.float32 and status.dtype == torch.int32
    assert out_l.shape == hess.shape and out_w.shape == hess.shape and tuple(status.shape) == (b,)
    if b == 0:
        return float('-inf')
    good = status.to(dev) == 1
    assert bool(((status == 0) | (status == 1)).all()), (what, 'status is 0 or 1')
    assert bool((out_l[~good] == 0).all()) and bool((out_w[~good] == 0).all()), (what, 'a bad row is all zeros')
    lw = logical(out_w)
    upper = torch.triu(torch.ones((dim, dim), dtype=torch.bool, device=dev), 1)
    assert bool((out_l[:, upper] == 0).all()) and bool((lw[:, upper] == 0).all()), (what, 'strict upper triangle is zero')
    assert not bool(torch.signbit(out_l[:, upper]).any()) and not bool(torch.signbit(lw[:, upper]).any()), (what, '+0.0')
    if not bool(good.any()):
        return float('-inf')
    h = sym_lower(hess.double())[good]
    l64, w64 = out_l.double()[good], lw.double()[good]
    r = row_scale.double().to(dev)[good].abs().reshape(-1, 1, 1)
    eye = torch.eye(dim, dtype=torch.float64, device=dev)
    assert bool(torch.isfinite(l64).all()) and bool(torch.isfinite(w64).all()), (what, 'a good row is finite')
    assert bool((l64.diagonal(dim1=1, dim2=2) > 0).all()), (what, 'positive diagonal')
    res1 = (l64 @ l64.transpose(1, 2) - h).abs()
    a1 = l64.abs() @ l64.abs().transpose(1, 2)
    res2 = (l64 @ w64 - row_scale.double().to(dev)[good].reshape(-1, 1, 1) * eye).abs()
    a2 = l64.abs() @ w64.abs()
    worst = max(float((res1 / (U * a1) - (dim + 1))[a1 > 0].max()),
                float(((res2 - U * r) / (U * a2) - dim)[a2 > 0].max()))
    _log('factor c', what, worst, c_f)
    assert bool((res1 <= (dim + 1 + c_f) * U * a1).all()), (what, 'L L^T off H', float((res1 - (dim + 1 + c_f) * U * a1).max()))
    assert bool((res2 <= (dim + c_f) * U * a2 + U * r).all()), (what, 'L W off r I', float((res2 - (dim + c_f) * U * a2 - U * r).max()))
    return worst


def _sqrt_bound(t, lo):
    """|sqrt a - sqrt b| for |a - b| <= t, min(a, b) >= lo >= 0."""
    first = torch.where(lo > 0, t / (2 * lo.clamp(min=1e-300).sqrt()), torch.full_like(t, float('inf')))
    return torch.minimum(first, t.sqrt())


def key_of(s, var, mode, c):
    return s / (1 + PI8 * var).sqrt() if mode == 0 else s + c * var.sqrt()


def conf_tables(z, rel_w, w_log, u, v, mode, c):
    """fp64 tables [P, R] of the pairs (u, v) (int64, in range): s, var, key and tau_s, tau_var, tau_key.
    w_log: the LOGICAL lower-triangular factors [R, dim, dim] (any float dtype)."""
    z64, w64, fac = z.double(), rel_w.double(), w_log.double()
    dim = z64.shape[1]
    phi = z64[u] * z64[v]
    s = phi @ w64.t()
    tau_s = (dim + 2) * U * (phi.abs() @ w64.abs().t())
    y = torch.einsum('rij,pj->pri', fac, phi)
    e = (dim + 2) * U * torch.einsum('rij,pj->pri', fac.abs(), phi.abs())
    var = (y * y).sum(-1)
    tau_var = (2 * y.abs() * e + e * e).sum(-1) + (dim + 2) * U * var
    key = key_of(s, var, mode, c)
    if mode == 0:
        d = (1 + PI8 * var).sqrt()
        dd = _sqrt_bound(PI8 * tau_var, 1 + PI8 * (var - tau_var).clamp(min=0))
        d_lo = (d - dd).clamp(min=1.0)
        tau_key = tau_s / d_lo + s.abs() * dd / (d * d_lo)
    else:
        tau_key = tau_s + abs(c) * _sqrt_bound(tau_var, (var - tau_var).clamp(min=0))
    return {'s': s, 'var': var, 'key': key, 'tau_s': tau_s, 'tau_var': tau_var, 'tau_key': tau_key}


def spec_pair_conf(z, rel_w, w_log, pairs, k, mode, c, known=None):
    """The exact fp64 confidence top-k on the host -> (key, relation int64, logit, var) [P, k], padded; tiny cases."""
    pairs = torch.as_tensor(pairs).cpu().long().reshape(2, -1)
    n, n_rel = z.shape[0], rel_w.shape[0]
    t = conf_tables(z.cpu(), rel_w.cpu(), w_log.cpu(), pairs[0], pairs[1], mode, c)
    km = known_mask(known, pairs[0], pairs[1], n, n_rel)
    p = pairs.shape[1]
    out = (torch.full((p, k), float('-inf'), dtype=torch.float64), torch.full((p, k), -1, dtype=torch.int64),
           torch.full((p, k), float('-inf'), dtype=torch.float64), torch.full((p, k), float('inf'), dtype=torch.float64))
    for i in range(p):
        cands = sorted((-float(t['key'][i, r]), r) for r in range(n_rel) if not bool(km[i, r]))
        for j, (_, r) in enumerate(cands[:k]):
            out[0][i, j], out[1][i, j], out[2][i, j], out[3][i, j] = t['key'][i, r], r, t['s'][i, r], t['var'][i, r]
    return out


def check_pair_conf(z, rel_w, w_phys, pairs, k, mode, c, got, known=None, c_q=C_Q, what='', chunk=2048):
    """Assert the query rules for got = (key, relation, logit, var [P, k], dense_logit, dense_var [P, R] or None) of
    `ops.distmult_pair_conf_topk`, on the device of z -> the largest excess over tau seen (units of U |value|)."""
    dev = z.device
    pairs = torch.as_tensor(pairs).to(dev).long().reshape(2, -1)
    n, n_rel, dim = z.shape[0], rel_w.shape[0], z.shape[1]
    w_log = logical(w_phys)
    big_p = pairs.shape[1]
    key_all, r_all, s_all, v_all = got[0].to(dev), got[1].to(dev).long(), got[2].to(dev), got[3].to(dev)
    dl_all, dv_all = got[4], got[5]
    for x in (key_all, r_all, s_all, v_all):
        assert tuple(x.shape) == (big_p, k), (what, tuple(x.shape), (big_p, k))
    assert (dl_all is None) == (dv_all is None)
    if dl_all is not None:
        assert tuple(dl_all.shape) == (big_p, n_rel) and tuple(dv_all.shape) == (big_p, n_rel)
    slot = torch.arange(k, device=dev)
    worst = float('-inf')

    def excess(off, tau, val):
        pos = val.abs() > 0
        return float(((off - tau) / (U * val.abs()))[pos].max()) if bool(pos.any()) else float('-inf')

    for p0 in range(0, big_p, chunk):
        u, v = pairs[0, p0:p0 + chunk], pairs[1, p0:p0 + chunk]
        inr = (u >= 0) & (u < n) & (v >= 0) & (v < n)
        uc, vc = u.clamp(0, n - 1), v.clamp(0, n - 1)
        key, r, s, var = (x[p0:p0 + chunk] for x in (key_all, r_all, s_all, v_all))
        t = conf_tables(z, rel_w, w_log, uc, vc, mode, c)
        b_key = t['tau_key'] + c_q * U * t['key'].abs()
        b_s = t['tau_s'] + c_q * U * t['s'].abs()
        b_var = t['tau_var'] + c_q * U * t['var']
        km = known_mask(known, uc, vc, n, n_rel)
        n_cand = torch.where(inr, (~km).sum(1), torch.zeros_like(u))
        # dense, entry by entry
        if dl_all is not None:
            dl, dv = dl_all[p0:p0 + chunk].to(dev), dv_all[p0:p0 + chunk].to(dev)
            assert bool(torch.isneginf(dl[~inr]).all()) and bool(torch.isposinf(dv[~inr]).all()), (what, 'dense row of a bad pair')
            off_s, off_v = (dl.double() - t['s']).abs(), (dv.double() - t['var']).abs()
            assert bool((off_s <= b_s)[inr].all()), (what, p0, 'dense logit off fp64', float((off_s - b_s)[inr].max()))
            assert bool((off_v <= b_var)[inr].all()), (what, p0, 'dense var off fp64', float((off_v - b_var)[inr].max()))
            assert bool((dv >= 0)[inr].all()), (what, 'variance >= 0')
            if bool(inr.any()):
                worst = max(worst, excess(off_s[inr], t['tau_s'][inr], t['s'][inr]), excess(off_v[inr], t['tau_var'][inr], t['var'][inr]))
        if k == 0:
            continue
        # 5. padding
        nv = (r >= 0).sum(1)
        valid = slot[None, :] < nv[:, None]
        assert bool(((r >= 0) == valid).all()), (what, p0, 'padding: valid entries are not a prefix')
        assert bool((r[~valid] == -1).all()) and bool(torch.isneginf(key[~valid]).all()) \
            and bool(torch.isneginf(s[~valid]).all()) and bool(torch.isposinf(var[~valid]).all()), (what, p0, 'padding values')
        assert bool((nv == n_cand.clamp(max=k)).all()), (what, p0, 'returned count is not min(k, candidates)')
        # 1. range, known, distinct
        assert bool((r[valid] < n_rel).all()), (what, p0, 'relation out of range')
        rc = r.clamp(min=0, max=n_rel - 1)
        assert not bool(km.gather(1, rc)[valid].any()), (what, p0, 'known relation returned')
        hits = torch.zeros((u.numel(), n_rel), dtype=torch.int32, device=dev)
        hits.scatter_add_(1, rc, valid.to(torch.int32))
        assert (int(hits.max()) <= 1) if hits.numel() else True, (what, p0, 'duplicate relation')
        # 2. values
        for name, x, ref, bound, tau in (('key', key, t['key'], b_key, t['tau_key']), ('logit', s, t['s'], b_s, t['tau_s']),
                                         ('var', var, t['var'], b_var, t['tau_var'])):
            x64, bd = ref.gather(1, rc), bound.gather(1, rc)
            off = (x.double() - x64).abs()
            assert bool((off <= bd)[valid].all()), (what, p0, name + ' off fp64', float((off - bd)[valid].max()))
            if bool(valid.any()):
                worst = max(worst, excess(off[valid], tau.gather(1, rc)[valid], x64[valid]))
        assert bool((var >= 0)[valid].all()), (what, 'variance >= 0')
        # 3. order
        if k > 1:
            ok = (key[:, :-1] > key[:, 1:]) | ((key[:, :-1] == key[:, 1:]) & (r[:, :-1] < r[:, 1:]))
            assert bool(ok[valid[:, 1:]].all()), (what, p0, 'order')
        # 4. completeness of full rows
        full = nv == k
        if bool(full.any()):
            k64, kb = t['key'].gather(1, rc), b_key.gather(1, rc)
            bound = k64[:, k - 1] + kb[:, k - 1]
            missing = ~km & (hits == 0)
            low = (t['key'] - b_key).masked_fill(~missing, float('-inf')).amax(1)
            assert bool((low <= bound)[full].all()), (what, p0, 'a better relation is missing', float((low - bound)[full].max()))
    _log('query c', what, worst, c_q)
    return worst


def kappa2(hess):
    """kappa_2 [B] of the symmetric matrices of the lower triangles of hess, in fp64."""
    ev = torch.linalg.eigvalsh(sym_lower(hess.double()))
    return ev[:, -1] / ev[:, 0]


def check_end_to_end(z, rel_w, hess32, n_pairs, u, v, var32, c_e=C_E, what=''):
    """Assert |var32 - var64| <= tau_var + C_E dim U kappa_2(H) var64 for var32 [P, B], the device's variances from
    (statistics -> factor -> query); the fp64 pipeline starts from the device's Hessian hess32 -> the largest excess."""
    dim = z.shape[1]
    kap = kappa2(hess32)
    assert bool((dim * U * kap <= KAPPA_CAP).all()), (what, 'dim U kappa_2 above 2^-10', float((dim * U * kap).max()))
    _, w64 = posterior64(hess32, n_pairs.to(hess32.device))
    t = conf_tables(z, rel_w, w64, u, v, 1, 0.0)
    off = (var32.double() - t['var']).abs()
    room = dim * U * kap[None, :] * t['var']
    pos = room > 0
    worst = float(((off - t['tau_var']) / room)[pos].max()) if bool(pos.any()) else float('-inf')
    _log('end to end c', what, worst, c_e)
    assert bool((off <= t['tau_var'] + c_e * room).all()), (what, 'var off fp64', float((off - t['tau_var'] - c_e * room).max()), worst)
    return worst
