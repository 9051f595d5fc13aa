"""fp64 specification of the drug fold-in (include/tipk.h section 4k) and the acceptance rule its results are held to.

With the frozen model's tables h_prot [n_prot, p], x0 [N, d0], h1 [N, d1], the parameters hgcn_w [p, pd], (basis1, att1, root1),
(basis2, att2, root2) and, per new drug m, xd_m [ne], its targets (t_m protein ids) and its interactions (deg_m pairs of an
existing drug and a relation, duplicates counted):
    pd_m = (1/max(t_m,1) * sum_{q in targets} h_prot[q]) @ hgcn_w
    x0_m = cat(xd_m, pd_m)  |  xd_m + pd_m
    h1_m = relu( 1/max(deg_m,1) * sum_e sum_b att1[rel_e,b] * (x0[src_e] @ basis1[b]) + x0_m @ root1 )
    z_m  =       1/max(deg_m,1) * sum_e sum_b att2[rel_e,b] * (h1[src_e] @ basis2[b]) + h1_m @ root2
`layer_row64` is one destination row of an R-GCN layer straight from this definition, `x0_row64` the first two lines;
`spec_fold_in` chains them in fp64.  `check_fold_in` holds a returned (x0_new, h1_new, z_new) to the acceptance rule, with
u = 2^-24 and gamma_m = m u / (1 - m u).  Every stage is evaluated in fp64 FROM THE PREVIOUS STAGE AS RETURNED (fp32 is exact in
fp64, so no error travels between stages) and bounded by gamma_m times the same formula on absolute values:
    x0_new : m = t_m + p + 3              (the sum over the targets, the reciprocal and its multiply, the chain over p, the add)
    h1_new : m = deg_m + B + d0 + 3       (the sum over the edges, over the bases, the chain over d0 -- the root chain is no
                                           longer --, the reciprocal, its multiply, the last add); ReLU is 1-Lipschitz, so the
                                           bound of the pre-activation carries over
    z_new  : m = deg_m + B + d1 + 3
The bounds are the standard ones for nested fp32 sums and hold for any summation order inside each sum: the rule skips nothing.
End to end, against the all-fp64 chain: |z_new - z64| <= tau_z + (tau_h1 + tau_x0 @ |root1|) @ |root2| -- an error of x0_m or
h1_m reaches the next stage through the root term alone, the neighbours' rows being held fixed.
"""
import torch

U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


def _cpu64(*ts):
    return tuple(t.detach().double().cpu() for t in ts)


def _ids(t):
    return torch.as_tensor(t).long().cpu().reshape(-1)


def layer_row64(table64, basis64, att64, root64, own64, src, rel, denom=None):
    """One destination row of the bias-free layer in fp64: table64 [N, d_in] holds the in-neighbours' rows, own64 [d_in] the
    node's own, (src, rel) its in-edges -> (row, the same formula on absolute values), float64 [d_out] each.
    denom: deg -> the mean's denominator (None = max(deg, 1), the definition)."""
    src, rel = _ids(src), _ids(rel)
    deg = src.numel()
    den = float(max(deg, 1) if denom is None else denom(deg))
    agg = torch.einsum('eb,ei->bi', att64[rel], table64[src])                      # A[b, :] = sum_e att[rel_e, b] x[src_e, :]
    agg_abs = torch.einsum('eb,ei->bi', att64[rel].abs(), table64[src].abs())
    row = torch.einsum('bi,bio->o', agg, basis64) / den + own64 @ root64
    row_abs = torch.einsum('bi,bio->o', agg_abs, basis64.abs()) / abs(den) + own64.abs() @ root64.abs()
    return row, row_abs


def x0_row64(xd64, h_prot64, hgcn_w64, targets, cat, denom=None):
    """The new drug's input row in fp64 -> (row, the same formula on absolute values), float64 [d0] each."""
    tg = _ids(targets)
    den = float(max(tg.numel(), 1) if denom is None else denom(tg.numel()))
    pd = (h_prot64[tg].sum(0) / den) @ hgcn_w64
    pd_abs = (h_prot64[tg].abs().sum(0) / abs(den)) @ hgcn_w64.abs()
    if cat:
        return torch.cat([xd64, pd]), torch.cat([xd64.abs(), pd_abs])
    return xd64 + pd, xd64.abs() + pd_abs


def _segments(csr):
    ptr = _ids(csr[0]).tolist()
    cols = [_ids(c) for c in csr[1:]]
    return [tuple(c[ptr[i]:ptr[i + 1]] for c in cols) for i in range(len(ptr) - 1)]


def spec_fold_in(h_prot, hgcn_w, x0, h1, layer1, layer2, xd, targets, interactions, cat, denom=None):
    """The all-fp64 chain -> (x0 [M, d0], h1 [M, d1], z [M, d2]) float64 on the host.  targets = (ptr, protein),
    interactions = (ptr, src, rel): the CSR lists of `ops.drug_fold_in`."""
    h_prot, hgcn_w, x0, h1, xd = _cpu64(h_prot, hgcn_w, x0, h1, xd)
    l1, l2 = _cpu64(*layer1), _cpu64(*layer2)
    rows = []
    for m, ((tg,), (src, rel)) in enumerate(zip(_segments(targets), _segments(interactions))):
        a = x0_row64(xd[m], h_prot, hgcn_w, tg, cat, denom)[0]
        b = torch.relu(layer_row64(x0, *l1, a, src, rel, denom)[0])
        rows.append((a, b, layer_row64(h1, *l2, b, src, rel, denom)[0]))
    if not rows:
        return tuple(torch.zeros(0, w, dtype=torch.float64) for w in (x0.shape[1], h1.shape[1], l2[2].shape[1]))
    return tuple(torch.stack([r[i] for r in rows]) for i in range(3))


def check_fold_in(h_prot, hgcn_w, x0, h1, layer1, layer2, xd, targets, interactions, cat, got, what=''):
    """Assert the acceptance rule for got = (x0_new [M, d0], h1_new [M, d1], z_new [M, d2]) (any device).
    -> dict: 'used_x0', 'used_h1', 'used_z', 'used_chain': the largest share of its bound each comparison used; 'tau_z' float64
    [M, d2], 'tau_h1' [M, d1]: the stage bounds of z and h1; 'z64' [M, d2]: the all-fp64 chain."""
    h_prot64, hgcn_w64, x064, h164, xd64 = _cpu64(h_prot, hgcn_w, x0, h1, xd)
    l1, l2 = _cpu64(*layer1), _cpu64(*layer2)
    g0, g1, g2 = (t.detach().cpu() for t in got)
    m_new, p = xd64.shape[0], h_prot64.shape[1]
    n_bases, d0, d1 = l1[0].shape[0], l1[0].shape[1], l2[0].shape[1]
    d2 = l2[0].shape[2]
    assert g0.shape == (m_new, d0) and g1.shape == (m_new, d1) and g2.shape == (m_new, d2), (what, 'shapes')
    assert g0.dtype == torch.float32 and g1.dtype == torch.float32 and g2.dtype == torch.float32, (what, 'dtypes')
    chain = spec_fold_in(h_prot, hgcn_w, x0, h1, layer1, layer2, xd, targets, interactions, cat)
    used = {'used_x0': 0.0, 'used_h1': 0.0, 'used_z': 0.0, 'used_chain': 0.0}
    tau_z, tau_h1 = torch.zeros(m_new, d2, dtype=torch.float64), torch.zeros(m_new, d1, dtype=torch.float64)

    def hold(key, have, want, tau, tag):
        err = (have.double() - want).abs()
        assert bool((err <= tau).all()), (tag, key, 'off fp64 by', float(err.max()), 'bound', float(tau.max()))
        used[key] = max(used[key], float((err / tau.clamp(min=1e-300)).max()))

    for m, ((tg,), (src, rel)) in enumerate(zip(_segments(targets), _segments(interactions))):
        tag = (what, 'new drug %d' % m)
        t_m, deg = tg.numel(), src.numel()
        want0, abs0 = x0_row64(xd64[m], h_prot64, hgcn_w64, tg, cat)
        tau0 = gamma(t_m + p + 3) * abs0
        hold('used_x0', g0[m], want0, tau0, tag)
        pre1, abs1 = layer_row64(x064, *l1, g0[m].double(), src, rel)               # from x0_new AS RETURNED
        tau1 = gamma(deg + n_bases + d0 + 3) * abs1
        hold('used_h1', g1[m], torch.relu(pre1), tau1, tag)
        want2, abs2 = layer_row64(h164, *l2, g1[m].double(), src, rel)              # from h1_new AS RETURNED
        tau2 = gamma(deg + n_bases + d1 + 3) * abs2
        hold('used_z', g2[m], want2, tau2, tag)
        tau_z[m], tau_h1[m] = tau2, tau1
        hold('used_chain', g2[m], chain[2][m], tau2 + (tau1 + tau0 @ l1[2].abs()) @ l2[2].abs(), tag)
    res = dict(used)
    res['tau_z'], res['tau_h1'], res['z64'] = tau_z, tau_h1, chain[2]
    return res
