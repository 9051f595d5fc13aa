"""fp64 specification of the protein attribution (include/tipk.h section 4o) and the acceptance rule its results are held to.

Operands: hp [P, p], W_pd [p, pd], the P -> D edges (protein t_e -> drug i_e, duplicates count), cnt_i = max(number of
P -> D edges into drug i, 1), xe [N, ne], cat | add, layer l = (basis_l [B, d_{l-1}, d_l], att_l [R, B], root_l), the stored
h [N, d1] with the mask m = (h > 0), and the D-D edges (src, dst, rel) with deg_j = max(in-degree of j, 1).
    pair cells   C_l[i, j, b] = 1/deg_j * sum_{e: i -> j} att_l[rel_e, b]                  (an explicit loop over the edges)
    G2[b, :]  = basis2[b] g
    a2[j, :]  = sum_b C2[j, v, b] G2[b, :] + [j = v] root2 g
    a1        = a2 * m
    U[i,b,:]  = sum_j C1[i, j, b] a1[j, :]
    a0[i, :]  = sum_b basis1[b] U[i, b, :] + root1 a1[i]
    a0e, a0p  = a0[:, :ne], a0[:, ne:]  (cat)   |   a0, a0  (add)
    own_i     = a0e[i] . xe[i]
    qv[i, :]  = W_pd a0p[i]
    c_{t,i}   = sum_{P -> D edges e = (t -> i)} 1/cnt_i * hp[t] . qv[i];   c_t = sum_i c_{t,i};   direct_t = c_{t,v}
and g . z[v] = sum_i own_i + sum_t c_t.  Candidates: the proteins with at least one P -> D edge.

The acceptance rule (`check_protein_attribution`), u = 2^-24, gamma_m = m u / (1 - m u).  S_t, S_i and S_direct are the SAME
pipeline run on the absolute value of every operand (g, basis, att, root, hp, W_pd, xe) with the mask unchanged -- the sum of
the magnitudes of every product that c_t, own_i, direct_t add up.  The standard bound for nested fp32 sums says: a value
computed through a chain of stages, stage s adding n_s products or terms with n_s roundings, differs from the exact value by
at most gamma_(sum n_s) times its abs-pipeline value, in ANY summation order.  The stages from g to c_t, and their lengths:
    G2                 d2                     one product-sum over d2
    a cell             mult + 2               mult - 1 adds, the reciprocal, one multiply (mult = the largest pair multiplicity);
                                              TWICE: C2 enters a2 and C1 enters U
    a2                 B + 2                  B products, the root term's add (the mask is exact)
    U                  N                      N products
    a0                 B d1 + d1              one chain over (b, o) and root1's o
    qv                 pd
    c_t                p x entries_t + 2      entries_t dot products of p, the reciprocal 1/cnt and its multiply, the adds
                                              over the entries (entries_t - 1 <= the slack of p x entries_t over p + entries_t
                                              for p >= 2; the + 2 covers p = 1 and a single entry)
so m_t = d2 + 2 (mult + 2) + (B + 2) + N + (B d1 + d1) + pd + p entries_t + 2 and tau_t = gamma_(m_t) S_t; direct_t is a part of
the same sum: tau_direct = gamma_(m_t) S_direct.  own_i ends in a product-sum over ne instead of the last two stages:
m_own = d2 + 2 (mult + 2) + (B + 2) + N + (B d1 + d1) + ne, tau_own_i = gamma_(m_own) S_i.  Nothing is measured, nothing tuned.
  1. every listed protein is a candidate and is listed once;
  2. each listed value is within tau_t, and each listed direct within tau_direct, of its fp64 value;
  3. the list is ordered: value descending, ties by ascending protein id;
  4. no unlisted candidate has an fp64 value above the k-th listed fp64 value plus the two taus;
  5. padding (-inf, -1, +0) fills exactly the slots beyond the candidate count;
  6. |features - sum own64| <= sum tau_own + u |sum own64|,  |proteins - sum c64| <= sum tau_t + u |sum c64|.
A node outside [0, N): a fully padded row with NaN features and proteins.  The rule skips nothing.
"""
from collections import namedtuple

import torch

U = 2.0 ** -24

# fp32 operands on the host; dd = (src, dst, rel) int64 [E]; pd_edges = (prot, drug) int64 [Epd]
Operands = namedtuple('Operands', ['hp', 'w_pd', 'xe', 'h', 'layer1', 'layer2', 'dd', 'pd_edges', 'cat'])


def gamma(m):
    return m * U / (1.0 - m * U)


def _d(t):
    return t.detach().double().cpu()


def cells64(att64, dd, n):
    """C[i, j, b] by an explicit loop over the edges, then 1/deg_j."""
    src, dst, rel = (t.tolist() for t in dd)
    C = torch.zeros(n, n, att64.shape[1], dtype=torch.float64)
    deg = torch.zeros(n, dtype=torch.float64)
    for s, t, r in zip(src, dst, rel):
        C[s, t] += att64[r]
        deg[t] += 1
    return C / deg.clamp(min=1)[None, :, None]


def pair_multiplicity(dd, n):
    if dd[0].numel() == 0:
        return 1
    return max(1, int(torch.bincount(dd[1] * n + dd[0]).max()))


class Pipeline(object):
    """The query-independent part, once per case: the cells of both layers and the P -> D lists, as given or in magnitude."""

    def __init__(self, op, absolute=False):
        f = (lambda t: _d(t).abs()) if absolute else _d
        self.hp, self.w_pd, self.xe = f(op.hp), f(op.w_pd), f(op.xe)
        self.b1, self.a1, self.r1 = (f(t) for t in op.layer1)
        self.b2, self.a2, self.r2 = (f(t) for t in op.layer2)
        self.mask = (op.h.detach().cpu() > 0).double()
        self.n, self.ne = self.xe.shape
        self.cat = bool(op.cat)
        self.C1, self.C2 = cells64(self.a1, op.dd, self.n), cells64(self.a2, op.dd, self.n)
        self.prot, self.drug = op.pd_edges[0].long().cpu(), op.pd_edges[1].long().cpu()
        self.n_prot = self.hp.shape[0]
        self.cnt = torch.bincount(self.drug, minlength=self.n).clamp(min=1).double()
        self.absolute = absolute

    def query(self, v, g):
        """(own [N], c [P], direct [P]) of the query (v, g), float64."""
        g = _d(g).abs() if self.absolute else _d(g)
        G2 = self.b2 @ g                                                   # [B, d1]
        a2 = self.C2[:, v, :] @ G2                                         # [N, d1]
        a2[v] += self.r2 @ g
        a1 = a2 * self.mask
        Uq = torch.einsum('ijb,jo->ibo', self.C1, a1)                      # [N, B, d1]
        a0 = torch.einsum('bco,ibo->ic', self.b1, Uq) + a1 @ self.r1.t()   # [N, d0]
        a0e, a0p = (a0[:, :self.ne], a0[:, self.ne:]) if self.cat else (a0, a0)
        own = (a0e * self.xe).sum(1)
        qv = a0p @ self.w_pd.t()                                           # [N, p]
        per_edge = (self.hp[self.prot] * qv[self.drug]).sum(1) / self.cnt[self.drug]
        c = torch.zeros(self.n_prot, dtype=torch.float64).index_add_(0, self.prot, per_edge)
        mine = self.drug == v
        direct = torch.zeros(self.n_prot, dtype=torch.float64).index_add_(0, self.prot[mine], per_edge[mine])
        return own, c, direct


class Spec(object):
    """The exact values and the taus of a case: `values(v, g)` -> dict(own, c, direct, tau_own [N], tau, tau_direct [P],
    cand bool [P]) float64."""

    def __init__(self, op):
        self.exact, self.mag = Pipeline(op), Pipeline(op, absolute=True)
        e = self.exact
        self.n, self.n_prot = e.n, e.n_prot
        self.entries = torch.bincount(e.prot, minlength=e.n_prot)
        self.cand = self.entries > 0
        B, d1, d2 = e.b2.shape
        p, pd = e.w_pd.shape
        mult = pair_multiplicity(tuple(t.long().cpu() for t in op.dd), e.n)
        common = d2 + 2 * (mult + 2) + (B + 2) + e.n + (B * d1 + d1)
        self.m_own = common + e.ne
        self.m_t = common + pd + p * self.entries.double() + 2

    def values(self, v, g):
        own, c, direct = self.exact.query(v, g)
        s_i, s_t, s_d = self.mag.query(v, g)
        gm = gamma(self.m_t)
        return {'own': own, 'c': c, 'direct': direct, 'tau_own': gamma(self.m_own) * s_i, 'tau': gm * s_t,
                'tau_direct': gm * s_d, 'cand': self.cand, 'S': float(s_i.sum() + s_t[self.cand].sum())}


def spec_protein_attribution(spec, q_node, probe, k):
    """The exact fp64 attribution of every query -> (contrib float64 [Q, k], protein int64 [Q, k], direct float64 [Q, k],
    features float64 [Q], proteins float64 [Q]); padding (-inf, -1, 0); a node out of range: padding and NaN."""
    nodes = [int(x) for x in torch.as_tensor(q_node).tolist()]
    Q = len(nodes)
    out_c = torch.full((Q, k), float('-inf'), dtype=torch.float64)
    out_p = torch.full((Q, k), -1, dtype=torch.int64)
    out_d = torch.zeros((Q, k), dtype=torch.float64)
    feat = torch.full((Q,), float('nan'), dtype=torch.float64)
    prot = torch.full((Q,), float('nan'), dtype=torch.float64)
    for i, v in enumerate(nodes):
        if v < 0 or v >= spec.n:
            continue
        e = spec.values(v, probe[i])
        ids = torch.nonzero(e['cand']).reshape(-1).tolist()
        feat[i], prot[i] = float(e['own'].sum()), float(e['c'][e['cand']].sum())
        order = sorted((t for t in ids if e['c'][t] == e['c'][t]), key=lambda t: (-float(e['c'][t]), t))[:k]
        for slot, t in enumerate(order):
            out_c[i, slot], out_p[i, slot], out_d[i, slot] = e['c'][t], t, e['direct'][t]
    return out_c, out_p, out_d, feat, prot


def check_protein_attribution(spec, q_node, probe, k, got, what=''):
    """Assert the acceptance rule for got = (contrib [Q, k], protein [Q, k], direct [Q, k], features [Q], proteins [Q]) (any
    device).  -> dict of float64 [Q] tensors 'features64', 'proteins64', 'tau_features', 'tau_proteins', 'S' (NaN / 0 for a
    node out of range) and the largest shares of tau used ('used_value', 'used_direct', 'used_features', 'used_proteins')."""
    nodes = [int(x) for x in torch.as_tensor(q_node).tolist()]
    Q = len(nodes)
    c_all, p_all, d_all, f_all, s_all = (t.detach().cpu() for t in got)
    assert c_all.shape == (Q, k) and p_all.shape == (Q, k) and d_all.shape == (Q, k), (what, 'list shapes')
    assert f_all.shape == (Q,) and s_all.shape == (Q,), (what, 'features / proteins shapes')
    res = {key: torch.zeros(Q, dtype=torch.float64) for key in ('features64', 'proteins64', 'tau_features', 'tau_proteins', 'S')}
    used = {'used_value': 0.0, 'used_direct': 0.0, 'used_features': 0.0, 'used_proteins': 0.0}
    tiny = 1e-300
    for i, v in enumerate(nodes):
        tag = (what, 'query %d node %d' % (i, v))
        cv, pv, dv = c_all[i].double(), p_all[i].long(), d_all[i].double()
        if v < 0 or v >= spec.n:
            assert bool(torch.isneginf(cv).all()) and bool((pv == -1).all()) and bool((dv == 0).all()), (tag, 'padded row')
            assert f_all[i] != f_all[i] and s_all[i] != s_all[i], (tag, 'NaN features and proteins')
            res['features64'][i] = res['proteins64'][i] = float('nan')
            continue
        e = spec.values(v, probe[i])
        c64, tau, cand = e['c'], e['tau'], e['cand']
        n_cand = int(cand.sum())
        # 5. padding fills exactly the slots beyond the candidate count
        nv = int((pv >= 0).sum())
        assert nv == min(k, n_cand), (tag, 'listed %d of %d candidates (k = %d)' % (nv, n_cand, k))
        assert bool((pv[:nv] >= 0).all()) and bool((pv[nv:] == -1).all()), (tag, 'padding ids')
        assert bool(torch.isneginf(cv[nv:]).all()) and bool((dv[nv:] == 0).all()), (tag, 'padding values')
        ids = pv[:nv]
        # 1. candidates, listed once
        assert bool((ids < spec.n_prot).all()) and bool(cand[ids].all()), (tag, 'a listed protein is no candidate')
        assert torch.unique(ids).numel() == nv, (tag, 'a protein is listed twice')
        # 2. values and direct
        err, err_d = (cv[:nv] - c64[ids]).abs(), (dv[:nv] - e['direct'][ids]).abs()
        assert bool((err <= tau[ids]).all()), (tag, 'value off fp64', float(err.max()))
        assert bool((err_d <= e['tau_direct'][ids]).all()), (tag, 'direct off fp64', float(err_d.max()))
        if nv:
            used['used_value'] = max(used['used_value'], float((err / tau[ids].clamp(min=tiny)).max()))
            used['used_direct'] = max(used['used_direct'], float((err_d / e['tau_direct'][ids].clamp(min=tiny)).max()))
        # 3. order
        if nv > 1:
            lv = c_all[i][:nv]
            ok = (lv[:-1] > lv[1:]) | ((lv[:-1] == lv[1:]) & (ids[:-1] < ids[1:]))
            assert bool(ok.all()), (tag, 'order')
        # 4. completeness
        if nv == k and n_cand > k:
            missing = cand.clone()
            missing[ids] = False
            bound = float(c64[ids[-1]] + tau[ids[-1]])
            worst = float((c64 - tau)[missing].max())
            assert worst <= bound, (tag, 'a larger contribution is missing', worst, bound)
        # 6. the two totals
        f64, s64 = float(e['own'].sum()), float(c64[cand].sum())
        tau_f, tau_s = float(e['tau_own'].sum()), float(tau[cand].sum())
        d_f, d_s = abs(float(f_all[i]) - f64), abs(float(s_all[i]) - s64)
        assert d_f <= tau_f + U * abs(f64), (tag, 'features off fp64', d_f, tau_f)
        assert d_s <= tau_s + U * abs(s64), (tag, 'proteins off fp64', d_s, tau_s)
        used['used_features'] = max(used['used_features'], d_f / max(tau_f + U * abs(f64), tiny))
        used['used_proteins'] = max(used['used_proteins'], d_s / max(tau_s + U * abs(s64), tiny))
        res['features64'][i], res['proteins64'][i], res['tau_features'][i], res['tau_proteins'][i] = f64, s64, tau_f, tau_s
        res['S'][i] = e['S']
    res.update(used)
    return res


def forward64(hp, w_pd, xe, layer1, layer2, dd, pd_edges, cat):
    """The encoder's drug side in fp64, straight from the definitions (differentiable torch ops): -> (x0, h, z)."""
    n = xe.shape[0]
    prot, drug = pd_edges[0].long(), pd_edges[1].long()
    cnt = torch.bincount(drug, minlength=n).clamp(min=1).double()
    pd = torch.zeros(n, w_pd.shape[1], dtype=torch.float64).index_add_(0, drug, hp[prot] @ w_pd) / cnt[:, None]
    x0 = torch.cat([xe, pd], 1) if cat else xe + pd
    src, dst, rel = (t.long() for t in dd)
    deg = torch.bincount(dst, minlength=n).clamp(min=1).double()

    def layer(x, basis, att, root):
        W = torch.einsum('rb,bio->rio', att, basis)
        msg = torch.einsum('ei,eio->eo', x[src], W[rel])
        return torch.zeros(n, basis.shape[2], dtype=torch.float64).index_add_(0, dst, msg) / deg[:, None] + x @ root

    h = torch.relu(layer(x0, *layer1))
    return x0, h, layer(h, *layer2)
