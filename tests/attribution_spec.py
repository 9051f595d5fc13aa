"""fp64 specification of the R-GCN edge attribution (include/tipk.h section 4j) and the acceptance rule its results are held
to.

With h [n, d_in], basis [B, d_in, d_out], att [R, B], root [d_in, d_out], the in-edge CSR (in_ptr, in_src, in_rel) of
`ops.in_edges_by_node` and a query (node v, probe g):
    c_e = 1/max(deg_v, 1) * sum_b att[rel_e, b] * sum_i h[src_e, i] * sum_o basis[b, i, o] g[o]     per in-edge e of v
    own = sum_i h[v, i] * sum_o root[i, o] g[o]                         and       g . z[v] = own + sum_e c_e.
`spec_attribution` ranks all in-edges of every query exactly in fp64 (value descending, position in the segment ascending):
the spec itself.  `check_attribution` holds a returned result to the acceptance rule, with u = 2^-24 and
gamma_m = m u / (1 - m u):
  tau_e   = gamma_(d_out + d_in + B + 2) * 1/deg * sum_{b,i,o} |att h basis g| -- the standard bound for three nested fp32
            chains, the reciprocal and the final multiply; it holds for any summation order;
  tau_own = gamma_(d_out + d_in + 2) * sum_{i,o} |h root g|, the same bound for the root chain (two nested sums);
  1. every listed entry is an in-edge of the node at a distinct CSR position, and src and rel are that edge's (the j-th
     listed entry with one (src, rel) is the j-th position of that pair: duplicate edges are adjacent and tie);
  2. each listed value is within tau_e of the fp64 value;
  3. the list is ordered: value descending, ties by ascending position;
  4. no unlisted edge has an fp64 value above the k-th listed fp64 value plus the two edges' tau;
  5. padding (-inf, -1, -1) fills exactly the slots beyond deg;
  and |own - own64| <= tau_own + u |own64|,  |total - sum c64| <= sum tau_e + u |sum c64|.
A node outside [0, n): a fully padded row with NaN own and total.  The rule skips nothing.
"""
import torch

U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


def _cpu64(*ts):
    return tuple(t.detach().double().cpu() for t in ts)


def edge_values64(h64, basis64, att64, root64, in_edges, node, g64):
    """All in-edges of `node` in segment order -> dict(src, rel int64 [deg]; c, tau float64 [deg]; own, tau_own floats)."""
    in_ptr, in_src, in_rel = in_edges
    e0, e1 = int(in_ptr[node]), int(in_ptr[node + 1])
    deg = e1 - e0
    src, rel = in_src[e0:e1].long().cpu(), in_rel[e0:e1].long().cpu()
    n_bases, d_in, d_out = basis64.shape
    G = basis64 @ g64                                                    # [B, d_in]
    Ga = basis64.abs() @ g64.abs()
    c = (att64[rel] * (h64[src] @ G.t())).sum(1) / max(deg, 1)
    ca = (att64[rel].abs() * (h64[src].abs() @ Ga.t())).sum(1) / max(deg, 1)
    own = float(h64[node] @ (root64 @ g64))
    own_abs = float(h64[node].abs() @ (root64.abs() @ g64.abs()))
    return {'src': src, 'rel': rel, 'c': c, 'tau': gamma(d_out + d_in + n_bases + 2) * ca, 'own': own,
            'tau_own': gamma(d_out + d_in + 2) * own_abs}


def spec_attribution(h, basis, att, root, in_edges, q_node, probe, k):
    """The exact fp64 attribution -> (contrib float64 [Q, k], src int64 [Q, k], rel int64 [Q, k], own float64 [Q], total
    float64 [Q], pos int64 [Q, k]: the listed edges' positions in their segments); padding (-inf, -1, -1, pos -1); a node
    out of range: padding and NaN."""
    h64, basis64, att64, root64, p64 = _cpu64(h, basis, att, root, probe)
    in_edges = tuple(t.cpu() for t in in_edges)
    nodes = [int(x) for x in torch.as_tensor(q_node).tolist()]
    n, Q = h64.shape[0], len(nodes)
    out_c = torch.full((Q, k), float('-inf'), dtype=torch.float64)
    out_s, out_r, out_p = (torch.full((Q, k), -1, dtype=torch.int64) for _ in range(3))
    own = torch.full((Q,), float('nan'), dtype=torch.float64)
    total = torch.full((Q,), float('nan'), dtype=torch.float64)
    for i, v in enumerate(nodes):
        if v < 0 or v >= n:
            continue
        e = edge_values64(h64, basis64, att64, root64, in_edges, v, p64[i])
        own[i], total[i] = e['own'], float(e['c'].sum())
        order = sorted((j for j in range(e['c'].numel()) if e['c'][j] == e['c'][j]), key=lambda j: (-float(e['c'][j]), j))[:k]
        for slot, j in enumerate(order):
            out_c[i, slot], out_s[i, slot], out_r[i, slot], out_p[i, slot] = e['c'][j], e['src'][j], e['rel'][j], j
    return out_c, out_s, out_r, own, total, out_p


def check_attribution(h, basis, att, root, in_edges, q_node, probe, k, got, what=''):
    """Assert the acceptance rule for got = (contrib [Q, k], src [Q, k], rel [Q, k], own [Q], total [Q]) (any device).
    -> dict of float64 [Q] tensors: 'own64', 'total64', 'tau_own', 'tau_sum' (NaN / 0 for a node out of range), and the
    largest shares of tau the listed values, own and total used ('used_edge', 'used_own', 'used_total')."""
    h64, basis64, att64, root64, p64 = _cpu64(h, basis, att, root, probe)
    in_edges = tuple(t.cpu() for t in in_edges)
    nodes = [int(x) for x in torch.as_tensor(q_node).tolist()]
    n, Q = h64.shape[0], len(nodes)
    c_all, s_all, r_all, own_all, tot_all = (t.detach().cpu() for t in got)
    assert c_all.shape == (Q, k) and s_all.shape == (Q, k) and r_all.shape == (Q, k), (what, 'list shapes')
    assert own_all.shape == (Q,) and tot_all.shape == (Q,), (what, 'own / total shapes')
    res = {key: torch.zeros(Q, dtype=torch.float64) for key in ('own64', 'total64', 'tau_own', 'tau_sum')}
    used = {'used_edge': 0.0, 'used_own': 0.0, 'used_total': 0.0}
    for i, v in enumerate(nodes):
        tag = (what, 'query %d node %d' % (i, v))
        cv, sv, rv = c_all[i].double(), s_all[i].long(), r_all[i].long()
        if v < 0 or v >= n:
            assert bool(torch.isneginf(cv).all()) and bool((sv == -1).all()) and bool((rv == -1).all()), (tag, 'padded row')
            assert own_all[i] != own_all[i] and tot_all[i] != tot_all[i], (tag, 'NaN own and total')
            res['own64'][i] = res['total64'][i] = float('nan')
            continue
        e = edge_values64(h64, basis64, att64, root64, in_edges, v, p64[i])
        c64, tau, deg = e['c'], e['tau'], e['c'].numel()
        # 5. padding fills exactly the slots beyond deg
        nv = int((sv >= 0).sum())
        assert nv == min(k, deg), (tag, 'listed %d of %d edges (k = %d)' % (nv, deg, k))
        assert bool((sv[:nv] >= 0).all()) and bool((sv[nv:] == -1).all()) and bool((rv[nv:] == -1).all()), (tag, 'padding')
        assert bool(torch.isneginf(cv[nv:]).all()), (tag, 'padding value')
        # 1. in-edges of the node at distinct positions
        where = {}
        for j, key in enumerate(zip(e['src'].tolist(), e['rel'].tolist())):
            where.setdefault(key, []).append(j)
        taken, pos = {}, []
        for key in zip(sv[:nv].tolist(), rv[:nv].tolist()):
            j = taken.get(key, 0)
            assert key in where and j < len(where[key]), (tag, 'not an in-edge of the node, or listed too often', key)
            pos.append(where[key][j])
            taken[key] = j + 1
        pos = torch.tensor(pos, dtype=torch.int64)
        # 2. values
        err = (cv[:nv] - c64[pos]).abs()
        assert bool((err <= tau[pos]).all()), (tag, 'value off fp64', float(err.max()))
        if nv:
            used['used_edge'] = max(used['used_edge'], float((err / tau[pos].clamp(min=1e-300)).max()))
        # 3. order
        if nv > 1:
            lv = c_all[i][:nv]
            ok = (lv[:-1] > lv[1:]) | ((lv[:-1] == lv[1:]) & (pos[:-1] < pos[1:]))
            assert bool(ok.all()), (tag, 'order')
        # 4. completeness
        if nv == k and deg > k:
            missing = torch.ones(deg, dtype=torch.bool)
            missing[pos] = False
            bound = float(c64[pos[-1]] + tau[pos[-1]])
            worst = float((c64 - tau)[missing].max())
            assert worst <= bound, (tag, 'a larger contribution is missing', worst, bound)
        # own and total
        own64, tot64, tau_sum = e['own'], float(c64.sum()), float(tau.sum())
        d_own, d_tot = abs(float(own_all[i]) - own64), abs(float(tot_all[i]) - tot64)
        assert d_own <= e['tau_own'] + U * abs(own64), (tag, 'own off fp64', d_own, e['tau_own'])
        assert d_tot <= tau_sum + U * abs(tot64), (tag, 'total off fp64', d_tot, tau_sum)
        used['used_own'] = max(used['used_own'], d_own / max(e['tau_own'] + U * abs(own64), 1e-300))
        used['used_total'] = max(used['used_total'], d_tot / max(tau_sum + U * abs(tot64), 1e-300))
        res['own64'][i], res['total64'][i], res['tau_own'][i], res['tau_sum'][i] = own64, tot64, e['tau_own'], tau_sum
    res.update(used)
    return res


def rgcn_layer64(h, basis, att, root, edge_index, rel):
    """z of the bias-free layer in fp64, straight from the definition (mean over ALL in-edges, source_to_target)."""
    h64, basis64, att64, root64 = _cpu64(h, basis, att, root)
    src, dst, rel = edge_index[0].long().cpu(), edge_index[1].long().cpu(), torch.as_tensor(rel).long().cpu()
    n = h64.shape[0]
    W = torch.einsum('rb,bio->rio', att64, basis64)
    msg = torch.einsum('ei,eio->eo', h64[src], W[rel])
    deg = torch.bincount(dst, minlength=n).clamp(min=1).double()
    return torch.zeros(n, basis64.shape[2], dtype=torch.float64).index_add_(0, dst, msg) / deg[:, None] + h64 @ root64
