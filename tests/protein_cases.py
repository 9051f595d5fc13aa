"""Cases for the protein stage (everything that produces x0, the input of the D-D layers: GCNConv x 2, MyHierarchyConv, the drug
mix, and the dispatcher `FMEncoder.mixed_drug_features`): P-P and P -> D graphs with deliberate edge cases, a plain fp64
restatement of the stage under torch autograd, the same formula over absolute values (the magnitude every tolerance is a multiple
of) and deterministic parameters that keep the one ReLU of the stage clear of its kink.  No GPU, no fixtures:
`tests/test_host_protein_cases.py` checks on the CPU that the cases hold what they promise, `tests/test_gpu_protein_routes.py`
runs the routes and the C handles on them.

Tolerance of every comparison: |got - want| <= k * 2^-24 * A elementwise, k per tensor.  A is the formula evaluated on |inputs|, |weights| and
the (positive) edge weights, with the fp64 reference's ReLU mask; k is the length of the longest chain of fp32 roundings that
feeds the tensor (`chain_lengths`), computed from the case.
"""
import ctypes

import torch

from oracle import tip_oracle as O
from tip_amd.plan import ITEM_LEADER

U24 = 2.0 ** -24
CHUNK = 16                       # edges per work item the layers are given: a hub row of > CHUNK edges is cut into pieces
VARIANTS = ('pruned', 'all_sources', 'drug_source', 'no_pd_edges_to_targets')
HUB, BIG_SRC, QUIET_SRC = 1, 2, 4          # proteins: P-P hub | source of > max_edges P -> D edges | source of the ignored edge only
RUN_START = 40                             # first protein of the run of consecutive kept source rows
MARGIN = 100.0                             # ReLU margin: no pre-activation within MARGIN x its tolerance of zero

# (n_prot, n_drug, seed) the tests use; every variant of each is checked on the host
SIZES = [(389, 41, 11), (700, 130, 12)]


def pd_limits():
    """(max_rows, max_edges) of a row workgroup of tipk_pd_stage_bwd, from the library (a host query: no GPU)."""
    from tip_amd import _lib
    mr, me = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().tipk_pd_stage_bwd_limits(ctypes.byref(mr), ctypes.byref(me))
    return mr.value, me.value


def isolated_proteins(n_prot):
    """Proteins without any P-P edge (not even a self-loop): 6, 19, 32, ... and the last one."""
    return sorted(set(range(6, n_prot, 13)) | {n_prot - 1})


# ------------------------------------------------------------------------------------------------ graphs
def protein_graph(n_prot, n_drug, seed, variant='pruned', limits=None):
    """-> (pp_edge_index [2, E], pd_edge_index [2, E'] in the concatenated node space (drug j = node n_prot + j), d_norm
    [n_drug]).  What every graph holds is listed in, and asserted by, `check_protein_graph`."""
    assert variant in VARIANTS and n_prot >= 300 and 40 <= n_drug
    max_rows, max_edges = limits or pd_limits()
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g)
    iso = isolated_proteins(n_prot)
    live = torch.tensor([v for v in range(n_prot) if v not in set(iso)])
    pick = lambda n: live[ri(0, live.numel(), n)]
    # ---- P-P: a symmetric base with a hub, duplicates (both directions), self-loops (one twice), 5 edges without a mirror
    a, b = pick(3 * n_prot), pick(3 * n_prot)
    off = (a != b) & (a != HUB) & (b != HUB)
    a, b = a[off], b[off]
    nb = pick(3 * CHUNK + 5)
    nb = nb[nb != HUB]
    a, b = torch.cat([a, nb]), torch.cat([b, torch.full_like(nb, HUB)])
    a, b = torch.cat([a, a[:20]]), torch.cat([b, b[:20]])
    src, dst = torch.cat([a, b]), torch.cat([b, a])
    have = set(zip(src.tolist(), dst.tolist()))
    du, dv = [], []
    while len(du) < 5:
        u, v = int(pick(1)), int(pick(1))
        if u != v and (u, v) not in have and (v, u) not in have:
            have.add((u, v))
            du.append(u)
            dv.append(v)
    loops = live[:: max(1, live.numel() // 8)][:8]
    src = torch.cat([src, torch.tensor(du), loops, loops[:1]])
    dst = torch.cat([dst, torch.tensor(dv), loops, loops[:1]])
    p = torch.randperm(src.numel(), generator=g)
    pp = torch.stack([src[p], dst[p]])
    # ---- P -> D
    d_norm = torch.rand(n_drug, generator=g) * 2 + 0.5
    if variant == 'no_pd_edges_to_targets':
        pd = torch.stack([ri(0, n_prot, 50), ri(0, n_prot, 50)])              # every edge ends at a protein row: ignored
        return pp, pd, d_norm
    run = list(range(RUN_START, RUN_START + max_rows + 6))
    special = {0, HUB, BIG_SRC, iso[0]} | set(run)
    pool = torch.tensor([v for v in range(5, n_prot - 1) if v not in special and v % 3 != 2])     # random sources
    rnd = lambda n: pool[ri(0, pool.numel(), n)]
    rest = list(range(7, n_drug - 1))                                         # drugs 6 and n_drug - 1: no targets
    per_drug = {0: torch.cat([torch.full((max_edges + 8,), BIG_SRC), rnd(300)]),          # > 512 edges, most from ONE source
                1: torch.cat([torch.tensor([iso[0]]), rnd(64)]),                           # 65
                2: torch.cat([torch.tensor([HUB]), rnd(199)]),                             # 200
                3: None, 4: rnd(64), 5: torch.tensor([0])}                                 # 512 | exactly 64 | exactly 1
    first = rnd(502)
    per_drug[3] = torch.cat([first, first[:10]])                              # duplicate (protein, drug) edges
    for j in rest:
        per_drug[j] = rnd(int(ri(2, 12, 1)))
    for i, v in enumerate(run):                                               # one edge each: > max_rows rows, few edges
        j = rest[i % len(rest)]
        per_drug[j] = torch.cat([per_drug[j], torch.tensor([v])])
    if variant == 'all_sources':
        used = set(torch.cat(list(per_drug.values())).tolist())
        for i, v in enumerate(v for v in range(n_prot) if v not in used):
            j = rest[i % len(rest)]
            per_drug[j] = torch.cat([per_drug[j], torch.tensor([v])])
    s = torch.cat([per_drug[j] for j in sorted(per_drug)])
    d = torch.cat([torch.full((per_drug[j].numel(),), n_prot + j) for j in sorted(per_drug)])
    s, d = torch.cat([s, torch.tensor([QUIET_SRC])]), torch.cat([d, torch.tensor([3])])    # ends at a protein row: ignored
    if variant == 'drug_source':
        s, d = torch.cat([s, torch.tensor([n_prot + 2])]), torch.cat([d, torch.tensor([n_prot + 8])])
    p = torch.randperm(s.numel(), generator=g)
    return pp, torch.stack([s[p], d[p]]), d_norm


def row_pieces(plan, row):
    """Work items the plan cuts output row `row` into (1: not split)."""
    it = plan.items.cpu().long()
    if plan.group_slots:
        lead = ((it[:, 3] & ITEM_LEADER) != 0) & (it[:, 2] == row)
        return int((it[lead, 3] >> 8).max()) if bool(lead.any()) else 1
    sr = plan.split_rows.cpu().long()
    m = sr[:, 0] == row
    return int((sr[m, 2] - sr[m, 1]).max()) if bool(m.any()) else 1


def check_protein_graph(pp, pd, d_norm, n_prot, n_drug, variant, limits=None):
    """Asserts every edge case `protein_graph` promises (a test must not silently lose one)."""
    from tip_amd.layers import deal_rows_by_edges, drug_workgroups, gcn_norm_graph
    max_rows, max_edges = limits or pd_limits()
    src, dst = pp[0], pp[1]
    assert int(pp.min()) >= 0 and int(pp.max()) < n_prot
    touched = set(src.tolist()) | set(dst.tolist())
    iso = [v for v in range(n_prot) if v not in touched]
    assert len(iso) >= 3 and n_prot - 1 in iso, 'isolated proteins'
    loops = (src[src == dst]).tolist()
    assert len(set(loops)) >= 4 and len(loops) > len(set(loops)), 'self-loops, one of them twice'
    key = (src * n_prot + dst)[src != dst]
    mirror = (dst * n_prot + src)[src != dst]
    assert key.unique().numel() < key.numel(), 'duplicate (u, v) edges'
    have = set(key.tolist())
    lone = [k for k in set(mirror.tolist()) if k not in have]
    assert len(lone) == 5 and len(have) > 250, 'five directed edges without a mirror on a symmetric base'
    # the hub row is cut into pieces by the forward plan the layers build with chunk = CHUNK
    graph = gcn_norm_graph(pp, n_prot, CHUNK, d=32)
    assert row_pieces(graph.fwd, HUB) > 1, 'hub row not split'
    assert row_pieces(graph.fwd, iso[0]) == 1
    assert bool((d_norm != 1).all()) and bool((d_norm > 0).all())
    s, d = pd[0], pd[1]
    assert int(pd.min()) >= 0 and int(pd.max()) < n_prot + n_drug
    if variant == 'no_pd_edges_to_targets':
        assert s.numel() > 0 and bool((d < n_prot).all())
        return
    assert int((d < n_prot).sum()) == 1, 'one edge ends at a protein row'
    assert int((s >= n_prot).sum()) == (1 if variant == 'drug_source' else 0)
    tgt = d >= n_prot
    cnt = torch.bincount(d[tgt] - n_prot, minlength=n_drug)
    assert int((cnt == 0).sum()) >= 2 and int(cnt[n_drug - 1]) == 0, 'drugs without targets'
    assert int((cnt > 512).sum()) == 1 and int(((cnt > 64) & (cnt <= 512)).sum()) >= 3
    assert bool((cnt == 1).any()) and bool((cnt == 64).any()) and bool((cnt == 512).any()) and bool((cnt == 65).any())
    _, wgs = drug_workgroups(cnt)
    widths = sorted(set(w[1] >> 8 for w in wgs))
    assert widths == [1, 4, 16], widths
    k = s[tgt] * (n_prot + n_drug) + d[tgt]
    assert k.unique().numel() < k.numel(), 'duplicate P -> D edges'
    prot = tgt & (s < n_prot)
    out_deg = torch.bincount(s[prot], minlength=n_prot)
    assert int(out_deg.max()) > max_edges and int(out_deg[BIG_SRC]) > max_edges, 'a source with more edges than max_edges'
    sources = torch.unique(s[s < n_prot])
    if variant == 'all_sources':
        assert sources.numel() == n_prot
    else:
        assert sources.numel() < n_prot and int(sources[0]) == 0 and n_prot - 1 not in sources.tolist()
    assert iso[0] in sources.tolist(), 'a kept row whose only in-edge is its own loop'
    assert HUB in sources.tolist()
    # a run of more than max_rows consecutive kept rows with at most max_edges edges: the ROW limit cuts it
    kept = torch.zeros(n_prot, dtype=torch.bool)
    kept[sources] = True
    win = range(RUN_START, RUN_START + max_rows + 1)
    assert bool(kept[list(win)].all()) and int(out_deg[list(win)].sum()) <= max_edges
    bounds = deal_rows_by_edges(out_deg[sources].tolist(), max_rows, max_edges)
    sizes = [b1 - b0 for b0, b1 in zip(bounds[:-1], bounds[1:])]
    assert max_rows in sizes, 'no row workgroup filled to max_rows'
    assert any(b1 - b0 == 1 and int(out_deg[sources][b0]) > max_edges for b0, b1 in zip(bounds[:-1], bounds[1:]))


# ------------------------------------------------------------------------------------------------ features and parameters
def sparse_features(n_prot, width, seed):
    """General sparse protein features [n_prot, width] (COO, NOT coalesced: entries in a random order), values != 1 of both signs,
    three per row; the last row is empty.  -> (indices [2, nnz], values [nnz])."""
    g = torch.Generator().manual_seed(seed + 500)
    rows = torch.arange(n_prot - 1).repeat_interleave(3)
    cols = torch.stack([torch.randperm(width, generator=g)[:3] for _ in range(n_prot - 1)]).view(-1)
    vals = (torch.rand(rows.numel(), generator=g) + 0.5) * (torch.randint(0, 2, (rows.numel(),), generator=g) * 2 - 1).float()
    vals[vals == 1] = 1.25
    p = torch.randperm(rows.numel(), generator=g)
    return torch.stack([rows[p], cols[p]]), vals[p]


def features(kind, n_prot, seed, width=24):
    """-> (dense fp32 matrix the reference uses | None for the identity, nonzeros per row that feed one value)."""
    if kind == 'identity':
        return None, 1
    if kind == 'sparse':
        idx, val = sparse_features(n_prot, width, seed)
        return torch.zeros(n_prot, width).index_put_((idx[0], idx[1]), val), 3
    assert kind == 'dense'
    return torch.randn(n_prot, width, generator=torch.Generator().manual_seed(seed + 600)), width


def _agg(t, row, col, w, n):
    return torch.zeros((n, t.shape[1]), dtype=t.dtype).index_add_(0, col, t[row] * w.unsqueeze(1))


def degrees(pp, pd, n_prot, n_drug):
    """Largest degrees of the case: (in, out) of the normalised P-P graph, loop included; (in-degree of a drug, out-degree of a
    source) of the P -> D edges that end at a drug."""
    row, col, _ = O.gcn_norm(pp, n_prot, torch.float64)
    d_pp = (int(torch.bincount(col, minlength=n_prot).max()), int(torch.bincount(row, minlength=n_prot).max()))
    keep = pd[1] >= n_prot
    d_pd = (1, 1)
    if bool(keep.any()):
        d_pd = (int(torch.bincount(pd[1][keep]).max()), int(torch.bincount(pd[0][keep]).max()))
    return d_pp, d_pd


W_ROUNDINGS = 7          # an edge weight of A_hat: deg^-1/2 twice (a square root and a reciprocal, or a pow of <= 1 ulp: 3 each), their product
M_ROUNDINGS = 1          # 1 / count of the mean


def k_pre1(pp, n_prot, in_terms):
    """Roundings into one pre-activation of conv1: in_terms products per table row, the row's in-degree of weighted rows summed,
    the edge weight's own roundings, the bias."""
    row, col, _ = O.gcn_norm(pp, n_prot, torch.float64)
    return int(torch.bincount(col, minlength=n_prot).max()) + in_terms + 1 + W_ROUNDINGS


def chain_lengths(pp, pd, n_prot, n_drug, in_terms, hid1, hid2, pd_dim, n_embed, mod, identity):
    """k of `|got - want| <= k 2^-24 A`, PER TENSOR (x0 under 'cat': per column): the number of fp32 roundings on the longest
    path from an input into one element, followed through the formulas of `stage_forward` and of its gradient.  Along a path
    the counts add: a sum of m terms costs m, a product of two computed values the sum of their counts + 1, a scalar factor its
    own roundings.  Parameters, features, the upstream gradient and the ReLU mask (clear of its kink by MARGIN) are exact."""
    (pp_in, pp_out), (pd_in, pd_out) = degrees(pp, pd, n_prot, n_drug)
    k = {'pre1': k_pre1(pp, n_prot, in_terms)}
    h2 = k['pre1'] + hid1 + pp_in + 1 + W_ROUNDINGS                   # h1 W2^T (hid1 terms), aggregated, + bias
    mean = h2 + pd_in + M_ROUNDINGS
    pdf = mean + hid2                                                 # mean W_h
    xd = 2                                                            # embed / d_norm (a reciprocal and a product at most)
    if mod == 'cat':
        k['x0'] = torch.cat([torch.full((n_embed,), float(xd)), torch.full((pd_dim,), float(pdf))]).double()
    else:
        k['x0'] = pdf + xd + 1
    k['grad.embed'] = xd                                              # upstream / d_norm
    k['grad.hgcn.weight'] = mean + 1 + n_drug                         # mean^T g: computed x exact, summed over the drugs
    g_h2 = pd_dim + pd_out + M_ROUNDINGS                              # g W_h^T, then the transposed P -> D gather
    k['grad.conv2.bias'] = g_h2 + n_prot
    g_xl2 = g_h2 + pp_out + W_ROUNDINGS                               # A_hat^T g_h2
    # g_xl2^T h1, or g_h2^T (A_hat h1) where conv2 aggregates first: two computed values, summed over proteins
    k['grad.conv2.weight'] = g_h2 + max(pp_in, pp_out) + W_ROUNDINGS + k['pre1'] + 1 + n_prot
    g_pre1 = g_xl2 + hid2                                             # g_xl2 W2, masked
    k['grad.conv1.bias'] = g_pre1 + n_prot
    g_xl1 = g_pre1 + pp_out + W_ROUNDINGS
    k['grad.conv1.weight'] = g_xl1 if identity else g_xl1 + n_prot    # identity: d W = (d lin)^T; else g_xl1^T x over proteins
    k['grad.x_prot'] = g_xl1 + hid1
    return k


def gcn_layer_chain(pp, n, in_terms, d_out, identity):
    """k per tensor of ONE GCNConv (`gcn_layer_reference`), either order of aggregation and dense map: out, g_b, g_w, g_x."""
    (pp_in, pp_out), _ = degrees(pp, torch.zeros((2, 0), dtype=torch.long), n, 1)
    g_xl = pp_out + W_ROUNDINGS                                       # A_hat^T g
    return dict(out=pp_in + W_ROUNDINGS + in_terms + 1,               # the aggregation, the dense map's terms, the bias
                g_b=n,                                                # a column sum of the (exactly masked) upstream gradient
                g_w=g_xl if identity else max(pp_in, pp_out) + W_ROUNDINGS + 1 + n,     # (d lin)^T | a sum over the nodes of products
                g_x=g_xl + d_out)


def hier_layer_chain(pd, n_source, n_target, d_in, d_out):
    """k per tensor of MyHierarchyConv (`hier_layer_reference`): out, g_w, g_x."""
    _, (pd_in, pd_out) = degrees(torch.zeros((2, 0), dtype=torch.long), pd, n_source, n_target)
    mean = pd_in + M_ROUNDINGS
    return dict(out=mean + d_in, g_w=mean + 1 + n_target, g_x=d_out + pd_out + M_ROUNDINGS)


def make_params(pp, n_prot, n_drug, x, in_terms, hid1, hid2, pd_dim, n_embed, seed):
    """Deterministic fp32 parameters under the layers' names.  conv1's channels (a row of lin.weight and its bias) are drawn until
    no pre-activation of the channel lies within MARGIN x its tolerance of zero: fp32 rounding cannot flip the ReLU mask, so
    every element of every tensor is compared (nothing is excluded)."""
    g = torch.Generator().manual_seed(seed + 900)
    in_dim = n_prot if x is None else x.shape[1]
    row, col, w = O.gcn_norm(pp, n_prot, torch.float64)
    k1 = k_pre1(pp, n_prot, in_terms)
    x64 = None if x is None else x.double()
    w_rows, b_vals = [], []
    bound = (6.0 / (in_dim + hid1)) ** 0.5 * (3.0 if x is None else 1.0)
    for _ in range(200):
        wc = ((torch.rand(64, in_dim, generator=g) * 2 - 1) * bound)
        bc = torch.randn(64, generator=g) * 0.1
        xl = wc.double().t() if x64 is None else x64 @ wc.double().t()
        xl_abs = wc.double().abs().t() if x64 is None else x64.abs() @ wc.double().abs().t()
        pre = _agg(xl, row, col, w, n_prot) + bc.double()
        mag = _agg(xl_abs, row, col, w, n_prot) + bc.double().abs()
        ok = (pre.abs() > MARGIN * k1 * U24 * mag).all(0)
        for i in torch.nonzero(ok).view(-1).tolist():
            w_rows.append(wc[i])
            b_vals.append(bc[i])
        if len(w_rows) >= hid1:
            break
    assert len(w_rows) >= hid1, 'no conv1 channels clear of the ReLU kink'
    p = {'conv1.weight': torch.stack(w_rows[:hid1]), 'conv1.bias': torch.stack(b_vals[:hid1])}
    p['conv2.weight'] = torch.randn(hid2, hid1, generator=g) / hid1 ** 0.5
    p['conv2.bias'] = torch.randn(hid2, generator=g) * 0.1
    p['hgcn.weight'] = torch.randn(hid2, pd_dim, generator=g) / hid2 ** 0.5
    p['embed'] = torch.randn(n_drug, n_embed, generator=g)
    return p


# ------------------------------------------------------------------------------------------------ reference
def pp_forward(p, pp, n_prot, x, mask=None):
    """PPEncoder in the dtype of `p` (src/layers.py:380-395): h1 = relu(A_hat (x W1^T) + b1); h2 = A_hat (h1 W2^T) + b2.
    x = None: identity features.  mask: h1 = pre1 * mask instead of the ReLU (the absolute-value evaluation).  -> (h2, pre1)"""
    row, col, w = O.gcn_norm(pp, n_prot, p['conv1.weight'].dtype)
    w1, w2 = p['conv1.weight'], p['conv2.weight']
    xl1 = w1.t() if x is None else x @ w1.t()
    pre1 = _agg(xl1, row, col, w, n_prot) + p['conv1.bias']
    h1 = torch.relu(pre1) if mask is None else pre1 * mask
    return _agg(h1 @ w2.t(), row, col, w, n_prot) + p['conv2.bias'], pre1


def stage_forward(p, graphs, n_prot, n_drug, x, mod, mask=None):
    """The stage in the dtype of `p` (src/layers.py:380-395, :196-247, :522-539), differentiable: `pp_forward`, then
    pd = mean over the P -> D edges of cat(h2, 0)[src] . W_h (rows of the drugs), x0 = cat | add of embed / d_norm and pd.
    -> (x0, pre1)"""
    pp, pd, d_norm = graphs
    dt = p['embed'].dtype
    h2, pre1 = pp_forward(p, pp, n_prot, x, mask)
    x_all = torch.cat([h2, torch.zeros((n_drug, h2.shape[1]), dtype=dt)])
    pdf, _ = O.hier_conv_fwd(x_all, pd, p['hgcn.weight'], n_prot)
    xd = p['embed'] / d_norm.to(dt).view(-1, 1)
    return (torch.cat([xd, pdf], 1) if mod == 'cat' else xd + pdf), pre1


GRAD_NAMES = ('embed', 'conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'hgcn.weight')


def _leaves(p, x, dt, absolute=False):
    f = (lambda t: t.detach().to(dt).abs()) if absolute else (lambda t: t.detach().to(dt))
    q = {k: f(v).clone().requires_grad_() for k, v in p.items()}
    xs = None if x is None else f(x).clone().requires_grad_()
    return q, xs


def stage_reference(p, graphs, n_prot, n_drug, x, mod, upstream, dtype=torch.float64):
    """-> {'x0', 'pre1', 'grad.<name>' for GRAD_NAMES, 'grad.x_prot' (dense x)}: the stage and every gradient of
    sum(x0 * upstream), by torch autograd in `dtype` on the CPU (fp64: the reference; fp32: what correct fp32 arithmetic gives)."""
    q, xs = _leaves(p, x, dtype)
    x0, pre1 = stage_forward(q, graphs, n_prot, n_drug, xs, mod)
    x0.backward(upstream.to(dtype))
    out = {'x0': x0.detach(), 'pre1': pre1.detach()}
    for k in GRAD_NAMES:
        out['grad.' + k] = q[k].grad
    if xs is not None:
        out['grad.x_prot'] = xs.grad
    return out


def abs_bound(p, graphs, n_prot, n_drug, x, mod, upstream, pre1_ref):
    """The same formulas on |inputs|, |weights| and the edge weights, with the reference's ReLU mask: per element the sum of the
    absolute values of the terms that `stage_reference` adds.  Keys as `stage_reference`."""
    q, xs = _leaves(p, x, torch.float64, absolute=True)
    mask = (pre1_ref > 0).double()
    x0, pre1 = stage_forward(q, graphs, n_prot, n_drug, xs, mod, mask=mask)
    (x0 * upstream.double().abs()).sum().backward()
    out = {'x0': x0.detach(), 'pre1': pre1.detach()}
    for k in GRAD_NAMES:
        out['grad.' + k] = q[k].grad
    if xs is not None:
        out['grad.x_prot'] = xs.grad
    return out


def worst_ratio(got, want, mag, k=1.0):
    """max |got - want| / (k 2^-24 A) over the elements (k: a number or one value per column); an element with A = 0 must be
    matched exactly (inf otherwise)."""
    got, want = got.detach().to('cpu', torch.float64), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), 'non-finite values'
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    ratio = torch.where(mag > 0, err / (U24 * mag.clamp(min=1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float((ratio / k).max())


class StageCase(object):
    """One (sizes, variant, feature kind, widths, mod): graphs, features, parameters, the fp64 reference, A and k."""

    def __init__(self, n_prot, n_drug, seed, variant, feat='identity', mod='cat', hid1=32, hid2=16, pd_dim=16, n_embed=48, limits=None):
        if mod == 'add':
            n_embed = pd_dim
        self.n_prot, self.n_drug, self.seed, self.variant, self.feat, self.mod = n_prot, n_drug, seed, variant, feat, mod
        self.hid1, self.hid2, self.pd_dim, self.n_embed = hid1, hid2, pd_dim, n_embed
        self.graphs = protein_graph(n_prot, n_drug, seed, variant, limits)
        self.x, self.in_terms = features(feat, n_prot, seed)
        pp, pd, _ = self.graphs
        self.params = make_params(pp, n_prot, n_drug, self.x, self.in_terms, hid1, hid2, pd_dim, n_embed, seed)
        self.d0 = n_embed + pd_dim if mod == 'cat' else n_embed
        self.upstream = torch.randn(n_drug, self.d0, generator=torch.Generator().manual_seed(seed + 700))
        self.k = chain_lengths(pp, pd, n_prot, n_drug, self.in_terms, hid1, hid2, pd_dim, n_embed, mod, self.x is None)
        self._ref = self._mag = None

    def ref(self):
        if self._ref is None:
            self._ref = stage_reference(self.params, self.graphs, self.n_prot, self.n_drug, self.x, self.mod, self.upstream)
        return self._ref

    def mag(self):
        if self._mag is None:
            self._mag = abs_bound(self.params, self.graphs, self.n_prot, self.n_drug, self.x, self.mod, self.upstream, self.ref()['pre1'])
        return self._mag

    def cpu32(self):
        return stage_reference(self.params, self.graphs, self.n_prot, self.n_drug, self.x, self.mod, self.upstream, torch.float32)

    def k_of(self, name):
        """k of tensor `name`: a number, or one value per column (x0 under 'cat')."""
        return self.k[name]

    def relu_margin(self):
        """min |pre1| / (k 2^-24 A) over conv1's pre-activations: > MARGIN means no ReLU mask can flip within the tolerance."""
        return float((self.ref()['pre1'].abs() / (self.k['pre1'] * U24 * self.mag()['pre1'])).min())


# ------------------------------------------------------------------------------------------------ one layer (the C handles)
def gcn_layer_reference(pp, n, x, weight, bias, relu, upstream, absolute=False, mask=None):
    """One GCNConv in fp64: out = relu?(A_hat (x W^T) + b) and the gradients of sum(out * upstream).  x = None: identity.
    absolute: the magnitudes (|.| of everything, `mask` = the reference's ReLU mask).  -> dict out, pre, g_x, g_w, g_b"""
    f = (lambda t: t.detach().double().abs()) if absolute else (lambda t: t.detach().double())
    row, col, w = O.gcn_norm(pp, n, torch.float64)
    wt = f(weight).clone().requires_grad_()
    b = None if bias is None else f(bias).clone().requires_grad_()
    xs = None if x is None else f(x).clone().requires_grad_()
    pre = _agg(wt.t() if xs is None else xs @ wt.t(), row, col, w, n)
    if b is not None:
        pre = pre + b
    if absolute:
        out = pre * mask if relu else pre
    else:
        out = torch.relu(pre) if relu else pre
    (out * f(upstream)).sum().backward()
    return dict(out=out.detach(), pre=pre.detach(), g_x=None if xs is None else xs.grad, g_w=wt.grad, g_b=None if b is None else b.grad)


def hier_layer_reference(pd, n_all, n_source, x_all, weight, upstream, absolute=False):
    """MyHierarchyConv in fp64 (oracle.hier_conv_fwd under autograd): out [n_all - n_source, d_out], g_x [n_all, d_in], g_w."""
    f = (lambda t: t.detach().double().abs()) if absolute else (lambda t: t.detach().double())
    xs, wt = f(x_all).clone().requires_grad_(), f(weight).clone().requires_grad_()
    out, _ = O.hier_conv_fwd(xs, pd, wt, n_source)
    (out * f(upstream)).sum().backward()
    return dict(out=out.detach(), g_x=xs.grad, g_w=wt.grad)


# ------------------------------------------------------------------------------------------------ the routes of the dispatcher
# id -> size (index into SIZES), variant, protein features, mod, (hid1, hid2) of the P-P encoder (hid2 = the hierarchy conv's input
# width), TIPK_NO_ENCODER_STEP, prune_pp_rows, the route `FMEncoder.mixed_drug_features` must take
ROUTE_CASES = {
    'A_cat_identity': (1, 'pruned', 'identity', 'cat', (32, 16), False, True, 'pd_stage'),
    'A_add_identity': (0, 'pruned', 'identity', 'add', (32, 16), False, True, 'pd_stage'),
    'A_cat_dense': (0, 'pruned', 'dense', 'cat', (32, 16), False, True, 'pd_stage'),
    'B_cat_identity': (0, 'pruned', 'identity', 'cat', (32, 16), True, True, 'agg_first_link'),
    'B_add_dense': (0, 'pruned', 'dense', 'add', (32, 16), True, True, 'agg_first_link'),
    'C_24_12_identity': (0, 'pruned', 'identity', 'cat', (24, 12), False, True, 'transform_first_rows'),
    'C_24_12_dense': (0, 'pruned', 'dense', 'add', (24, 12), False, True, 'transform_first_rows'),
    'C_sparse': (0, 'pruned', 'sparse', 'cat', (32, 16), False, True, 'sparse_rows'),
    'D_prune_off': (0, 'pruned', 'identity', 'cat', (32, 16), False, False, 'unpruned'),
    'D_all_sources': (1, 'all_sources', 'dense', 'cat', (32, 16), False, True, 'unpruned'),
    'E_width7_cat': (0, 'pruned', 'identity', 'cat', (32, 7), False, True, 'mean_mm_fused'),
    'E_width7_add': (0, 'pruned', 'dense', 'add', (32, 7), False, True, 'mean_mm_fused'),
    'E_width72_cat': (0, 'pruned', 'sparse', 'cat', (32, 72), False, True, 'mean_mm_unfused'),
    'E_width72_add': (0, 'all_sources', 'identity', 'add', (32, 72), False, True, 'mean_mm_unfused'),
    'F_drug_source': (0, 'drug_source', 'identity', 'cat', (32, 16), False, True, 'concat'),
    'F_drug_source_add': (0, 'drug_source', 'dense', 'add', (32, 16), False, True, 'concat'),
}
_CASES = {}


def route_case(cid, limits=None):
    """The StageCase of a ROUTE_CASES row (built once per process: the fp64 reference is shared and never modified)."""
    if cid not in _CASES:
        size, variant, feat, mod, (hid1, hid2), _, _, _ = ROUTE_CASES[cid]
        n_prot, n_drug, seed = SIZES[size]
        _CASES[cid] = StageCase(n_prot, n_drug, seed, variant, feat, mod, hid1, hid2, limits=limits)
    return _CASES[cid]
