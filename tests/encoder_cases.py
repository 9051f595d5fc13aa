"""Cases for the WHOLE encoder step (tip_amd/encoder.py `_EncoderStep`, include/tipk.h section 10d): the table CASES, the fp64
reference, the magnitude A and chain length k of every compared tensor, parameters that keep both ReLUs clear of their kink, and
the graph edits (`probes`) that show the bound is tight enough to see one dropped, doubled or misfiled edge.  No GPU, no
fixtures: `tests/test_host_encoder_cases.py` checks on the CPU that the cases hold what they promise,
`tests/test_gpu_encoder_step_edges.py` runs the step and the C handle on them.

Nothing is restated: the P-P and P -> D graphs, conv1's parameters, the stage's chain lengths and `worst_ratio` are
`protein_cases`'; the D-D graphs are `route_harness.small_graph`'s; the reference is `oracle.tip_oracle.fm_encoder_fwd` / `_bwd`
in float64 (float32: what correct fp32 arithmetic gives).

Tolerance of every comparison, z and the twelve gradients: |got - want| <= k 2^-24 A elementwise.  A is the encoder's formula
evaluated on |parameters| with the fp64 reference's two ReLU masks (autograd over `protein_cases.stage_forward` and
`oracle.rgcn_fwd`); k is the number of fp32 roundings on the longest path into an element (`chain_lengths`), computed from the
case.  No tolerance is chosen by hand.
"""
import torch

import protein_cases as P
from oracle import tip_oracle as O
from route_harness import _finish, check_small_graph, small_graph

U24 = P.U24
NB, HID1, PP_HID1, PP_HID2 = 32, 32, 32, 16        # the only widths the fused kernels take: 32 bases, n_hid1 32, PPEncoder 32 -> 16
SPLIT1 = ('split_last', 1)                          # the largest R whose [R, 32] att table stays in ONE LDS column block
SPLIT2 = ('split_first', 2)                         # one relation more
DOMINANT = 8.0                                      # |dominant term of a1| / RMS(rest of a1), at most
PROBE_FACTOR = 10.0                                 # a probe moves some element by at least this many bounds
DD_KINDS = ('dir', 'sym', 'near', 'dense', 'one_edge', 'tiny')
PROT_VARIANTS = P.VARIANTS + ('tiny',)
FUSED_IDS = ('cat_sym_41', 'add_dir_130_h32', 'cat_near_41_h32', 'r1', 'split1_last', 'n1024', 'n64', 'dense_41', 'one_edge')
REFUSED_IDS = ('split2_first', 'n1025', 'all_sources', 'drug_source', 'no_pd_edges_to_targets')
PROBE_KINDS = ('rel1_edge', 'dup_triple', 'hub_in_edge', 'pd_single', 'pp_self_loop', 'move_edge')

# id, n_prot, n_drug, seed, protein variant, R, D-D kind, mod ('cat' 48 + 16 | 'add' 64 / 64), n_hid2, what must happen
# ('fused' | 'refused' | 'any': the two decisions must only agree)
CASES = [
    ('cat_sym_41', 389, 41, 11, 'pruned', 40, 'sym', 'cat', 16, 'fused'),
    ('add_dir_130_h32', 700, 130, 12, 'pruned', 33, 'dir', 'add', 32, 'fused'),
    ('cat_near_41_h32', 389, 41, 13, 'pruned', 40, 'near', 'cat', 32, 'fused'),
    ('r1', 389, 50, 14, 'pruned', 1, 'dir', 'cat', 16, 'fused'),
    ('split1_last', 389, 41, 15, 'pruned', SPLIT1, 'sym', 'cat', 16, 'fused'),
    ('n1024', 700, 1024, 16, 'pruned', 20, 'near', 'cat', 16, 'fused'),
    ('n64', 389, 64, 17, 'pruned', 12, 'sym', 'add', 16, 'fused'),
    ('dense_41', 389, 41, 18, 'pruned', 12, 'dense', 'cat', 16, 'fused'),
    ('one_edge', 389, 41, 19, 'pruned', 4, 'one_edge', 'add', 16, 'fused'),
    ('tiny_9', 12, 9, 20, 'tiny', 5, 'tiny', 'cat', 16, 'any'),
    ('split2_first', 389, 41, 15, 'pruned', SPLIT2, 'sym', 'cat', 16, 'refused'),
    ('n1025', 700, 1025, 16, 'pruned', 20, 'near', 'cat', 16, 'refused'),
    ('all_sources', 389, 41, 11, 'all_sources', 40, 'sym', 'cat', 16, 'refused'),
    ('drug_source', 389, 41, 11, 'drug_source', 40, 'sym', 'add', 16, 'refused'),
    ('no_pd_edges_to_targets', 389, 41, 11, 'no_pd_edges_to_targets', 40, 'sym', 'cat', 16, 'refused'),
]
CASE_IDS = [c[0] for c in CASES]
FIELDS = ('id', 'n_prot', 'n_drug', 'seed', 'variant', 'R', 'kind', 'mod', 'n_hid2', 'expect')
STATE = ('embed', 'pp_encoder.conv1.lin.weight', 'pp_encoder.conv1.bias', 'pp_encoder.conv2.lin.weight', 'pp_encoder.conv2.bias',
         'hgcn.weight', 'rgcn1.basis', 'rgcn1.att', 'rgcn1.root', 'rgcn2.basis', 'rgcn2.att', 'rgcn2.root')
_STAGE = {'embed': 'embed', 'conv1.weight': 'pp_encoder.conv1.lin.weight', 'conv1.bias': 'pp_encoder.conv1.bias',
          'conv2.weight': 'pp_encoder.conv2.lin.weight', 'conv2.bias': 'pp_encoder.conv2.bias', 'hgcn.weight': 'hgcn.weight'}
TENSORS = ('z',) + tuple('grad.' + s for s in STATE)


def _lib():
    from tip_amd import _lib as L
    return L.lib()


def split_of(r):
    """LDS column blocks the [r, 32] att table needs in the two-layer cell launch (1: the fused step takes it)."""
    return int(_lib().tipk_stream_gather_supported(int(r), NB, 1))


def resolve_r(v):
    """R of a row: an int, or a boundary computed from the library's host predicate (never written down)."""
    if isinstance(v, int):
        return v
    lo, hi = 1, 1 << 20                                                # split_of(r) == 1 for r <= boundary only
    assert split_of(lo) == 1 and split_of(hi) != 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if split_of(mid) == 1 else (lo, mid)
    assert split_of(lo) == 1 and split_of(lo + 1) != 1
    return lo if v == SPLIT1 else lo + 1


def row(cid):
    c = dict(zip(FIELDS, CASES[CASE_IDS.index(cid)]))
    c['R'] = resolve_r(c['R'])
    return c


# ------------------------------------------------------------------------------------------------ graphs
TINY_LONE_DRUG, TINY_BARE_DRUG, TINY_ISOLATED = 1, 8, 11            # one P -> D edge | no targets | protein without P-P edges


def tiny_protein_graph(n_prot, n_drug, seed):
    """12 proteins, 9 drugs (`protein_graph` needs n_drug >= 40): a ring over proteins 0 .. 9 with a chord, one duplicate, one
    directed edge without a mirror, two self-loops (one twice); protein 10 hangs on 0, protein 11 is isolated.  P -> D: drug 0
    has 5 targets, drug 1 exactly one, drug 2 a duplicate edge, drug 8 none; proteins 0 .. 6 are sources; one edge ends at a
    protein row (ignored)."""
    assert (n_prot, n_drug) == (12, 9)
    und = [(i, (i + 1) % 10) for i in range(10)] + [(0, 5), (0, 10), (2, 3)]
    src = [a for a, b in und] + [b for a, b in und] + [4, 7, 7, 3, 3]
    dst = [b for a, b in und] + [a for a, b in und] + [8, 7, 7, 3, 9]
    pp = torch.tensor([src, dst])
    per_drug = {0: [0, 1, 2, 3, 4], 1: [5], 2: [0, 6, 6], 3: [1, 2], 4: [3, 4], 5: [0, 5], 6: [6, 2], 7: [1, 4, 5]}
    s = [v for j in sorted(per_drug) for v in per_drug[j]] + [2]
    d = [n_prot + j for j in sorted(per_drug) for _ in per_drug[j]] + [3]
    g = torch.Generator().manual_seed(seed)
    p = torch.randperm(len(s), generator=g)
    return pp, torch.stack([torch.tensor(s)[p], torch.tensor(d)[p]]), torch.rand(n_drug, generator=g) * 2 + 0.5


def check_tiny_protein_graph(pp, pd, d_norm, n_prot, n_drug):
    src, dst = pp[0], pp[1]
    touched = set(src.tolist()) | set(dst.tolist())
    assert TINY_ISOLATED not in touched and len(touched) == n_prot - 1, 'one isolated protein'
    loops = src[src == dst].tolist()
    assert len(set(loops)) == 2 and len(loops) == 3, 'two self-loops, one of them twice'
    key = (src * n_prot + dst)[src != dst]
    assert key.unique().numel() < key.numel(), 'duplicate (u, v) edges'
    assert len(set((dst * n_prot + src)[src != dst].tolist()) - set(key.tolist())) == 2, 'directed edges without a mirror'
    assert int((pd[1] < n_prot).sum()) == 1 and int(pd[0].max()) < n_prot
    tgt = pd[1] >= n_prot
    cnt = torch.bincount(pd[1][tgt] - n_prot, minlength=n_drug)
    assert int(cnt[TINY_LONE_DRUG]) == 1 and int(cnt[TINY_BARE_DRUG]) == 0 and int((cnt == 1).sum()) == 1
    k = pd[0][tgt] * (n_prot + n_drug) + pd[1][tgt]
    assert k.unique().numel() < k.numel(), 'duplicate P -> D edges'
    assert 0 < torch.unique(pd[0]).numel() < n_prot and bool((d_norm != 1).all()) and bool((d_norm > 0).all())


def dense_graph(N, R, seed):
    """`small_graph(.., 'sym')` (empty first and last relation, the one-edge relation, duplicates, self-loops, isolated nodes)
    plus EVERY ordered pair of the non-isolated drugs in a random used relation, and the hub linked to every one of them in
    EVERY used relation: all link words full, the longest pair_grads chains."""
    ei, rel, _ = small_graph(N, R, seed, 'sym')
    g = torch.Generator().manual_seed(seed + 50)
    m = N - max(1, N // 12) - 1                                        # nodes 0 .. m - 1 and the hub N - 1 are not isolated
    used = torch.arange(2, R - 1)
    iu = torch.triu_indices(m, m, 1)
    pr = used[torch.randint(0, used.numel(), (iu.shape[1],), generator=g)]
    hu = torch.arange(m).repeat_interleave(used.numel())
    hr = used.repeat(m)
    hub = torch.full_like(hu, N - 1)
    src = torch.cat([ei[0], iu[0], iu[1], hu, hub])
    dst = torch.cat([ei[1], iu[1], iu[0], hub, hu])
    return _finish(src, dst, torch.cat([rel, pr, pr, hr, hr]), N, R)


def check_dense_graph(ei, rel, N, R):
    check_small_graph(ei, rel, N, R, 'sym', False)
    m = N - max(1, N // 12) - 1
    live = list(range(m)) + [N - 1]
    have = set((ei[0] * N + ei[1]).tolist())
    assert all(u * N + v in have for u in live for v in live if u != v), 'a pair of non-isolated drugs without a link'
    hub_rel = set(rel[ei[1] == N - 1].tolist())
    assert hub_rel >= set(range(2, R - 1)), 'the hub misses a used relation'
    for u in range(m):
        assert set(rel[(ei[0] == u) & (ei[1] == N - 1)].tolist()) >= set(range(2, R - 1))
    deg = torch.bincount(ei[1], minlength=N)
    assert bool((deg[m:N - 1] == 0).all()), 'isolated nodes'


ONE_EDGE = (2, 7)


def one_edge_graph(N, R):
    """A single directed edge, in relation 1: every other drug has in-degree 0 and takes the 1 / max(deg, 1) path."""
    assert R >= 3 and N > max(ONE_EDGE)
    return _finish(torch.tensor([ONE_EDGE[0]]), torch.tensor([ONE_EDGE[1]]), torch.tensor([1]), N, R)


def check_one_edge_graph(ei, rel, N, R):
    assert ei.shape == (2, 1) and rel.tolist() == [1] and int(ei[0, 0]) != int(ei[1, 0])
    assert int((torch.bincount(ei[1], minlength=N) == 0).sum()) == N - 1


def tiny_dd_graph(N, R):
    """9 drugs, 5 relations, symmetric: relations 0 and 4 empty, relation 1 one self-loop, three pairs in relations 2 and 3 (one
    of them twice), a self-loop, the hub (drug 8) linked to drugs 0 .. 5 in both; drugs 6 and 7 are isolated."""
    assert (N, R) == (9, 5)
    a = [0, 2, 4, 0, 2] + list(range(6)) * 2
    b = [1, 3, 5, 1, 2] + [8] * 12
    r = [2, 3, 2, 2, 3] + [2] * 6 + [3] * 6
    a, b, r = torch.tensor(a + [0]), torch.tensor(b + [0]), torch.tensor(r + [1])
    off = a != b
    return _finish(torch.cat([a, b[off]]), torch.cat([b, a[off]]), torch.cat([r, r[off]]), N, R)


def check_tiny_dd_graph(ei, rel, N, R):
    cnt = torch.bincount(rel, minlength=R)
    assert int(cnt[0]) == 0 and int(cnt[R - 1]) == 0 and int(cnt[1]) == 1
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg[6]) == 0 and int(deg[7]) == 0 and int(deg[N - 1]) >= 2 * int(deg[:N - 1].max()), 'isolated drugs, the hub'
    keys = (rel * N + ei[0]) * N + ei[1]
    assert keys.unique().numel() < keys.numel() and int((ei[0] == ei[1]).sum()) == 2
    assert torch.equal(torch.sort(keys).values, torch.sort((rel * N + ei[1]) * N + ei[0]).values), 'symmetric'


def dd_graph(kind, N, R, seed):
    if kind == 'tiny':
        return tiny_dd_graph(N, R)
    if kind == 'dense':
        return dense_graph(N, R, seed)
    if kind == 'one_edge':
        return one_edge_graph(N, R)
    return small_graph(N, R, seed, kind)


def check_graphs(case):
    """Every edge case the generators promise, for THIS case's graphs (a test must not silently lose one)."""
    d = case.data
    pp, pd, d_norm, ei, rg = d['pp_train_indices'], d['dp_edge_index'], d['d_norm'], d['dd_train_idx'], d['dd_train_range']
    rel = O._relation_of_edges(rg, ei.shape[1])
    if case.variant == 'tiny':
        check_tiny_protein_graph(pp, pd, d_norm, case.n_prot, case.n_drug)
    else:
        P.check_protein_graph(pp, pd, d_norm, case.n_prot, case.n_drug, case.variant)
    if case.kind == 'dense':
        check_dense_graph(ei, rel, case.n_drug, case.R)
    elif case.kind == 'one_edge':
        check_one_edge_graph(ei, rel, case.n_drug, case.R)
    elif case.kind == 'tiny':
        check_tiny_dd_graph(ei, rel, case.n_drug, case.R)
    else:
        check_small_graph(ei, rel, case.n_drug, case.R, case.kind, False)


# ------------------------------------------------------------------------------------------------ chain lengths
def dd_stats(ei, rg, N):
    """What the D-D chain lengths depend on: edges per ordered pair (relations per pair cell), distinct in- and out-neighbours
    of a node, edges of a relation -- the largest of each."""
    src, dst = ei[0], ei[1]
    pair, per_pair = torch.unique(src * N + dst, return_counts=True)
    din = torch.bincount(pair % N, minlength=N)
    dout = torch.bincount(pair // N, minlength=N)
    e_rel = (rg[:, 1] - rg[:, 0])
    return dict(cell=int(per_pair.max()), din=max(1, int(din.max())), dout=max(1, int(dout.max())), e_rel=max(1, int(e_rel.max())))


def rgcn_chain(k_x, k_g, d_in, d_out, n, st):
    """k per tensor of one R-GCN layer on the pair form, forward and backward, for an input of chain length k_x and an upstream
    gradient of chain length k_g (counts add along a path: a sum of m terms costs m, a product of two computed values the sum
    of their counts + 1; `protein_cases.chain_lengths`).

        XB_b = x basis_b                                       d_in products
        cell(u, v) = sum of att_r over the relations of u -> v  relations per pair cell
        agg(v) = sum_u sum_b cell(u, v)_b XB_b(u)              ONE flat sum over 32 bases x the in-neighbours (pair product + slab sum:
                                                               no order is assumed, so the count is that of the terms)
        out = agg / deg + x root                               1 / deg and its product; d_in products; the sum of the two
        g' = g / deg;  dXB_b(u) = sum_v cell(u, v)_b g'(v)     out-neighbours
        d basis_b = x^T dXB_b,  d root = x^T g                 sums over the N nodes of products of two computed values
        d x = sum_b dXB_b basis_b^T + g root^T                 one flat sum over 32 x d_out (+ d_out) terms
        d att_r = sum over r's edges u -> v of <g'(v), XB_b(u)>  d_out products of two computed values, then the relation's edges"""
    k_xb = k_x + d_in
    k_agg = k_xb + st['cell'] + 1 + NB * st['din']
    k_g1 = k_g + 2
    k_dxb = k_g1 + st['cell'] + 1 + st['dout']
    return dict(out=max(k_agg + 2, k_x + d_in) + 1, basis=k_x + k_dxb + 1 + n, root=k_x + k_g + 1 + n,
                att=k_g1 + k_xb + 1 + d_out + st['e_rel'], x=max(k_dxb + NB * d_out, k_g + d_out) + 1)


def chain_lengths(data, mod, n_embed, pd_dim, n_hid2):
    """k of every compared tensor: `protein_cases.chain_lengths` for the stage that produces x0, `rgcn_chain` through the two
    D-D layers forward, back through them, and the stage's own gradient chains on top of d x0's.  The upstream gradient, the
    parameters and both ReLU masks (clear of their kink by MARGIN) are exact."""
    n_prot, n_drug = data['n_prot'], data['n_drug']
    st = dd_stats(data['dd_train_idx'], data['dd_train_range'], n_drug)
    ks = P.chain_lengths(data['pp_train_indices'], data['dp_edge_index'], n_prot, n_drug, 1, PP_HID1, PP_HID2, pd_dim, n_embed, mod, True)
    k_x0 = int(torch.as_tensor(ks['x0']).max())
    d_in = n_embed + pd_dim if mod == 'cat' else n_embed
    fwd1 = rgcn_chain(k_x0, 0, d_in, HID1, n_drug, st)
    l2 = rgcn_chain(fwd1['out'], 0, HID1, n_hid2, n_drug, st)           # the upstream gradient of z is exact
    l1 = rgcn_chain(k_x0, l2['x'], d_in, HID1, n_drug, st)              # d a1 = d x1 under the exact mask
    k = {'a1': fwd1['out'], 'z': l2['out'], 'pre1': ks['pre1']}
    for name, kk in (('rgcn1', l1), ('rgcn2', l2)):
        for t in ('basis', 'att', 'root'):
            k['grad.%s.%s' % (name, t)] = kk[t]
    for short, full in _STAGE.items():                                  # linear in d x0: its chain is added
        k['grad.' + full] = ks['grad.' + short] + l1['x']
    return k


# ------------------------------------------------------------------------------------------------ parameters
def _mostly_positive(shape, g, flip=8):
    """Uniform in [0.25, 1.25], one value in `flip` negated (0: none).  Sums of such terms hardly cancel, so A stays within a
    small factor of |want| and k 2^-24 A is a RELATIVE bound of about k 2^-24: with zero-mean parameters A is 30 to 100 times
    |want| after two layers, and a bound that wide cannot see one edge of a hub."""
    t = 0.25 + torch.rand(*shape, generator=g)
    if flip:
        t = torch.where(torch.randint(0, flip, shape, generator=g) == 0, -t, t)
    return t


def _signs(n, g):
    """+-1, both values, in a random order."""
    s = torch.ones(n, dtype=torch.float64)
    s[torch.randperm(n, generator=g)[: n // 2]] = -1
    return s


def make_params(data, mod, n_embed, pd_dim, n_hid2, seed):
    """The twelve fp32 parameters under the reference's state_dict names.  conv1: `protein_cases.make_params` (its channels
    are drawn until the first ReLU is clear of its kink).  The second ReLU acts on a1 = rgcn1(x0): redrawing channels cannot
    clear N x 32 values, so the clearance is CONSTRUCTED -- column 0 of x0 is a per-node sign (embed's column 0 is set so that
    embed / d_norm (+ the P -> D part under 'add') gives +-1), row 0 of root1 a per-channel sign times a constant, and
    basis1[:, 0, :] is small, so that sign(a1[v, c]) is decided by x0[v, 0] root1[0, c].  The constant is DOMINANT x the RMS
    of everything else in a1: large enough to decide the sign, small enough that the rest still shows in every comparison."""
    n_prot, n_drug, R = data['n_prot'], data['n_drug'], data['dd_train_range'].shape[0]
    graphs = (data['pp_train_indices'], data['dp_edge_index'], data['d_norm'])
    sp = P.make_params(graphs[0], n_prot, n_drug, None, 1, PP_HID1, PP_HID2, pd_dim, n_embed, seed)
    g = torch.Generator().manual_seed(seed + 1300)
    d_in = n_embed + pd_dim if mod == 'cat' else n_embed
    p = {full: sp[short] for short, full in _STAGE.items()}
    p['rgcn1.basis'] = _mostly_positive((NB, d_in, HID1), g) / d_in
    p['rgcn1.att'] = _mostly_positive((R, NB), g, flip=0) / NB
    p['rgcn1.root'] = _mostly_positive((d_in, HID1), g) / d_in
    p['rgcn2.basis'] = _mostly_positive((NB, HID1, n_hid2), g) / HID1
    p['rgcn2.att'] = _mostly_positive((R, NB), g, flip=0) / NB
    p['rgcn2.root'] = _mostly_positive((HID1, n_hid2), g) / HID1
    p['rgcn1.basis'][:, 0, :] *= 1.0 / 32
    node_scale = 2.0 ** (torch.rand(n_drug, generator=g) * 3 - 1.5)          # rows of x0 differ by up to 8 x: an edge's source shows
    p['embed'] = _mostly_positive((n_drug, n_embed), g, flip=0) * (node_scale * data['d_norm']).view(-1, 1)
    s_node, s_chan = _signs(n_drug, g), _signs(HID1, g)
    # column 0 of x0 = +-1: solve for embed's column 0 in fp64 (its fp32 rounding moves x0 by 2 ulp at most)
    q = {short: p[full].double().clone() for short, full in _STAGE.items()}
    q['embed'][:, 0] = 0
    x0, _ = P.stage_forward(q, graphs, n_prot, n_drug, None, mod)
    col0 = (s_node - x0[:, 0]) * data['d_norm'].double()
    p['embed'][:, 0] = col0.float()
    q['embed'][:, 0] = p['embed'][:, 0].double()
    x0, _ = P.stage_forward(q, graphs, n_prot, n_drug, None, mod)
    root = p['rgcn1.root'].double().clone()
    root[0] = 0
    rest, _ = O.rgcn_fwd(x0, data['dd_train_idx'], data['dd_train_range'], p['rgcn1.basis'].double(), p['rgcn1.att'].double(), root)
    const = DOMINANT * float(rest.pow(2).mean().sqrt())
    p['rgcn1.root'][0] = (s_chan * const).float()
    return p


# ------------------------------------------------------------------------------------------------ reference and magnitude
def reference(p, data, mod, upstream, dtype=torch.float64):
    """-> {'z', 'grad.<state_dict name>' x 12, 'a1', 'h1'}: `oracle.fm_encoder_fwd` / `fm_encoder_bwd` on the CPU in `dtype`."""
    q = {k: v.to(dtype) for k, v in p.items()}
    z, saved = O.fm_encoder_fwd(q, data, mod)
    grads = O.fm_encoder_bwd(upstream.to(dtype), q, data, saved, mod)
    a1, _ = O.rgcn_fwd(saved['x0'], data['dd_train_idx'], data['dd_train_range'], q['rgcn1.basis'], q['rgcn1.att'], q['rgcn1.root'])
    out = {'z': z, 'a1': a1, 'h1': saved['pp'][3]}
    for s in STATE:
        out['grad.' + s] = grads[s]
    return out


def composed(q, data, mod, mask1=None, mask2=None):
    """The encoder under autograd from the pieces the bound needs a mask in: `protein_cases.stage_forward`, `oracle.rgcn_fwd`
    twice.  mask1 / mask2 replace the two ReLUs (the absolute-value evaluation).  -> (z, a1, pre1)"""
    stage = {short: q[full] for short, full in _STAGE.items()}
    graphs = (data['pp_train_indices'], data['dp_edge_index'], data['d_norm'])
    x0, pre1 = P.stage_forward(stage, graphs, data['n_prot'], data['n_drug'], None, mod, mask=mask1)
    ei, rg = data['dd_train_idx'], data['dd_train_range']
    a1, _ = O.rgcn_fwd(x0, ei, rg, q['rgcn1.basis'], q['rgcn1.att'], q['rgcn1.root'])
    x1 = torch.relu(a1) if mask2 is None else a1 * mask2
    z, _ = O.rgcn_fwd(x1, ei, rg, q['rgcn2.basis'], q['rgcn2.att'], q['rgcn2.root'])
    return z, a1, pre1


def magnitude(p, data, mod, upstream, ref):
    """A of every compared tensor (and of a1, pre1): the same formulas on |parameters| and |upstream| with the reference's two
    ReLU masks -- per element the sum of the absolute values of the terms the reference adds."""
    q = {k: v.double().abs().clone().requires_grad_() for k, v in p.items()}
    z, a1, pre1 = composed(q, data, mod, (ref['h1'] > 0).double(), (ref['a1'] > 0).double())
    (z * upstream.double().abs()).sum().backward()
    out = {'z': z.detach(), 'a1': a1.detach(), 'pre1': pre1.detach()}
    for s in STATE:
        out['grad.' + s] = q[s].grad
    return out


class EncoderCase(object):
    """One row of CASES: graphs, parameters, upstream gradient, the fp64 reference, A and k (built once, never modified)."""

    def __init__(self, cid, unit_norm=False):
        for k, v in row(cid).items():
            setattr(self, k, v)
        self.n_embed, self.pd_dim = (48, 16) if self.mod == 'cat' else (64, 64)
        if self.variant == 'tiny':
            pp, pd, d_norm = tiny_protein_graph(self.n_prot, self.n_drug, self.seed)
        else:
            pp, pd, d_norm = P.protein_graph(self.n_prot, self.n_drug, self.seed, self.variant)
        if unit_norm:                                                        # what a NULL d_norm means (include/tipk.h section 10d)
            d_norm = torch.ones_like(d_norm)
        ei, _, rg = dd_graph(self.kind, self.n_drug, self.R, self.seed)
        self.data = dict(n_prot=self.n_prot, n_drug=self.n_drug, pp_train_indices=pp, dp_edge_index=pd, d_norm=d_norm,
                         dd_train_idx=ei, dd_train_range=rg)
        self.params = make_params(self.data, self.mod, self.n_embed, self.pd_dim, self.n_hid2, self.seed)
        # the upstream gradient of a row grows with the row's in-degree: the layer divides it by that degree again, so every
        # edge carries a gradient term of the same size (a hub's edges would otherwise carry 1 / deg of it, below any bound)
        deg = torch.bincount(ei[1], minlength=self.n_drug).clamp(min=1).float()
        self.upstream = _mostly_positive((self.n_drug, self.n_hid2), torch.Generator().manual_seed(self.seed + 1700)) * deg.view(-1, 1)
        self.k = chain_lengths(self.data, self.mod, self.n_embed, self.pd_dim, self.n_hid2)
        self._ref = self._mag = None

    def ref(self):
        if self._ref is None:
            self._ref = reference(self.params, self.data, self.mod, self.upstream)
        return self._ref

    def mag(self):
        if self._mag is None:
            self._mag = magnitude(self.params, self.data, self.mod, self.upstream, self.ref())
        return self._mag

    def cpu32(self):
        return reference(self.params, self.data, self.mod, self.upstream, torch.float32)

    def ratio(self, name, got):
        """max |got - want| / (k 2^-24 A) of tensor `name`: <= 1 passes."""
        return P.worst_ratio(got, self.ref()[name], self.mag()[name], self.k[name])

    def relu_margin(self, name):
        """min |pre-activation| / (k 2^-24 A), name 'a1' (rgcn1's output) or 'pre1' (conv1's): > MARGIN means no rounding
        within the tolerance flips the mask."""
        if name == 'pre1':
            stage = {short: self.params[full].double() for short, full in _STAGE.items()}
            pre = P.pp_forward(stage, self.data['pp_train_indices'], self.n_prot, None)[1]
        else:
            pre = self.ref()['a1']
        return float((pre.abs() / (self.k[name] * U24 * self.mag()[name])).min())

    def dominance(self):
        """|x0[v, 0] root1[0, c]| / RMS(a1 without that term): at most DOMINANT (+ rounding)."""
        a1 = self.ref()['a1']
        x0_col = a1.new_ones(self.n_drug)                                # |x0[:, 0]| = 1 by construction
        dom = x0_col.view(-1, 1) * self.params['rgcn1.root'][0].double().abs().view(1, -1)
        sign = torch.sign(a1)
        rest = a1 - sign * dom                                           # the sign of a1 IS the sign of the dominant term
        return float(dom.max() / rest.pow(2).mean().sqrt())


_CASES = {}


def case(cid, unit_norm=False):
    """The EncoderCase of a CASES row (built once per process: the fp64 reference is shared and never modified).  unit_norm: the
    same row with d_norm = 1 and parameters built for it."""
    if (cid, unit_norm) not in _CASES:
        _CASES[cid, unit_norm] = EncoderCase(cid, unit_norm)
    return _CASES[cid, unit_norm]


# ------------------------------------------------------------------------------------------------ sensitivity probes
def _drop_dd(data, e):
    """the data without D-D edge e (the ranges shifted)."""
    ei, rg = data['dd_train_idx'], data['dd_train_range']
    keep = torch.ones(ei.shape[1], dtype=torch.bool)
    keep[e] = False
    rg2 = rg.clone()
    rg2[:, 0] -= (rg[:, 0] > e).long()
    rg2[:, 1] -= (rg[:, 1] > e).long()
    return dict(data, dd_train_idx=ei[:, keep], dd_train_range=rg2)


def _drop_col(data, key, e):
    keep = torch.ones(data[key].shape[1], dtype=torch.bool)
    keep[e] = False
    return dict(data, **{key: data[key][:, keep]})


def probes(c):
    """[(kind, edited data, moves)] -- single-edge edits of the case's graphs that a kernel could get wrong without the route
    tests noticing: a dropped, doubled or misfiled edge.  moves = False only for 'pp_self_loop': GCNConv REPLACES existing
    self-loops by one unit loop per node (`oracle.gcn_norm`, PyG's `gcn_norm`), so dropping one must change nothing at all;
    'pp_edge' (a P-P edge into the P-P hub) is the edit of that graph that must show."""
    d = c.data
    N, n_prot = c.n_drug, c.n_prot
    ei, rg, pp, pd = d['dd_train_idx'], d['dd_train_range'], d['pp_train_indices'], d['dp_edge_index']
    rel = O._relation_of_edges(rg, ei.shape[1])
    out = []
    cnt = rg[:, 1] - rg[:, 0]
    if c.R >= 3 and int(cnt[1]) == 1:
        out.append(('rel1_edge', _drop_dd(d, int(rg[1, 0])), True))
    key = (rel * N + ei[0]) * N + ei[1]
    uniq, n_of = torch.unique(key, return_counts=True)
    if bool((n_of > 1).any()):
        # the duplicate whose destination has the fewest in-edges: its mean moves most
        deg = torch.bincount(ei[1], minlength=N)
        dup = uniq[n_of > 1]
        best = dup[torch.argmin(deg[dup % N])]
        out.append(('dup_triple', _drop_dd(d, int((key == best).nonzero()[0])), True))
    hub = N - 1
    into_hub = (ei[1] == hub).nonzero().view(-1)
    if into_hub.numel() >= 8:
        # the in-edge whose source has the fewest out-edges and whose relation the fewest edges
        dout = torch.bincount(ei[0], minlength=N)
        score = dout[ei[0][into_hub]] * (int(cnt.max()) + 1) + cnt[rel[into_hub]]
        out.append(('hub_in_edge', _drop_dd(d, int(into_hub[torch.argmin(score)])), True))
    tgt = pd[1] >= n_prot
    n_t = torch.bincount(pd[1][tgt] - n_prot, minlength=N)
    lone = (n_t == 1).nonzero().view(-1)
    if lone.numel():
        e = int(((pd[1] == n_prot + int(lone[0]))).nonzero()[0])
        out.append(('pd_single', _drop_col(d, 'dp_edge_index', e), True))
    loops = (pp[0] == pp[1]).nonzero().view(-1)
    if loops.numel():
        out.append(('pp_self_loop', _drop_col(d, 'pp_train_indices', int(loops[0])), False))
    srcs = set(pd[0][tgt].tolist())
    into = [int(e) for e in ((pp[0] != pp[1]) & (pp[1] < n_prot)).nonzero().view(-1) if int(pp[1][e]) in srcs]
    if into:
        indeg = torch.bincount(pp[1], minlength=n_prot)
        e = min(into, key=lambda e: int(indeg[pp[1][e]]))
        out.append(('pp_edge', _drop_col(d, 'pp_train_indices', e), True))
    if c.R >= 3:
        # the last edge of relation r becomes the first of r + 1: only the boundary between the two blocks moves
        cands = [r for r in range(c.R - 1) if int(cnt[r]) >= 1]
        r = min(cands, key=lambda r: (int(cnt[r + 1]) == 0, int(cnt[r]) + int(cnt[r + 1])))     # a used neighbour, few edges
        rg2 = rg.clone()
        rg2[r, 1] -= 1
        rg2[r + 1, 0] -= 1
        out.append(('move_edge', dict(d, dd_train_range=rg2), True))
    return out


def probe_effect(c, data):
    """max over the compared tensors and their elements of |reference(edited) - reference| / (k 2^-24 A), with the case's own k
    and A: how many bounds the edit moves the most sensitive element."""
    ref, mag = c.ref(), c.mag()
    new = reference(c.params, data, c.mod, c.upstream)
    worst, where = 0.0, None
    for name in TENSORS:
        diff = (new[name] - ref[name]).abs()
        m = mag[name]
        r = torch.where(m > 0, diff / (c.k[name] * U24 * m.clamp(min=1e-300)), torch.where(diff > 0, torch.full_like(diff, float('inf')), diff))
        if float(r.max()) > worst:
            worst, where = float(r.max()), name
    return worst, where
