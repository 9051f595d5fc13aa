"""The SMALL- and MID-graph routes of an R-GCN layer against fp64, at layer level (-m gpu), plus the op-level handle on the same
graphs.  The module-level table CASES names, per case, the shape, the route switches and the forward / backward route the
launch labels must show; `test_route_table_covers_every_route` (no GPU) fails when a route, a boundary or a variant loses its
last case.

Below the large-graph sizes (tests/test_gpu_large_routes.py) `rgcn_graph` and `_RGCN` choose among the pair form (cells of
att rows, a dense product on `tipk_pair_product` or on the tiled GEMM; symmetric graphs build half the cells), the LDS-resident
`rel_gather` and Y + `gather_sum` forward, and `pair_grads`, `rel_stream` + `node_products` / `dy_products` (fused with the
row mask, or two GEMMs), `rel_gather`, `gather_rows_csr` and `gather_sum` backward, then the dense tail on `wg_gemm_group` or,
where a reduction is too long for it, `gemm_group`.  The boundaries are computed from the library's own predicates (the R at
which the att table needs 2 / 4 / no LDS column blocks, the N at which the transposed pass stops fitting), not written down.

Every case runs twice: with random values (rel 1e-5 on out, 1e-4 on the gradients, scaled by max |want|) and with small
integers on a graph whose in-degrees are 0 or powers of two, where the result must equal fp64 BIT FOR BIT -- a dropped,
doubled or mis-scaled edge fails without any tolerance argument (`_exact_bound` proves beforehand that every partial sum of
the case is exact in fp32).  A second forward + backward pass must give the same bits."""
import ctypes as C
import re

import pytest
import torch

from oracle import tip_oracle as O
from route_harness import _bits, _close, _labels, check_small_graph, small_graph

DEV = 'cuda:0'
gpu = pytest.mark.gpu

FWD_ROUTES = ('pair_sym', 'pair_dir', 'pair_gemm', 'rel_gather', 'Y')
BWD_ROUTES = ('pair_grads', 'node_products_xbt', 'node_products', 'dy_fused', 'dy_unfused', 'rel_gather', 'csr', 'gather_sum')
TAILS = ('wg', 'grouped')

# symbolic sizes, resolved from the library's predicates (`_resolve`):
SPLIT1 = ('split_last', 1)        # the largest R whose att table [R, nb] stays in ONE LDS column block
SPLIT2 = ('split_first', 2)       # the smallest R that needs 2 column blocks (the two-layer cell launch is off there)
SPLIT4 = ('split_first', 4)
SPLIT0 = ('split_first', 0)       # the smallest R whose table does not fit at all: no pair form
RS256_LAST = ('rs_last', 256)     # the largest N whose transposed pass at d_out = 256 still streams from LDS
RS256_OFF = ('rs_first0', 256)    # the smallest N where it does not (rel_gather backward)

# id, N, R, d_in, d_out, n_bases, graph kind, switches, forward route, backward route, dense tail, variants
# (dense tail 'grouped': some product of the tail is not taken by `wg_gemm_job` -- d_out > 32 or 64 bases, or a reduction
# over N > 2 048 nodes -- and the tail runs on `gemm_group`)
CASES = [
    ('sym_nb32', 97, 40, 64, 32, 32, 'sym', (), 'pair_sym', 'pair_grads', 'wg', ()),
    ('near_sym_nb32', 97, 40, 64, 32, 32, 'near', (), 'pair_dir', 'pair_grads', 'wg', ()),
    ('sym_nb16', 203, 30, 48, 16, 16, 'sym', (), 'pair_sym', 'node_products_xbt', 'wg', ()),
    ('sym_nb8_d8', 61, 25, 24, 8, 8, 'sym', (), 'pair_sym', 'dy_fused', 'wg', ()),
    ('dir_nb32_d16', 150, 33, 32, 16, 32, 'dir', (), 'pair_dir', 'pair_grads', 'wg', ('etype',)),
    ('dir_nb16_d4', 99, 20, 16, 4, 16, 'dir', (), 'pair_dir', 'dy_fused', 'wg', ()),
    ('sym_d64_gemm', 130, 30, 32, 64, 32, 'sym', (), 'pair_gemm', 'node_products_xbt', 'grouped', ()),
    ('dir_nb64_gemm', 70, 20, 32, 32, 64, 'dir', (), 'pair_gemm', 'dy_unfused', 'grouped', ()),
    ('dir_no_pair_product', 97, 40, 32, 32, 32, 'dir', ('TIPK_NO_PAIR_PRODUCT',), 'pair_gemm', 'pair_grads', 'wg', ()),
    ('sym_no_pair_bwd', 97, 40, 64, 32, 32, 'sym', ('TIPK_NO_PAIR_BWD',), 'pair_sym', 'node_products_xbt', 'wg', ()),
    ('sym_no_dy_fused', 101, 40, 32, 8, 8, 'sym', ('TIPK_NO_DY_FUSED',), 'pair_sym', 'dy_unfused', 'wg', ()),
    ('nb5_rel_gather', 100, 40, 32, 32, 5, 'dir', (), 'rel_gather', 'node_products', 'wg', ('relu', 'gate')),
    ('nb12_d256_rs_last', RS256_LAST, 12, 16, 256, 12, 'dir', (), 'rel_gather', 'dy_fused', 'grouped', ()),
    ('nb5_d256_rs_off', RS256_OFF, 12, 16, 256, 5, 'sym', (), 'rel_gather', 'rel_gather', 'wg', ()),
    ('nb12_d6_Y', 203, 17, 16, 6, 12, 'dir', (), 'Y', 'gather_sum', 'wg', ('relu', 'gate')),
    ('no_rellocal', 97, 40, 32, 32, 32, 'sym', ('TIPK_NO_RELLOCAL',), 'Y', 'csr', 'wg', ()),
    ('n1024', 1024, 20, 16, 16, 8, 'dir', (), 'pair_dir', 'node_products_xbt', 'wg', ()),
    ('n1025', 1025, 20, 16, 16, 8, 'dir', (), 'Y', 'csr', 'wg', ()),
    ('n1025_d6', 1025, 10, 8, 6, 8, 'sym', (), 'Y', 'gather_sum', 'wg', ('etype',)),
    ('n4097', 4097, 9, 16, 32, 5, 'dir', (), 'Y', 'csr', 'grouped', ()),
    ('split1_last', 41, SPLIT1, 16, 16, 32, 'sym', (), 'pair_sym', 'pair_grads', 'wg', ()),
    ('split2_first', 42, SPLIT2, 16, 16, 32, 'sym', (), 'pair_sym', 'pair_grads', 'wg', ()),
    ('split4_first', 43, SPLIT4, 16, 32, 32, 'dir', (), 'pair_dir', 'pair_grads', 'wg', ()),
    ('split0_first', 40, SPLIT0, 16, 16, 32, 'sym', (), 'rel_gather', 'node_products', 'wg', ()),
    ('n1', 1, 3, 8, 8, 8, 'sym', (), 'pair_sym', 'dy_fused', 'wg', ()),
    ('r1', 50, 1, 16, 16, 8, 'dir', (), 'pair_dir', 'node_products_xbt', 'wg', ()),
]
CASE_IDS = [c[0] for c in CASES]


def _lib():
    from tip_amd import _lib as L
    return L.lib()


def _first(pred, lo=1, hi=1 << 22):
    """the smallest v in [lo, hi) with pred(v) (pred monotone: False ... False True ... True)."""
    assert pred(hi - 1)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def _resolve(v, nb):
    """a size of the table: an int, or a boundary computed from the library's predicates (the routes' own switches do not
    apply here: `tipk_*_supported` directly)."""
    if isinstance(v, int):
        return v
    kind, arg = v
    L = _lib()
    split = lambda r: int(L.tipk_stream_gather_supported(r, nb, 4))
    order = {1: 0, 2: 1, 4: 2, 0: 3}                                    # the split only moves 1 -> 2 -> 4 -> 0 as R grows
    if kind == 'split_first':
        r = _first(lambda r: order[split(r)] >= order[arg])
        assert split(r) == arg and split(r - 1) != arg
        return r
    if kind == 'split_last':
        r = _first(lambda r: order[split(r)] > order[arg]) - 1
        assert split(r) == arg and split(r + 1) != arg
        return r
    rs = lambda n: int(L.tipk_stream_gather_supported(n, arg, 4))
    n0 = _first(lambda n: rs(n) == 0, 1, 1025)
    assert rs(n0) == 0 and rs(n0 - 1) > 0
    return n0 if kind == 'rs_first0' else n0 - 1


def _case(cid):
    c = dict(zip(('id', 'N', 'R', 'd_in', 'd_out', 'nb', 'kind', 'switches', 'fwd', 'bwd', 'tail', 'variants'), CASES[CASE_IDS.index(cid)]))
    c['N'], c['R'] = _resolve(c['N'], c['nb']), _resolve(c['R'], c['nb'])
    return c


# ---------------------------------------------------------------------------------------------
# route of a pass, from its launch labels
# ---------------------------------------------------------------------------------------------
def fwd_route(lf, graph):
    """every forward route whose signature the labels show (a correct pass shows exactly one)."""
    found = []
    pair = 'pair_cells' in lf
    if pair and 'pair_product[' in lf:
        found.append('pair_sym' if graph.pair_fwd.symmetric else 'pair_dir')
    if pair and re.search(r'(^| )gemm\[[^ ]*slabs=g', lf):             # the pair product on the tiled GEMM (kgroup slabs)
        found.append('pair_gemm')
    if 'rel_gather[dd.fwd' in lf:
        found.append('rel_gather')
    if 'gather_sum[dd.fwd' in lf:
        found.append('Y')
    if 'row_products' in lf or 'dest_products' in lf:
        found.append('large')
    return found


def bwd_route(lf, lb):
    found = []
    if 'pair_grads[' in lb and 'pair_att_gather[' in lb:
        found.append('pair_grads')
    if 'rel_stream[dd.bwd' in lb:
        if 'node_products[' in lb:
            found.append('node_products_xbt' if 'pair_cells' in lf else 'node_products')
        elif 'dy_products[' in lb:
            found.append('dy_fused')
        else:
            found.append('dy_unfused')
    if 'rel_gather[dd.bwd' in lb:
        found.append('rel_gather')
    if 'gather_rows_csr[' in lb:
        found.append('csr')
    if 'gather_sum[dd.bwd' in lb:
        found.append('gather_sum')
    if 'row_products' in lb:
        found.append('large')
    return found


# ---------------------------------------------------------------------------------------------
# exact-integer variant
# ---------------------------------------------------------------------------------------------
def _ints(shape, gen):
    """-1, 0, 1 with probabilities 1/4, 1/2, 1/4."""
    return torch.tensor([-1.0, 0.0, 0.0, 1.0])[torch.randint(0, 4, shape, generator=gen)]


def _exact_bound(x, ei, rg, basis, att, root, up):
    """(max over every sum the layer forms of its sum of |terms|) x (the largest in-degree): below 2^24 every partial sum, in
    any order, is an exact fp32 number (integers scaled by 1 / deg, a power of two)."""
    ax, ab, aa, ar, au = (t.abs() for t in (x, basis, att, root, up))
    out, saved = O.rgcn_fwd(ax, ei, rg, ab, aa, ar)
    gx, gb, ga, gr = O.rgcn_bwd(au, ax, ei, ab, aa, ar, saved)
    xb, deg, rel = saved
    n, r, nb = x.shape[0], att.shape[0], att.shape[1]
    y = aa @ xb.reshape(nb, -1)
    g_y = O.gather_sum(au / deg.unsqueeze(1), ei[1], rel * n + ei[0], r * n).reshape(r, -1)
    g_xb = aa.t() @ g_y
    terms = (out * deg.unsqueeze(1), gx, gb, ga, gr, xb, y, g_xb, aa.sum(0))
    return max(float(t.max()) if t.numel() else 0.0 for t in terms) * float(deg.max())


def _want(x64, ei, rg, params, up64, relu, gate):
    basis, att, root = params
    want, saved = O.rgcn_fwd(x64, ei, rg, basis, att, root)
    g_out = up64
    if relu:
        g_out = torch.where(want > 0, g_out, torch.zeros_like(g_out))
        want = torch.relu(want)
    wx, wb, wa, wr = O.rgcn_bwd(g_out, x64, ei, basis, att, root, saved)
    if gate:
        wx = wx * (x64 > 0)
    return want, (wx, wb, wa, wr)


def _compare(got, want, exact, rel_tol):
    if exact:
        g = got.detach().to('cpu', torch.float64)
        assert torch.equal(g, want), 'not bit-equal to fp64: max |diff| %g at %d elements' % (
            float((g - want).abs().max()), int((g != want).sum()))
    else:
        _close(got, want, rel_tol)


def _run_case(cid, exact):
    from tip_amd.layers import MyRGCNConv, MyRGCNConv2
    c = _case(cid)
    N, R, d_in, d_out, nb = c['N'], c['R'], c['d_in'], c['d_out'], c['nb']
    relu, gate, etype = ('relu' in c['variants']), ('gate' in c['variants']), ('etype' in c['variants'])
    assert not (etype and (relu or gate)), 'MyRGCNConv.forward takes neither fuse_relu nor gate_input'
    seed = N * 7 + R * 3 + d_out + nb + (1000 if exact else 0)
    ei_c, et_c, rg_c = small_graph(N, R, seed, c['kind'], pow2=exact)
    check_small_graph(ei_c, et_c, N, R, c['kind'], exact)
    torch.manual_seed(seed)
    m = (MyRGCNConv if etype else MyRGCNConv2)(d_in, d_out, R, nb, after_relu=False).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    if exact:
        for p in (m.basis, m.att, m.root):
            p.data.copy_(_ints(p.shape, gen))
        x_c, up_c = _ints((N, d_in), gen), _ints((N, d_out), gen)
    else:
        x_c, up_c = torch.randn(N, d_in, generator=gen), torch.randn(N, d_out, generator=gen)
    if etype:
        # the edge-type form takes the edges in any order: shuffled, relation ids no longer sorted
        perm = torch.randperm(ei_c.shape[1], generator=gen)
        ei, et = ei_c[:, perm].to(DEV), et_c[perm].to(DEV)
        assert not bool((et[1:] >= et[:-1]).all())
        call = lambda x: m(x, ei, et)
    else:
        ei, et, rg = ei_c.to(DEV), et_c.to(DEV), rg_c.to(DEV)
        call = lambda x: m(x, ei, et, rg, fuse_relu=relu, gate_input=gate)

    def step():
        m.zero_grad()
        x = x_c.to(DEV).requires_grad_(True)
        out, lf = _labels(lambda: call(x))
        _, lb = _labels(lambda: out.backward(up_c.to(DEV)))
        return out.detach(), x.grad, [p.grad.clone() for p in (m.basis, m.att, m.root)], lf, lb
    out, gx, (gb, ga, gr), lf, lb = step()
    graph = m._cache.value
    assert fwd_route(lf, graph) == [c['fwd']], (cid, c['fwd'], lf)
    assert bwd_route(lf, lb) == [c['bwd']], (cid, c['bwd'], lf, lb)
    assert ('wg_gemm_group[' in lb) == (c['tail'] == 'wg'), (cid, c['tail'], lb)
    if c['kind'] != 'dir' and graph.pair_fwd is not None:
        # the one-edge break of symmetry must turn the half-cell form off (and nothing else may)
        assert graph.pair_fwd.symmetric == (c['kind'] == 'sym' and _lib().tipk_pair_product_supported(nb, d_out) == 1), cid
    if c['bwd'] == 'node_products_xbt':
        assert ('xbt', N, nb, d_out, str(torch.device(DEV))) in graph._pair_cells

    params = tuple(p.detach().double().cpu() for p in (m.basis, m.att, m.root))
    x64, up64 = x_c.double(), up_c.double()
    if exact:
        assert _exact_bound(x64, ei_c, rg_c, *params, up64) < 2 ** 24, cid
    want, grads = _want(x64, ei_c, rg_c, params, up64, relu, gate)
    _compare(out, want, exact, 1e-5)
    for got, w in zip((gx, gb, ga, gr), grads):
        _compare(got, w, exact, 1e-4)
    out2, gx2, grads2, lf2, lb2 = step()                                # second forward + backward: the same bits, the same route
    assert (lf2, lb2) == (lf, lb)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(gx), _bits(gx2))
    for a_, b_ in zip((gb, ga, gr), grads2):
        assert torch.equal(_bits(a_), _bits(b_))


@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize('exact', [False, True], ids=['random', 'exact'])
@pytest.mark.parametrize('cid', CASE_IDS)
def test_rgcn_route_matrix_vs_fp64(cid, exact, monkeypatch):
    for name in _case(cid)['switches']:
        monkeypatch.setenv(name, '1')
    _run_case(cid, exact)


# ---------------------------------------------------------------------------------------------
# two layers as FMEncoder drives them: ReLU handed down, output slab sum deferred, cells of both layers in one launch
# ---------------------------------------------------------------------------------------------
# id, N, R, d_in, n_bases, d_out of layer 2, graph kind, one cell launch for both layers, layer hand-over (sum_slabs_xb)
TWO_LAYER = [
    ('sym_nb32', 97, 40, 64, 32, 16, 'sym', True, True),
    ('dir_nb32', 77, 29, 40, 32, 32, 'dir', True, True),
    ('sym_nb16', 90, 25, 48, 16, 16, 'sym', True, False),          # no pair-form backward at 16 bases: no hand-over
    ('sym_nb32_split2', 45, SPLIT2, 32, 32, 16, 'sym', False, True),     # 2 column blocks: one layer per cell launch
]
TWO_IDS = [t[0] for t in TWO_LAYER]


@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize('switch', [None, 'TIPK_NO_CELLS_TWO', 'TIPK_NO_LAYER_HANDOVER'])
@pytest.mark.parametrize('tid', TWO_IDS)
def test_two_layer_handoffs_vs_fp64(tid, switch, monkeypatch):
    from tip_amd.layers import MyRGCNConv2
    _, N, R, d_in, nb, d_out, kind, cells_two, handover = TWO_LAYER[TWO_IDS.index(tid)]
    R = _resolve(R, nb)
    if switch:
        monkeypatch.setenv(switch, '1')
    seed = N + R + d_in
    ei_c, et_c, rg_c = small_graph(N, R, seed, kind)
    check_small_graph(ei_c, et_c, N, R, kind, False)
    torch.manual_seed(seed)
    m1 = MyRGCNConv2(d_in, 32, R, nb, after_relu=False).to(DEV)
    m2 = MyRGCNConv2(32, d_out, R, nb, after_relu=True).to(DEV)
    m1.paired = m2.paired = True                                      # as FMEncoder.__init__ sets them
    m1.plan_share = m2.plan_share = {}
    gen = torch.Generator().manual_seed(seed + 1)
    x_c, up_c = torch.randn(N, d_in, generator=gen), torch.randn(N, d_out, generator=gen)
    ei, et, rg = ei_c.to(DEV), et_c.to(DEV), rg_c.to(DEV)

    def step():
        m1.zero_grad()
        m2.zero_grad()
        x = x_c.to(DEV).requires_grad_(True)

        def fwd():
            tok = object()
            h = m1(x, ei, et, rg, fuse_relu='gated_downstream', defer_output=True, next_layer=m2, cells_token=tok)
            return m2(h, ei, et, rg, gate_input=True, cells_token=tok)
        out, lf = _labels(fwd)
        _, lb = _labels(lambda: out.backward(up_c.to(DEV)))
        return out.detach(), x.grad, [p.grad.clone() for m in (m1, m2) for p in (m.basis, m.att, m.root)], lf, lb
    out, gx, grads, lf, lb = step()
    g1 = m1.graph_for(N, ei, rg)
    assert g1.pair_fwd is not None and g1.pair_fwd.symmetric == (kind == 'sym')
    want_two = cells_two and switch != 'TIPK_NO_CELLS_TWO'
    want_ho = handover and switch != 'TIPK_NO_LAYER_HANDOVER'
    assert ('pair_cells2[' in lf) == want_two and ('pair_cells[' in lf) == (not want_two), (tid, switch, lf)
    assert ('sum_slabs_xb[' in lf) == want_ho, (tid, switch, lf)
    assert 'gather_sum[dd' not in lf + lb and 'rel_gather' not in lf + lb, (lf, lb)
    assert ('pair_grads[' in lb) == (nb == 32), lb

    p1 = tuple(p.detach().double().cpu() for p in (m1.basis, m1.att, m1.root))
    p2 = tuple(p.detach().double().cpu() for p in (m2.basis, m2.att, m2.root))
    x64 = x_c.double()
    pre1, s1 = O.rgcn_fwd(x64, ei_c, rg_c, *p1)
    h = torch.relu(pre1)
    want, s2 = O.rgcn_fwd(h, ei_c, rg_c, *p2)
    gh, gb2, ga2, gr2 = O.rgcn_bwd(up_c.double(), h, ei_c, *p2, s2)
    gx1, gb1, ga1, gr1 = O.rgcn_bwd(torch.where(pre1 > 0, gh, torch.zeros_like(gh)), x64, ei_c, *p1, s1)
    _close(out, want, 1e-5)
    for got, w in zip([gx] + grads, (gx1, gb1, ga1, gr1, gb2, ga2, gr2)):
        _close(got, w, 1e-4)
    out2, gx2, grads2, _, _ = step()
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(gx), _bits(gx2))
    for a_, b_ in zip(grads, grads2):
        assert torch.equal(_bits(a_), _bits(b_))


# ---------------------------------------------------------------------------------------------
# the op-level handle (include/tipk.h section 10) on the same graphs
# ---------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _handle_pass(L, h, x, basis, att, root, up, flags):
    """tipk_rgcn_fwd + tipk_rgcn_bwd_ex on a workspace filled with NaN bit patterns -> (out, gx, g basis, g att, g root)."""
    n, d_in = x.shape
    nb, _, d_out = basis.shape
    ws = torch.full((L.tipk_rgcn_workspace_bytes(h, d_in, d_out, nb),), 255, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(n, d_out, device=DEV)
    assert L.tipk_rgcn_fwd(h, _p(x), d_in, d_in, _p(basis), _p(att), _p(root), nb, d_out, 0, _p(out), d_out, _p(ws), ws.numel(), st) == 0
    if not flags:
        ws.fill_(255)                                                   # nothing of the forward pass may be read back
    gx, gb, ga, gr = torch.empty_like(x), torch.empty_like(basis), torch.empty_like(att), torch.empty_like(root)
    assert L.tipk_rgcn_bwd_ex(h, _p(x), d_in, d_in, _p(basis), _p(att), _p(root), nb, d_out, _p(up), d_out, None, 0, _p(gx), d_in,
                              _p(gb), _p(ga), _p(gr), _p(ws), ws.numel(), flags, st) == 0
    torch.cuda.synchronize()
    return out, gx, gb, ga, gr


# id, N, R, d_in, d_out, n_bases, graph kind, route the handle reports after tipk_graph_prepare_rgcn, edge-type form
HANDLE_CASES = [
    ('r0_n1025_d6', 1025, 9, 16, 6, 5, 'dir', 0, False),
    ('r0_n1025_d64', 1025, 9, 16, 64, 5, 'sym', 0, False),
    ('r0_n1025_d128', 1025, 9, 16, 128, 5, 'dir', 0, False),
    ('r0_n4097_d6', 4097, 7, 16, 6, 5, 'dir', 0, False),
    ('r0_n4097_d64', 4097, 7, 16, 64, 5, 'dir', 0, False),
    ('r0_n4097_d128', 4097, 7, 16, 128, 5, 'sym', 0, False),
    ('r1_nb16_sym', 203, 30, 32, 16, 16, 'sym', 1, False),
    ('r1_nb16_dir', 150, 33, 32, 16, 16, 'dir', 1, False),
    ('r1_nb16_etype', 150, 33, 32, 16, 16, 'dir', 1, True),
    ('r2_split2', 41, SPLIT2, 16, 16, 32, 'sym', 2, False),
    ('r2_split2_dir', 43, SPLIT2, 32, 32, 32, 'dir', 2, False),
]
HANDLE_IDS = [t[0] for t in HANDLE_CASES]


@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize('flags', [0, 1], ids=['cold', 'from_fwd'])
@pytest.mark.parametrize('hid', HANDLE_IDS)
def test_graph_handle_routes_vs_fp64(hid, flags):
    """Route 0 (generic) past the pair sizes, route 1 (pair-form forward, generic backward) and route 2 at a split-2 R against
    fp64, with and without TIPK_RGCN_WORKSPACE_FROM_FWD; on the pair routes the handle must also give the modules' bits
    (route 1: the forward pass; route 2: everything)."""
    from tip_amd.layers import MyRGCNConv2
    L = _lib()
    _, N, R, d_in, d_out, nb, kind, route, etype = HANDLE_CASES[HANDLE_IDS.index(hid)]
    R = _resolve(R, nb)
    seed = N + R + d_out + nb
    ei_c, et_c, rg_c = small_graph(N, R, seed, kind)
    check_small_graph(ei_c, et_c, N, R, kind, False)
    torch.manual_seed(seed)
    m = MyRGCNConv2(d_in, d_out, R, nb, after_relu=False).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    x_c, up_c = torch.randn(N, d_in, generator=gen), torch.randn(N, d_out, generator=gen)
    x, up = x_c.to(DEV), up_c.to(DEV)
    basis, att, root = (p.detach().contiguous() for p in (m.basis, m.att, m.root))
    h = C.c_void_p()
    if etype:
        perm = torch.randperm(ei_c.shape[1], generator=gen)
        ei_h, et_h = ei_c[:, perm].contiguous().to(DEV), et_c[perm].to(DEV)
        assert not bool((et_h[1:] >= et_h[:-1]).all())
        assert L.tipk_graph_build(_p(ei_h), _p(et_h), None, 8, ei_h.shape[1], N, R, None, C.byref(h)) == 0
    else:
        ei_h, rg_h = ei_c.to(DEV), rg_c.to(DEV)
        assert L.tipk_graph_build(_p(ei_h), None, _p(rg_h), 8, ei_h.shape[1], N, R, None, C.byref(h)) == 0
    try:
        prep = L.tipk_graph_prepare_rgcn(h, nb, d_out)
        assert prep == (0 if route else -2), prep
        assert L.tipk_graph_rgcn_route(h, nb, d_out) == route
        out, gx, gb, ga, gr = _handle_pass(L, h, x, basis, att, root, up, flags)
    finally:
        assert L.tipk_graph_destroy(h) == 0
    params = tuple(t.double().cpu() for t in (basis, att, root))
    want, grads = _want(x_c.double(), ei_c, rg_c, params, up_c.double(), False, False)
    _close(out, want, 1e-5)
    for got, w in zip((gx, gb, ga, gr), grads):
        _close(got, w, 1e-4)
    if route:
        ei, et, rg = ei_c.to(DEV), et_c.to(DEV), rg_c.to(DEV)
        xm = x_c.to(DEV).requires_grad_(True)
        mo, lf = _labels(lambda: m(xm, ei, et, rg))
        assert fwd_route(lf, m.graph_for(N, ei, rg))[0].startswith('pair_'), lf
        if not etype:                                                   # (the same edge order: the same plans)
            assert torch.equal(_bits(out), _bits(mo))
        if route == 2:
            mo.backward(up)
            for got, ref in ((gx, xm.grad), (gb, m.basis.grad), (ga, m.att.grad), (gr, m.root.grad)):
                assert torch.equal(_bits(got), _bits(ref))


# ---------------------------------------------------------------------------------------------
# no GPU: the tables keep every route, boundary and variant
# ---------------------------------------------------------------------------------------------
def _raw(c):
    return dict(zip(('id', 'N', 'R', 'd_in', 'd_out', 'nb', 'kind', 'switches', 'fwd', 'bwd', 'tail', 'variants'), c))


# what the route matrix must contain; each entry a predicate over one case of CASES
REQUIREMENTS = {
    'pair_sym nb=8': lambda c: c['fwd'] == 'pair_sym' and c['nb'] == 8,
    'pair_sym nb=16': lambda c: c['fwd'] == 'pair_sym' and c['nb'] == 16,
    'pair_sym nb=32': lambda c: c['fwd'] == 'pair_sym' and c['nb'] == 32,
    'near-symmetric': lambda c: c['kind'] == 'near' and c['fwd'] == 'pair_dir',
    'its symmetric twin': lambda c: c['kind'] == 'sym' and not c['switches'] and any(
        o['kind'] == 'near' and (o['N'], o['R'], o['d_in'], o['d_out'], o['nb']) == (c['N'], c['R'], c['d_in'], c['d_out'], c['nb'])
        for o in map(_raw, CASES)),
    'pair_dir': lambda c: c['fwd'] == 'pair_dir' and c['kind'] == 'dir',
    'pair_gemm, d_out > 32': lambda c: c['fwd'] == 'pair_gemm' and c['d_out'] > 32,
    'pair_gemm, nb = 64': lambda c: c['fwd'] == 'pair_gemm' and c['nb'] == 64,
    'pair_gemm, TIPK_NO_PAIR_PRODUCT': lambda c: c['fwd'] == 'pair_gemm' and 'TIPK_NO_PAIR_PRODUCT' in c['switches'],
    'rel_gather, nb no power of two': lambda c: c['fwd'] == 'rel_gather' and c['nb'] & (c['nb'] - 1),
    'rel_gather, att table past the LDS': lambda c: c['fwd'] == 'rel_gather' and c['R'] == SPLIT0,
    'Y at N = 1025': lambda c: c['fwd'] == 'Y' and c['N'] == 1025,
    'Y at a mid-size N': lambda c: c['fwd'] == 'Y' and c['N'] == 4097,
    'Y at a non-power-of-two d_out': lambda c: c['fwd'] == 'Y' and c['d_out'] == 6,
    'Y under TIPK_NO_RELLOCAL': lambda c: c['fwd'] == 'Y' and 'TIPK_NO_RELLOCAL' in c['switches'],
    'pair_grads': lambda c: c['bwd'] == 'pair_grads',
    'node_products + xbt, nb != 32': lambda c: c['bwd'] == 'node_products_xbt' and c['nb'] != 32,
    'node_products + xbt of the tiled GEMM': lambda c: c['bwd'] == 'node_products_xbt' and c['fwd'] == 'pair_gemm',
    'node_products + xbt, TIPK_NO_PAIR_BWD': lambda c: c['bwd'] == 'node_products_xbt' and 'TIPK_NO_PAIR_BWD' in c['switches'],
    'node_products without xbt': lambda c: c['bwd'] == 'node_products',
    'dy_fused, d_out = 4': lambda c: c['bwd'] == 'dy_fused' and c['d_out'] == 4,
    'dy_fused, d_out = 8': lambda c: c['bwd'] == 'dy_fused' and c['d_out'] == 8 and c['N'] > 1,
    'dy_fused, d_out = 256': lambda c: c['bwd'] == 'dy_fused' and c['d_out'] == 256,
    'dy_unfused, TIPK_NO_DY_FUSED': lambda c: c['bwd'] == 'dy_unfused' and 'TIPK_NO_DY_FUSED' in c['switches'],
    'dy_unfused, nb > 32': lambda c: c['bwd'] == 'dy_unfused' and c['nb'] > 32,
    'rel_gather backward, d_out = 256, first N past the stream table': lambda c: c['bwd'] == 'rel_gather' and c['N'] == RS256_OFF,
    'stream table at its last N': lambda c: c['N'] == RS256_LAST,
    'csr at N = 1025': lambda c: c['bwd'] == 'csr' and c['N'] == 1025,
    'csr at a small N': lambda c: c['bwd'] == 'csr' and isinstance(c['N'], int) and c['N'] <= 1024,
    'gather_sum backward at N = 1025': lambda c: c['bwd'] == 'gather_sum' and c['N'] == 1025,
    'gather_sum backward at a small N': lambda c: c['bwd'] == 'gather_sum' and isinstance(c['N'], int) and c['N'] <= 1024,
    'dense tail on gemm_group: a reduction past the one-workgroup products': lambda c: c['tail'] == 'grouped' and c['N'] == 4097,
    'N = 1024': lambda c: c['N'] == 1024,
    'split 1, last R': lambda c: c['R'] == SPLIT1,
    'split 2, first R': lambda c: c['R'] == SPLIT2,
    'split 4, first R': lambda c: c['R'] == SPLIT4,
    'N = 1': lambda c: c['N'] == 1,
    'R = 1': lambda c: c['R'] == 1,
    'fuse_relu + gate_input on rel_gather': lambda c: {'relu', 'gate'} <= set(c['variants']) and c['fwd'] == 'rel_gather',
    'fuse_relu + gate_input on Y': lambda c: {'relu', 'gate'} <= set(c['variants']) and c['fwd'] == 'Y',
    'MyRGCNConv on a pair route': lambda c: 'etype' in c['variants'] and c['fwd'].startswith('pair_'),
    'MyRGCNConv off the pair form': lambda c: 'etype' in c['variants'] and not c['fwd'].startswith('pair_'),
}


def test_route_table_covers_every_route():
    """Every forward route, backward route and dense tail of the small / mid-size graphs has a case (the exact-integer variant
    runs every case, so every route has one as well); every requirement above has a case, and every case is the ONLY one that
    meets some requirement -- dropping any case from CASES fails here, without a GPU."""
    cases = [_raw(c) for c in CASES]
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    assert {c['fwd'] for c in cases} == set(FWD_ROUTES)
    assert {c['bwd'] for c in cases} == set(BWD_ROUTES)
    assert {c['tail'] for c in cases} == set(TAILS)
    meets = {name: [c['id'] for c in cases if pred(c)] for name, pred in REQUIREMENTS.items()}
    missing = [name for name, ids in meets.items() if not ids]
    assert not missing, missing
    sole = {ids[0] for ids in meets.values() if len(ids) == 1}
    assert sole == set(CASE_IDS), sorted(set(CASE_IDS) - sole)
    # two-layer hand-offs: at least three pair-form shapes, each switch able to change the labels
    assert len(TWO_LAYER) >= 3 and any(t[7] for t in TWO_LAYER) and any(t[8] for t in TWO_LAYER)
    assert {t[7] for t in HANDLE_CASES} == {0, 1, 2} and any(t[8] for t in HANDLE_CASES)
    assert {(t[1], t[4]) for t in HANDLE_CASES if t[7] == 0} == {(n, d) for n in (1025, 4097) for d in (6, 64, 128)}
    # the pair form pads the source range to PAIR_KGROUP: N is no multiple of it, but at N = 1024 (the last pair-form N)
    from tip_amd.ops import PAIR_KGROUP
    for c in cases:
        if c['fwd'].startswith('pair_') and isinstance(c['N'], int) and c['N'] not in (1, 1024):
            assert c['N'] % PAIR_KGROUP, c['id']


def test_route_boundaries_come_from_the_library():
    """The symbolic sizes resolve to the boundaries the library reports (R 1 -> 2 -> 4 -> 0 column blocks of the att table,
    the last N of the LDS-resident transposed pass at d_out = 256), and N = 1024 / 1025 straddle the small-graph plans."""
    from tip_amd import _lib as Lm
    import os
    if not os.path.exists(Lm.LIB_PATH):
        Lm.build()
    L = _lib()
    for nb in (16, 32, 64):
        r1, r2, r4, r0 = (_resolve(v, nb) for v in (SPLIT1, SPLIT2, SPLIT4, SPLIT0))
        assert r1 + 1 == r2 < r4 < r0
        assert [L.tipk_stream_gather_supported(r, nb, 4) for r in (r1, r2, r4 - 1, r4, r0 - 1, r0)] == [1, 2, 2, 4, 4, 0]
    last, off = _resolve(RS256_LAST, 0), _resolve(RS256_OFF, 0)
    assert off == last + 1 and L.tipk_stream_gather_supported(off, 256, 4) == 0 < L.tipk_stream_gather_supported(last, 256, 4)
    assert L.tipk_rel_gather_supported(off, 256, 1) > 0                 # where the stream table stops fitting, rel_gather takes it
    assert L.tipk_rel_gather_supported(1024, 32, 0) > 0 and L.tipk_rel_gather_supported(1025, 32, 0) == 0
