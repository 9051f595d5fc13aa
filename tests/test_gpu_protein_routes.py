"""The protein stage against fp64 (-m gpu): every route of `FMEncoder.mixed_drug_features` (asserted from the launch labels), GCNConv
on kept rows, and the C handles of GCNConv / MyHierarchyConv (`tipk_gcn_*`, `tipk_hier_*`), on the graphs of
`tests/protein_cases.py` (isolated proteins, self-loops, duplicates, edges without a mirror, a split hub row, drugs without targets
and drugs on every workgroup width of the P -> D launch, a source beyond `max_edges`, a run of kept rows beyond `max_rows`, an
edge that ends at a protein row).

Every tensor is compared elementwise: |got - want| <= k 2^-24 A, k per tensor (`protein_cases.chain_lengths`, `abs_bound`);
conv1's pre-activations are clear of zero by 100 x their tolerance (tests/test_host_protein_cases.py), so no element is
excluded.  Every comparison prints its ratio |got - want| / (2^-24 A) next to k (`-s`); profiles/protein_routes_errors.md
explains the bound and how to read the lines.  Bitwise equality is claimed only between two runs of the same route."""
import ctypes as C
import re

import pytest
import torch

import protein_cases as P
from route_harness import _bits, _labels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OK, EINVAL, EUNSUPPORTED = 0, -1, -2

# route -> (labels its pass must launch, labels it must not); regular expressions over the sorted labels of one forward +
# backward pass
ROUTE_MARKS = {
    'pd_stage': ([r'pd_stage_bwd\[', r'gather_sum_lin\[pp\.fwd\.rows', r'drug_mix_gather_fwd\['], [r'drug_mix_bwd\[', r'drug_mix_mm\[', r'drug_mix\[']),
    'agg_first_link': ([r'gather_sum_lin\[pp\.fwd\.rows', r'drug_mix_gather_fwd\[', r'drug_mix_bwd\[', r'gather_sum\[pp\.bwd\.rows,d=\d+\]\+\d+ sums'],
                       [r'pd_stage_bwd\[', r'drug_mix_mm\[', r'drug_mix\[']),
    'transform_first_rows': ([r'gather_sum\[pp\.fwd\.rows,d=12\]', r'gather_sum\[pp\.bwd\.rows,d=12\]', r'drug_mix_gather_fwd\['],
                             [r'gather_sum_lin\[', r'pd_stage_bwd\[', r'drug_mix_mm\[', r'drug_mix\[']),
    'sparse_rows': ([r'gather_sum\[feat\.fwd,d=32\]', r'gather_sum_lin\[pp\.fwd\.rows', r'gather_sum\[pp\.bwd\.rows,d=32\]( |$)', r'drug_mix_gather_fwd\['],
                    [r'pd_stage_bwd\[', r'pp\.bwd\.rows,d=\d+\]\+', r'drug_mix_mm\[', r'drug_mix\[']),
    'unpruned': ([r'gather_sum\[pp\.fwd,d=16\]', r'gather_sum\[pp\.bwd,d=16\]', r'drug_mix_gather_fwd\['],
                 [r'pp\.fwd\.rows', r'pp\.bwd\.rows', r'pd_stage_bwd\[', r'drug_mix_mm\[', r'drug_mix\[']),
    'mean_mm_fused': ([r'drug_mix_mm\[[^\]]*,fused\]', r'gather_sum\[pd\.fwd,d=7\]', r'gather_sum\[pd\.bwd,d=7\]'],
                      [r'drug_mix_gather_fwd\[', r'pd_stage_bwd\[', r'drug_mix\[', r',unfused\]']),
    'mean_mm_unfused': ([r'drug_mix_mm\[[^\]]*,unfused\]', r'gather_sum\[pd\.fwd,d=72\]', r'gather_sum\[pd\.bwd,d=72\]'],
                        [r'drug_mix_gather_fwd\[', r'pd_stage_bwd\[', r'drug_mix\[', r',fused\]']),
    'concat': ([r'drug_mix\[', r'gather_sum\[pd\.fwd,d=16\]', r'gather_sum\[pp\.fwd,d=16\]'],
               [r'pp\.fwd\.rows', r'drug_mix_gather_fwd\[', r'pd_stage_bwd\[', r'drug_mix_mm\[']),
}


def _lib():
    from tip_amd import _lib as L
    return L.lib()


def _limits():
    return P.pd_limits()


def _check(name, got, want, mag, k, where):
    """k: a number, or one value per column.  Prints the measured ratio |got - want| / (2^-24 A) next to k (profiles/)."""
    ratio, used = P.worst_ratio(got, want, mag), P.worst_ratio(got, want, mag, k)
    print('RATIO %s %s %.2f (k = %d, used %.4f)' % (where, name, ratio, int(torch.as_tensor(k).max()), used))
    assert used <= 1, (where, name, ratio, k)


# ------------------------------------------------------------------------------------------------ the dispatcher's routes
def _identity(n):
    ar = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.ones(n), (n, n)).to(DEV)


def _encoder(cid, case):
    from tip_amd.layers import FMEncoder, MyHierarchyConv, PPEncoder
    _, _, feat, mod, (hid1, hid2), _, prune, _ = P.ROUTE_CASES[cid]
    n_prot, n_drug = case.n_prot, case.n_drug
    in_dim = n_prot if feat == 'identity' else 24
    enc = FMEncoder(DEV, n_drug, 3, in_dim, n_prot, n_drug, prot_drug_dim=case.pd_dim, num_base=4, n_embed=case.n_embed, n_hid1=8,
                    n_hid2=4, mod=mod)
    if (hid1, hid2) != (32, 16):
        enc.pp_encoder = PPEncoder(in_dim, hid1, hid2)
        enc.hgcn = MyHierarchyConv(hid2, case.pd_dim, n_prot, n_drug)
        enc.hdrug = torch.zeros((n_drug, hid2), device=DEV)
    enc = enc.to(DEV)
    c1, c2 = enc.pp_encoder.conv1, enc.pp_encoder.conv2
    c1.chunk = c2.chunk = enc.hgcn.chunk = P.CHUNK
    enc.prune_pp_rows = prune
    p = case.params
    with torch.no_grad():
        for dst, key in ((c1.lin.weight, 'conv1.weight'), (c1.bias, 'conv1.bias'), (c2.lin.weight, 'conv2.weight'), (c2.bias, 'conv2.bias'),
                         (enc.hgcn.weight, 'hgcn.weight'), (enc.embed, 'embed')):
            assert dst.shape == p[key].shape
            dst.copy_(p[key].to(DEV))
    assert c1.lin.weight.t().is_contiguous() and c2.lin.weight.t().is_contiguous()      # [in, out] memory behind the [out, in] shape
    return enc


def _x_prot(case):
    if case.feat == 'identity':
        return _identity(case.n_prot)
    if case.feat == 'sparse':
        idx, val = P.sparse_features(case.n_prot, 24, case.seed)
        x = torch.sparse_coo_tensor(idx.to(DEV), val.to(DEV), (case.n_prot, 24))
        assert not x.is_coalesced()
        return x
    return case.x.to(DEV).requires_grad_()


def _named_grads(enc, x_prot):
    c1, c2 = enc.pp_encoder.conv1, enc.pp_encoder.conv2
    out = {'grad.embed': enc.embed.grad, 'grad.conv1.weight': c1.lin.weight.grad, 'grad.conv1.bias': c1.bias.grad,
           'grad.conv2.weight': c2.lin.weight.grad, 'grad.conv2.bias': c2.bias.grad, 'grad.hgcn.weight': enc.hgcn.weight.grad}
    if not x_prot.is_sparse:
        out['grad.x_prot'] = x_prot.grad
    return out


@pytest.mark.parametrize('cid', list(P.ROUTE_CASES))
def test_route(cid, monkeypatch):
    from tip_amd.plan import group_slots_for
    _, variant, feat, mod, (hid1, hid2), no_step, prune, route = P.ROUTE_CASES[cid]
    monkeypatch.delenv('TIPK_NO_ENCODER_STEP', raising=False)
    if no_step:
        monkeypatch.setenv('TIPK_NO_ENCODER_STEP', '1')
    case = P.route_case(cid, _limits())
    pp, pd, d_norm = case.graphs
    P.check_protein_graph(pp, pd, d_norm, case.n_prot, case.n_drug, variant, _limits())
    L = _lib()
    # what the route relies on, asked of the library itself
    if (hid1, hid2) in ((32, 16), (24, 12)):
        assert bool(L.tipk_gather_sum_lin_supported(hid1, hid2, group_slots_for(hid1))) == ((hid1, hid2) == (32, 16))
    assert bool(L.tipk_drug_mix_gather_supported(hid2, case.pd_dim)) == (hid2 in (12, 16))
    enc = _encoder(cid, case)
    x_prot, x_drug = _x_prot(case), _identity(case.n_drug)
    pp_d, pd_d, dn_d = pp.to(DEV), pd.to(DEV), d_norm.to(DEV).contiguous()
    up_wide = torch.zeros(case.n_drug, case.d0 + 8)
    up_wide[:, 4:4 + case.d0] = case.upstream
    up = up_wide.to(DEV)[:, 4:4 + case.d0]                                # a column slice: strided rows
    assert not up.is_contiguous()

    def one_pass():
        for t in list(enc.parameters()) + [x_prot]:
            t.grad = None
        x0 = enc.mixed_drug_features(x_drug, dn_d, x_prot, pp_d, pd_d, None)
        x0.backward(up)
        return x0.detach(), _named_grads(enc, x_prot)

    (x0, grads), labels = _labels(one_pass)
    must, must_not = ROUTE_MARKS[route]
    for pat in must:
        assert re.search(pat, labels), (cid, route, 'missing', pat, labels)
    for pat in must_not:
        assert not re.search(pat, labels), (cid, route, 'unexpected', pat, labels)
    # the hub row is split in the plans of this pass (the layers' own builder, their chunk and widths)
    from tip_amd.layers import gcn_norm_graph
    c1, c2 = enc.pp_encoder.conv1, enc.pp_encoder.conv2
    assert P.row_pieces(gcn_norm_graph(pp_d, case.n_prot, c1.chunk, c1.out_channels).fwd, P.HUB) > 1
    rows = enc.hgcn.source_rows(pd_d)
    assert (rows is None) == (variant == 'drug_source')
    if variant == 'all_sources':
        assert rows.numel() == case.n_prot
    pruned = prune and rows is not None and rows.numel() < case.n_prot        # conv2 ran on the kept rows only
    assert pruned == (route not in ('unpruned', 'concat') and variant != 'all_sources')
    assert pruned == ('pp.fwd.rows' in labels)
    hub = int((rows.cpu() == P.HUB).nonzero()) if pruned else P.HUB
    for d in (c2.in_channels, c2.out_channels):                               # aggregate-first | transform-first
        assert P.row_pieces(gcn_norm_graph(pp_d, case.n_prot, c2.chunk, d, rows if pruned else None).fwd, hub) > 1
    ref, mag = case.ref(), case.mag()
    _check('x0', x0, ref['x0'], mag['x0'], case.k_of('x0'), cid)
    # (general sparse features are a constant of the graph: the reference holds them as a dense matrix, the layer gives no gradient)
    assert set(grads) == set(k for k in ref if k.startswith('grad.')) - ({'grad.x_prot'} if feat == 'sparse' else set())
    for name, got in grads.items():
        assert got is not None, name
        _check(name, got, ref[name], mag[name], case.k_of(name), cid)
    for conv in (c1, c2):
        assert conv.lin.weight.grad.stride() == conv.lin.weight.stride()
    # drugs without targets: the P -> D part of their row is an exact zero
    cnt = torch.bincount(pd[1][pd[1] >= case.n_prot] - case.n_prot, minlength=case.n_drug)
    if mod == 'cat':
        assert bool((x0[(cnt == 0).to(DEV), case.n_embed:] == 0).all())
    # the same route again: the same bits
    x0_b, grads_b = one_pass()
    torch.cuda.synchronize()
    assert torch.equal(_bits(x0), _bits(x0_b))
    for name in grads:
        assert torch.equal(_bits(grads[name]), _bits(grads_b[name])), name


def test_route_table_covers_every_route_feature_kind_and_mod():
    rows = list(P.ROUTE_CASES.values())
    assert {r[7] for r in rows} == set(ROUTE_MARKS)
    assert {r[2] for r in rows} == {'identity', 'sparse', 'dense'}
    for routes in (('pd_stage',), ('agg_first_link',), ('mean_mm_fused', 'mean_mm_unfused')):
        assert {r[3] for r in rows if r[7] in routes} == {'cat', 'add'}, routes
    assert {r[1] for r in rows} == {'pruned', 'all_sources', 'drug_source'}
    assert any(not r[6] for r in rows) and any(r[5] for r in rows)


@pytest.mark.parametrize('d_in,d_out', [(32, 16), (24, 12)])
def test_gcn_conv_on_kept_rows_with_a_loop_only_row(d_in, d_out):
    """GCNConv alone: `gate_input=True` off the aggregate-first route is refused; `rows=` with a kept row whose only in-edge is
    its own loop (weight exactly 1: out = x W^T + b there), aggregate-first (32 -> 16) and transform-first (24 -> 12)."""
    from tip_amd.layers import GCNConv
    n_prot, n_drug, seed = P.SIZES[0]
    pp, pd, _ = P.protein_graph(n_prot, n_drug, seed, 'pruned', _limits())
    rows = torch.unique(pd[0])
    iso = P.isolated_proteins(n_prot)[0]
    assert iso in rows.tolist() and not bool((pp == iso).any())
    g = torch.Generator().manual_seed(d_in)
    x, w = torch.randn(n_prot, d_in, generator=g), torch.randn(d_out, d_in, generator=g) / d_in ** 0.5
    b, up = torch.randn(d_out, generator=g), torch.randn(rows.numel(), d_out, generator=g)
    conv = GCNConv(d_in, d_out, chunk=P.CHUNK).to(DEV)
    with torch.no_grad():
        conv.lin.weight.copy_(w.to(DEV))
        conv.bias.copy_(b.to(DEV))
    xd, pp_d, rows_d = x.to(DEV).requires_grad_(), pp.to(DEV), rows.to(DEV)
    agg_first = conv.aggregates_first(xd, rows_d)
    assert agg_first == (d_in == 32)
    with pytest.raises(NotImplementedError):
        conv(xd, pp_d, gate_input=True)                                       # every row: transform-first
    if not agg_first:
        with pytest.raises(NotImplementedError):
            conv(xd, pp_d, rows=rows_d, gate_input=True)
    out, labels = _labels(lambda: conv(xd, pp_d, rows=rows_d))
    assert ('gather_sum_lin[pp.fwd.rows' in labels) == agg_first
    out.backward(up.to(DEV))
    up_all = torch.zeros(n_prot, d_out).index_copy_(0, rows, up)
    ref = P.gcn_layer_reference(pp, n_prot, x, w, b, False, up_all)
    mag = P.gcn_layer_reference(pp, n_prot, x, w, b, False, up_all, absolute=True)
    k = P.gcn_layer_chain(pp, n_prot, d_in, d_out, identity=False)
    where = 'gcn_rows_%d_%d' % (d_in, d_out)
    _check('out', out, ref['out'][rows], mag['out'][rows], k['out'], where)
    i = int((rows == iso).nonzero())
    lone = x[iso].double() @ w.double().t() + b.double()
    # the loop's weight is exactly 1: d_in products, their sum, the bias
    assert float(((out[i].detach().cpu().double() - lone).abs() / mag['out'][iso]).max()) <= (d_in + 2) * P.U24
    _check('g_x', xd.grad, ref['g_x'], mag['g_x'], k['g_x'], where)
    _check('g_w', conv.lin.weight.grad, ref['g_w'], mag['g_w'], k['g_w'], where)
    _check('g_b', conv.bias.grad, ref['g_b'], mag['g_b'], k['g_b'], where)
    assert conv.lin.weight.grad.stride() == conv.lin.weight.stride()


# ------------------------------------------------------------------------------------------------ the C handles
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


CANARY, PAD = 0xA5, 256


class _Workspace(object):
    """Exactly `nbytes` of workspace inside a larger buffer filled with a canary on both sides."""

    def __init__(self, nbytes):
        assert nbytes >= 0
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * PAD,), CANARY, dtype=torch.uint8, device=DEV)
        self.ws = self.buf[PAD:PAD + self.nbytes]
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + PAD)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.nbytes:] == CANARY).all())


def _padded(t, pad=4, fill=777.0):
    """(buffer [rows, cols + pad] filled with `fill`, its [:, :cols] view holding t): a matrix with a padded leading dimension."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _build(kind, ei, idx_bytes, *dims):
    L = _lib()
    ei_d = ei.to(DEV).to(torch.int32 if idx_bytes == 4 else torch.int64).contiguous()
    h = C.c_void_p()
    fn = L.tipk_gcn_graph_build if kind == 'gcn' else L.tipk_hier_graph_build
    st = fn(_ptr(ei_d) if ei_d.numel() else None, idx_bytes, ei_d.shape[1], *dims, C.byref(h))
    return st, h


def _gcn_layer(case):
    """conv1 of a stage case as the layer under test: its pre-activations are clear of the ReLU kink."""
    p = case.params
    return case.x, p['conv1.weight'], p['conv1.bias']


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('feat', ['identity', 'dense'])
@pytest.mark.parametrize('idx_bytes', [4, 8])
def test_gcn_handle(idx_bytes, feat, relu):
    L = _lib()
    case = P.route_case('A_add_identity' if feat == 'identity' else 'A_cat_dense', _limits())
    pp, pd, _ = case.graphs
    n = case.n_prot
    x, w, b = _gcn_layer(case)
    d_out = w.shape[0]
    up = torch.randn(n, d_out, generator=torch.Generator().manual_seed(5))
    ref = P.gcn_layer_reference(pp, n, x, w, b, bool(relu), up)
    mag = P.gcn_layer_reference(pp, n, x, w, b, bool(relu), up, absolute=True, mask=(ref['pre'] > 0).double())
    k = P.gcn_layer_chain(pp, n, case.in_terms, d_out, identity=x is None)
    st, h = _build('gcn', pp, idx_bytes, n)
    assert st == OK and h.value
    try:
        d_in = n if x is None else x.shape[1]
        nbytes = L.tipk_gcn_workspace_bytes(h, d_in, d_out)
        assert nbytes > 0
        ws = _Workspace(nbytes)
        out_buf, out = _padded(torch.zeros(n, d_out))
        up_buf, up_d = _padded(up)
        b_d = b.to(DEV)
        if x is None:
            w_mem = w.t().contiguous().to(DEV)                                # [in, out] memory: w_so = 1, w_si = d_out
            w_so, w_si = 1, d_out
            x_ptr, ld_x, gx_buf, gx, ld_gx = None, 0, None, None, 0
        else:
            w_mem = w.contiguous().to(DEV)                                    # [out, in] memory
            w_so, w_si = d_in, 1
            x_buf, x_d = _padded(x, pad=8)
            x_ptr, ld_x = _ptr(x_d), x_buf.stride(0)
            gx_buf, gx = _padded(torch.zeros(n, d_in), pad=8)
            ld_gx = gx_buf.stride(0)
        assert L.tipk_gcn_fwd(h, x_ptr, ld_x, d_in, _ptr(w_mem), w_so, w_si, _ptr(b_d), d_out, relu, _ptr(out), out_buf.stride(0),
                              ws.ptr(), ws.nbytes, _stream()) == OK
        assert ws.intact()
        where = 'gcn_handle_%s_relu%d_idx%d' % (feat, relu, idx_bytes)
        _check('out', out, ref['out'], mag['out'], k['out'], where)
        assert bool((out_buf[:, d_out:] == 777.0).all())
        g_w = torch.full_like(w_mem, 555.0)
        g_b = torch.full((d_out,), 555.0, device=DEV)

        def bwd(gx_p, gb_p):
            return L.tipk_gcn_bwd(h, x_ptr, ld_x, d_in, _ptr(w_mem), w_so, w_si, d_out, _ptr(up_d), up_buf.stride(0),
                                  _ptr(out) if relu else None, out_buf.stride(0) if relu else 0, gx_p, ld_gx, _ptr(g_w), w_so, w_si, gb_p,
                                  ws.ptr(), ws.nbytes, _stream())
        assert bwd(_ptr(gx), _ptr(g_b)) == OK
        assert ws.intact()
        g_w_ref, g_w_mag = (ref['g_w'].t(), mag['g_w'].t()) if x is None else (ref['g_w'], mag['g_w'])
        _check('g_w', g_w, g_w_ref, g_w_mag, k['g_w'], where)
        _check('g_b', g_b, ref['g_b'], mag['g_b'], k['g_b'], where)
        if x is not None:
            _check('g_x', gx, ref['g_x'], mag['g_x'], k['g_x'], where)
            assert bool((gx_buf[:, d_in:] == 777.0).all())
        # g_x = NULL and g_bias = NULL: the same d W, nothing else written
        first = g_w.clone()
        g_w.fill_(555.0)
        g_b.fill_(555.0)
        if gx is not None:
            gx.fill_(333.0)
        assert bwd(None, None) == OK
        assert ws.intact()
        assert torch.equal(_bits(g_w), _bits(first)) and bool((g_b == 555.0).all()) and (gx is None or bool((gx == 333.0).all()))
    finally:
        assert L.tipk_graph_destroy(h) == OK


@pytest.mark.parametrize('feat', ['identity', 'dense'])
def test_gcn_handle_on_a_graph_without_edges(feat):
    """n_edges = 0: the unit loops alone, out = x W^T + b (identity features: W^T + b) and d W = x^T g, d b = 1^T g, d x = g W."""
    L = _lib()
    n, d_in, d_out = 70, 24, 16
    g = torch.Generator().manual_seed(3)
    x = None if feat == 'identity' else torch.randn(n, d_in, generator=g)
    d_in = n if x is None else d_in
    w, b, up = torch.randn(d_out, d_in, generator=g), torch.randn(d_out, generator=g), torch.randn(n, d_out, generator=g)
    empty = torch.zeros((2, 0), dtype=torch.int64)
    ref = P.gcn_layer_reference(empty, n, x, w, b, False, up)
    mag = P.gcn_layer_reference(empty, n, x, w, b, False, up, absolute=True)
    st, h = _build('gcn', empty, 8, n)
    assert st == OK and h.value
    try:
        ws = _Workspace(L.tipk_gcn_workspace_bytes(h, d_in, d_out))
        out, g_b = torch.empty(n, d_out, device=DEV), torch.empty(d_out, device=DEV)
        up_d, b_d = up.to(DEV), b.to(DEV)
        if x is None:
            w_mem, w_so, w_si, x_d, gx = w.t().contiguous().to(DEV), 1, d_out, None, None
        else:
            w_mem, w_so, w_si, x_d = w.contiguous().to(DEV), d_in, 1, x.to(DEV)
            gx = torch.empty(n, d_in, device=DEV)
        g_w = torch.empty_like(w_mem)
        assert L.tipk_gcn_fwd(h, _ptr(x_d), d_in if x is not None else 0, d_in, _ptr(w_mem), w_so, w_si, _ptr(b_d), d_out, 0, _ptr(out), d_out,
                              ws.ptr(), ws.nbytes, _stream()) == OK
        assert L.tipk_gcn_bwd(h, _ptr(x_d), d_in if x is not None else 0, d_in, _ptr(w_mem), w_so, w_si, d_out, _ptr(up_d), d_out, None, 0,
                              _ptr(gx), d_in if gx is not None else 0, _ptr(g_w), w_so, w_si, _ptr(g_b), ws.ptr(), ws.nbytes, _stream()) == OK
        assert ws.intact()
        k = P.gcn_layer_chain(empty, n, 1 if x is None else d_in, d_out, identity=x is None)
        where = 'gcn_handle_no_edges_' + feat
        _check('out', out, ref['out'], mag['out'], k['out'], where)
        _check('g_w', g_w, ref['g_w'].t() if x is None else ref['g_w'], mag['g_w'].t() if x is None else mag['g_w'], k['g_w'], where)
        _check('g_b', g_b, ref['g_b'], mag['g_b'], k['g_b'], where)
        if x is not None:
            _check('g_x', gx, ref['g_x'], mag['g_x'], k['g_x'], where)
    finally:
        assert L.tipk_graph_destroy(h) == OK


@pytest.mark.parametrize('variant', ['pruned', 'drug_source', 'no_pd_edges_to_targets'])
@pytest.mark.parametrize('idx_bytes', [4, 8])
def test_hier_handle(idx_bytes, variant):
    L = _lib()
    n_prot, n_drug, seed = P.SIZES[0]
    pp, pd, d_norm = P.protein_graph(n_prot, n_drug, seed, variant, _limits())
    P.check_protein_graph(pp, pd, d_norm, n_prot, n_drug, variant, _limits())
    n_all, d_in, d_out = n_prot + n_drug, 16, 16
    g = torch.Generator().manual_seed(7)
    x, w, up = torch.randn(n_all, d_in, generator=g), torch.randn(d_in, d_out, generator=g), torch.randn(n_drug, d_out, generator=g)
    ref = P.hier_layer_reference(pd, n_all, n_prot, x, w, up)
    mag = P.hier_layer_reference(pd, n_all, n_prot, x, w, up, absolute=True)
    k = P.hier_layer_chain(pd, n_prot, n_drug, d_in, d_out)
    st, h = _build('hier', pd, idx_bytes, n_all, n_prot)
    assert st == OK and h.value
    try:
        ws = _Workspace(L.tipk_hier_workspace_bytes(h, d_in, d_out))
        x_buf, x_d = _padded(x)
        out_buf, out = _padded(torch.zeros(n_drug, d_out))
        up_buf, up_d = _padded(up)
        gx_buf, gx = _padded(torch.zeros(n_all, d_in))
        w_d, g_w = w.to(DEV), torch.full((d_in, d_out), 555.0, device=DEV)
        assert L.tipk_hier_fwd(h, _ptr(x_d), x_buf.stride(0), d_in, _ptr(w_d), d_out, _ptr(out), out_buf.stride(0), ws.ptr(), ws.nbytes,
                               _stream()) == OK

        def bwd(gx_p):
            return L.tipk_hier_bwd(h, _ptr(x_d), x_buf.stride(0), d_in, _ptr(w_d), d_out, _ptr(up_d), up_buf.stride(0), gx_p, gx_buf.stride(0),
                                   _ptr(g_w), ws.ptr(), ws.nbytes, _stream())
        assert bwd(_ptr(gx)) == OK
        assert ws.intact()
        where = 'hier_handle_%s_idx%d' % (variant, idx_bytes)
        _check('out', out, ref['out'], mag['out'], k['out'], where)
        _check('g_x', gx, ref['g_x'], mag['g_x'], k['g_x'], where)
        _check('g_w', g_w, ref['g_w'], mag['g_w'], k['g_w'], where)
        assert bool((out_buf[:, d_out:] == 777.0).all()) and bool((gx_buf[:, d_in:] == 777.0).all())
        keep = pd[1] >= n_prot
        cnt = torch.bincount(pd[1][keep] - n_prot, minlength=n_drug)
        assert int((cnt == 0).sum()) >= 2
        assert bool((out[(cnt == 0).to(DEV)] == 0).all()), 'drugs without targets: exact zero rows'
        if variant == 'no_pd_edges_to_targets':
            assert bool((out == 0).all()) and bool((gx == 0).all()) and bool((g_w == 0).all())
        first = g_w.clone()
        g_w.fill_(555.0)
        gx.fill_(333.0)
        assert bwd(None) == OK                                                # g_x = NULL
        assert ws.intact()
        assert torch.equal(_bits(g_w), _bits(first)) and bool((gx == 333.0).all())
    finally:
        assert L.tipk_graph_destroy(h) == OK


def test_handles_refuse_bad_arguments():
    """A misaligned or short workspace and a handle of the wrong kind: TIPK_EINVAL; an index out of range: the build returns
    TIPK_EINVAL and leaves *graph_out NULL."""
    L = _lib()
    n_prot, n_drug, seed = P.SIZES[0]
    pp, pd, _ = P.protein_graph(n_prot, n_drug, seed, 'pruned', _limits())
    n_all = n_prot + n_drug
    for kind, ei, dims, bad_values in (('gcn', pp, (n_prot,), (n_prot, -1)), ('hier', pd, (n_all, n_prot), (n_all, -1))):
        for bad in bad_values:
            for where in ((0, 5), (1, ei.shape[1] - 1)):
                e2 = ei.clone()
                e2[where] = bad
                for idx_bytes in (4, 8):
                    st, h = _build(kind, e2, idx_bytes, *dims)
                    assert st == EINVAL and not h.value, (kind, bad, where, idx_bytes)
    st, hg = _build('gcn', pp, 8, n_prot)
    assert st == OK
    st, hh = _build('hier', pd, 8, n_all, n_prot)
    assert st == OK
    try:
        d = 16
        assert L.tipk_gcn_workspace_bytes(hh, d, d) == -1 and L.tipk_hier_workspace_bytes(hg, d, d) == -1
        ws = _Workspace(max(L.tipk_gcn_workspace_bytes(hg, d, d), L.tipk_hier_workspace_bytes(hh, d, d)) + 256)
        xg, xh = torch.randn(n_prot, d, device=DEV), torch.randn(n_all, d, device=DEV)
        w, b = torch.randn(d, d, device=DEV), torch.randn(d, device=DEV)
        og, oh = torch.full((n_prot, d), 555.0, device=DEV), torch.full((n_drug, d), 555.0, device=DEV)
        gxg, gxh, gw, gb = torch.full_like(xg, 555.0), torch.full_like(xh, 555.0), torch.full_like(w, 555.0), torch.full_like(b, 555.0)
        need_g, need_h = L.tipk_gcn_workspace_bytes(hg, d, d), L.tipk_hier_workspace_bytes(hh, d, d)
        mis = C.c_void_p(ws.buf.data_ptr() + PAD + 4)

        def calls(h_gcn, h_hier, wp, nb_g, nb_h):
            s = _stream()
            return [L.tipk_gcn_fwd(h_gcn, _ptr(xg), d, d, _ptr(w), d, 1, _ptr(b), d, 0, _ptr(og), d, wp, nb_g, s),
                    L.tipk_gcn_bwd(h_gcn, _ptr(xg), d, d, _ptr(w), d, 1, d, _ptr(og), d, None, 0, _ptr(gxg), d, _ptr(gw), d, 1, _ptr(gb), wp, nb_g, s),
                    L.tipk_hier_fwd(h_hier, _ptr(xh), d, d, _ptr(w), d, _ptr(oh), d, wp, nb_h, s),
                    L.tipk_hier_bwd(h_hier, _ptr(xh), d, d, _ptr(w), d, _ptr(oh), d, _ptr(gxh), d, _ptr(gw), wp, nb_h, s)]
        assert calls(hg, hh, mis, need_g, need_h) == [EINVAL] * 4, 'misaligned workspace'
        assert calls(hg, hh, ws.ptr(), need_g - 1, need_h - 1) == [EINVAL] * 4, 'short workspace'
        assert calls(hh, hg, ws.ptr(), ws.nbytes, ws.nbytes) == [EINVAL] * 4, 'handle of the wrong kind'
        torch.cuda.synchronize()
        for t in (og, oh, gxg, gxh, gw, gb):
            assert bool((t == 555.0).all())
        assert ws.intact() and bool((ws.ws == CANARY).all())
    finally:
        assert L.tipk_graph_destroy(hg) == OK and L.tipk_graph_destroy(hh) == OK


@pytest.mark.parametrize('combo', ['dense_gw_si', 'identity_gw_so', 'identity_fwd_w_so'])
def test_unsupported_strides_leave_outputs_untouched(combo):
    """`gw_si != 1` with dense x, `gw_so != 1` with identity features, `w_so != 1` with identity features in the forward call:
    TIPK_EUNSUPPORTED, and every output buffer (and the workspace) keeps its bits."""
    L = _lib()
    n_prot, n_drug, seed = P.SIZES[0]
    pp, _, _ = P.protein_graph(n_prot, n_drug, seed, 'pruned', _limits())
    n, d_out = n_prot, 16
    dense = combo == 'dense_gw_si'
    d_in = 24 if dense else n
    st, h = _build('gcn', pp, 8, n)
    assert st == OK
    try:
        ws = _Workspace(L.tipk_gcn_workspace_bytes(h, d_in, d_out))
        x = torch.randn(n, d_in, device=DEV) if dense else None
        w = torch.randn(2 * d_in * d_out + 2 * n * d_out, device=DEV)           # room for any of the strides below
        g_w = torch.full_like(w, 555.0)
        g_b, g_x = torch.full((d_out,), 555.0, device=DEV), torch.full((n, d_in), 555.0, device=DEV)
        out, up, gate = torch.full((n, d_out), 555.0, device=DEV), torch.randn(n, d_out, device=DEV), torch.randn(n, d_out, device=DEV)
        b = torch.randn(d_out, device=DEV)
        if combo == 'identity_fwd_w_so':
            st = L.tipk_gcn_fwd(h, None, 0, d_in, _ptr(w), 2, 2 * d_out, _ptr(b), d_out, 1, _ptr(out), d_out, ws.ptr(), ws.nbytes, _stream())
        elif dense:
            st = L.tipk_gcn_bwd(h, _ptr(x), d_in, d_in, _ptr(w), d_in, 1, d_out, _ptr(up), d_out, _ptr(gate), d_out, _ptr(g_x), d_in,
                                _ptr(g_w), 2 * d_in, 2, _ptr(g_b), ws.ptr(), ws.nbytes, _stream())
        else:
            st = L.tipk_gcn_bwd(h, None, 0, d_in, _ptr(w), 1, d_out, d_out, _ptr(up), d_out, _ptr(gate), d_out, None, 0,
                                _ptr(g_w), 2, 2 * d_out, _ptr(g_b), ws.ptr(), ws.nbytes, _stream())
        assert st == EUNSUPPORTED
        torch.cuda.synchronize()
        for name, t in (('g_weight', g_w), ('g_bias', g_b), ('g_x', g_x), ('out', out)):
            assert bool((t == 555.0).all()), name + ' was written by an unsupported call'
        assert ws.intact() and bool((ws.ws == CANARY).all()), 'the workspace was written by an unsupported call'
    finally:
        assert L.tipk_graph_destroy(h) == OK
