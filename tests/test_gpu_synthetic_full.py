"""-m gpu: BASELINE config 5 AT FULL SIZE on one GPU (10 000 drugs, 2 000 relations, 50 M directed D-D
edges, dim 128 -- it fits in 288 GB) -- VERDICT r1 next-round item 1b.  The oracle cannot run this size in
seconds, so the checks are (i) size-independent properties (linearity, adjoint identity) and (ii) rows of
the outputs / gradients recomputed on the CPU in fp64 straight from the edge list with the REFERENCE's
evaluation order (per-edge X[src] . W_r, scatter-mean over all relations, + X root -- src/layers.py:162-188),
64 random rows per layer.  Config 5 feeds X directly (no P-P / P->D stages)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def synth():
    from tip_amd.data import synthetic_data_dict
    dd = synthetic_data_dict()                                            # config 5 defaults, seed 1111
    assert dd['n_drug'] == 10000 and dd['n_dd_et'] == 2000 and dd['dd_train_idx'].shape[1] == 50_000_000
    return dd


def _layer(seed, after_relu):
    from tip_amd.layers import MyRGCNConv2
    torch.manual_seed(seed)
    return MyRGCNConv2(128, 128, 2000, 32, after_relu=after_relu).to(DEV)


def _brute_rows(rows, x, ei, et, m):
    """fp64 reference rows: out[o] = (1/deg_o) sum_{e: dst=o} x[src_e] W_{r_e} + x[o] root."""
    basis, att, root = (t.detach().double().cpu() for t in (m.basis, m.att, m.root))
    w = (att @ basis.view(basis.shape[0], -1)).view(att.shape[0], basis.shape[1], basis.shape[2])
    src, dst = ei[0], ei[1]
    out = torch.zeros(len(rows), basis.shape[2], dtype=torch.float64)
    sel = torch.nonzero(torch.isin(dst, torch.as_tensor(rows))).view(-1)
    dsel = dst[sel]
    for i, o in enumerate(rows):
        e = sel[dsel == o]
        acc = torch.einsum('ei,eio->o', x[src[e]], w[et[e]])
        out[i] = acc / max(1, e.numel()) + x[o] @ root
    return out


def _check_layer_grads(m, x, upstream, g_x, ei, et, deg, rgc):
    """One layer's gradients from ITS upstream, fp64 on the GPU (plain torch): g' = upstream / deg(dst);
    dXB[b, v] = sum_{e: src_e = v} att[r_e, b] g'[dst_e];  dX[v] = upstream[v] root^T + sum_b basis_b dXB[b, v];
    d basis[b] = X^T dXB[b];  d att[r, b] = sum_{e in r} <X[src_e] basis_b, g'[dst_e]>."""
    n = x.shape[0]
    basis, att, root = (t.detach().double() for t in (m.basis, m.att, m.root))
    gp = upstream / deg[:, None]
    src, dst = ei[0], ei[1]
    rows = torch.tensor(sorted(np.random.RandomState(1).choice(n, 6, replace=False).tolist()) + [0, n - 1], device=x.device)
    bases = torch.tensor([0, 5, 17, 31], device=x.device)
    in_rows = torch.tensor([0, 3, 64, 127], device=x.device)
    # dXB restricted to the 8 rows (all bases) and to the 4 bases (all rows): chunks of edges, index_add in fp64
    pos = torch.full((n,), -1, dtype=torch.long, device=x.device)
    pos[rows] = torch.arange(rows.numel(), device=x.device)
    dxb_rows = torch.zeros(rows.numel(), basis.shape[0], gp.shape[1], dtype=torch.float64, device=x.device)
    dxb_b = torch.zeros(bases.numel(), n, gp.shape[1], dtype=torch.float64, device=x.device)
    step = 1 << 21
    for a in range(0, src.numel(), step):
        s_, d_, r_ = src[a:a + step], dst[a:a + step], et[a:a + step]
        g_e = gp[d_]
        for i in range(bases.numel()):
            dxb_b[i].index_add_(0, s_, att[r_, bases[i]].unsqueeze(1) * g_e)
        sel = pos[s_] >= 0
        dxb_rows.index_add_(0, pos[s_[sel]], att[r_[sel]].unsqueeze(2) * g_e[sel].unsqueeze(1))
    want_x = upstream[rows] @ root.t() + torch.einsum('vbo,bio->vi', dxb_rows, basis)
    got_x = g_x[rows].double()
    torch.testing.assert_close(got_x, want_x, rtol=1e-4, atol=2e-5 * float(want_x.abs().max()))
    want_b = torch.einsum('vi,bvo->bio', x[:, in_rows], dxb_b)
    got_b = m.basis.grad[bases][:, in_rows].double()
    torch.testing.assert_close(got_b, want_b, rtol=1e-4, atol=2e-5 * float(want_b.abs().max()))
    # d att: relations across the range, the last tile (1984 .. 1999) included
    for r in (0, 7, 640, 1234, 1984, 1990, 1998, 1999):
        a, b = int(rgc[r, 0]), int(rgc[r, 1])
        s_, d_ = src[a:b], dst[a:b]
        want = torch.einsum('ei,bio,eo->b', x[s_], basis, gp[d_])
        got = m.att.grad[r].double()
        torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-5 * float(want.abs().max()))


@pytest.mark.timeout(1500)
def test_config5_full_size_two_layers_rows_and_properties(synth):
    dd = synth
    N = dd['n_drug']
    ei_c, et_c = dd['dd_train_idx'], dd['dd_train_et']
    ei, et, rg = ei_c.to(DEV), et_c.to(DEV), dd['dd_train_range'].to(DEV)
    m1, m2 = _layer(1, False), _layer(2, True)
    g = torch.Generator().manual_seed(5)
    x0_c = torch.randn(N, 128, generator=g)
    x0 = x0_c.to(DEV).requires_grad_(True)
    h1 = m1(x0, ei, et, rg)
    h1.retain_grad()
    x1 = torch.relu(h1)
    x1.retain_grad()
    out = m2(x1, ei, et, rg)
    up_c = torch.randn(N, 128, generator=g)
    (out * up_c.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x0.grad).all())

    # (ii) 64 random rows of each layer's output from the edge list, fp64, reference evaluation order
    rows = sorted(np.random.RandomState(0).choice(N, 64, replace=False).tolist())
    want1 = _brute_rows(rows, x0_c.double(), ei_c, et_c, m1)
    got1 = h1.detach()[rows].double().cpu()
    torch.testing.assert_close(got1, want1, rtol=1e-5, atol=1e-5 * float(want1.abs().max()))
    x1_c = x1.detach().double().cpu()
    want2 = _brute_rows(rows, x1_c, ei_c, et_c, m2)
    torch.testing.assert_close(out.detach()[rows].double().cpu(), want2, rtol=1e-5, atol=1e-5 * float(want2.abs().max()))

    # gradients of layer 2 by hand for a few relations / rows:  g' = up / deg;
    #   d att[r, b] = sum_{e in r} g'[dst_e] . (x1[src_e] basis_b);   d root = x1^T up
    deg = torch.bincount(ei_c[1], minlength=N).clamp(min=1).double()
    gp = up_c.double() / deg[:, None]
    basis2 = m2.basis.detach().double().cpu()
    rel_ids = [0, 7, 1234, 1999]
    rgc = dd['dd_train_range']
    for r in rel_ids:
        a, b = int(rgc[r, 0]), int(rgc[r, 1])
        s, d_ = ei_c[0, a:b], ei_c[1, a:b]
        xb = torch.einsum('ei,bio->ebo', x1_c[s], basis2)                  # [E_r, B, out]
        want = torch.einsum('ebo,eo->b', xb, gp[d_])
        got = m2.att.grad[r].double().cpu()
        torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-5 * float(want.abs().max()))
    want_root = x1_c.t() @ up_c.double()
    torch.testing.assert_close(m2.root.grad.double().cpu(), want_root, rtol=1e-4, atol=2e-5 * float(want_root.abs().max()))

    # dX, d basis and d att of EACH layer against that layer's own upstream (layer 2: up; layer 1: the gradient that reached
    # h1), so that an error in one layer does not feed the other's check; fp64 torch on the GPU, from the edge list
    ei64, et64 = ei.long(), et.long()
    deg_d = torch.bincount(ei64[1], minlength=N).clamp(min=1).double()
    for m, x_in, upstream, gx in ((m2, x1.detach(), up_c.to(DEV), x1.grad), (m1, x0_c.to(DEV), h1.grad, x0.grad)):
        _check_layer_grads(m, x_in.double(), upstream.double(), gx, ei64, et64, deg_d, dd['dd_train_range'])

    # (i) linearity of a layer and the adjoint identity <J x', y> = <x', J^T y> at full size
    xa, xb_ = torch.randn(N, 128, device=DEV), torch.randn(N, 128, device=DEV)
    with torch.no_grad():
        lhs = m1(0.3 * xa - 1.7 * xb_, ei, et, rg)
        rhs = 0.3 * m1(xa, ei, et, rg) - 1.7 * m1(xb_, ei, et, rg)
    torch.testing.assert_close(lhs, rhs, rtol=1e-4, atol=2e-5 * float(rhs.abs().max()))
    xq = xa.clone().requires_grad_(True)
    y = torch.randn(N, 128, device=DEV)
    (m1(xq, ei, et, rg) * y).sum().backward()
    with torch.no_grad():
        jx = m1(xb_, ei, et, rg)
    a_ = float((jx.double() * y.double()).sum())
    b_ = float((xb_.double() * xq.grad.double()).sum())
    assert abs(a_ - b_) <= 1e-4 * max(1.0, abs(a_)), (a_, b_)
    # bitwise reproducibility of the large-graph path (fixed summation order, no float atomics)
    with torch.no_grad():
        assert torch.equal(m1(xa, ei, et, rg), m1(xa, ei, et, rg))
