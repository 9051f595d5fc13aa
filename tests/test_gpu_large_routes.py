"""-m gpu: the LARGE-graph routes of an R-GCN layer against fp64, at layer level.

Past the pair / LDS-resident forms (here: N >= 8 192, Y = R N d_out fp32 > 192 MB) `rgcn_graph` and `_RGCN` choose per pass
among `row_products_s`, the per-lane `row_products`, `dest_products`, the Y route over a segmented `gather_sum` plan (forward)
and `gather_rows_csr` / `gather_sum` (backward), by the layer's widths and node count.  Every case runs `MyRGCNConv2` forward and
backward with an upstream `up`, compares out, dX, d basis, d att and d root with `oracle.tip_oracle.rgcn_fwd / rgcn_bwd` in
float64 on the CPU (the reference's arithmetic, nothing of `tip_amd`), ASSERTS from the launch labels which route each pass
took (a later threshold change must not quietly make a case test something else) and that a second pass gives the same bits.

Every graph has relations 0 and R - 1 without edges (and, for R >= 66, the whole tile of relations 32 .. 63), nodes without
in-edges and nodes without out-edges, a hub with 10 000 in-edges, duplicate edges and self-loops."""
import pytest
import torch

from oracle import tip_oracle as O
from route_harness import _assert_route, _bits, _close, _graph, _labels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Y_BYTES = 192 << 20

def _run_case(N, R, d_in, d_out, nb, fwd, bwd, seed, fuse_relu=False, inf_up=False):
    from tip_amd.layers import MyRGCNConv2
    from tip_amd.plan import relations_per_segment
    assert R * N * d_out * 4 > Y_BYTES, 'not a large-graph case'
    ei_c, et_c, rg_c = _graph(N, R, seed)
    torch.manual_seed(seed)
    m = MyRGCNConv2(d_in, d_out, R, nb, after_relu=False).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    x_c = torch.randn(N, d_in, generator=g)
    up_c = torch.randn(N, d_out, generator=g)
    if inf_up:
        # node 1000: a few in-edges; the backward row sums by source put the Inf into rows (r, s) of those sources, whose
        # later rows must stay finite (their d att is finite in fp64)
        up_c[1000] = float('inf')
    ei, et, rg = ei_c.to(DEV), et_c.to(DEV), rg_c.to(DEV)

    def step():
        m.zero_grad()
        x = x_c.to(DEV).requires_grad_(True)
        out, lf = _labels(lambda: m(x, ei, et, rg, fuse_relu=fuse_relu))
        _, lb = _labels(lambda: out.backward(up_c.to(DEV)))
        return out.detach(), x.grad, [p.grad.clone() for p in (m.basis, m.att, m.root)], lf, lb
    out, gx, (gb, ga, gr), lf, lb = step()
    _assert_route(lf, fwd, 'forward')
    _assert_route(lb, bwd, 'backward')
    if fwd == 'Y':
        assert R % relations_per_segment(N, d_out) != 0                 # the last segment is partial
        assert m.graph_for(N, ei, rg).dest_fwd is None
    assert 'pair_' not in lf + lb and 'rel_gather' not in lf + lb and 'rel_stream' not in lf + lb, (lf, lb)

    basis, att, root = (p.detach().double().cpu() for p in (m.basis, m.att, m.root))
    x64 = x_c.double()
    want, saved = O.rgcn_fwd(x64, ei_c, rg_c, basis, att, root)
    g_out = up_c.double()
    if fuse_relu:
        g_out = torch.where(want > 0, g_out, torch.zeros_like(g_out))
        want = torch.relu(want)
    wx, wb, wa, wr = O.rgcn_bwd(g_out, x64, ei_c, basis, att, root, saved)
    _close(out, want, 1e-5)
    for got, w in ((gx, wx), (gb, wb), (ga, wa), (gr, wr)):
        _close(got, w, 1e-4)
    if inf_up:
        assert not bool(torch.isfinite(wa).all()) and int(torch.isfinite(wa).all(1).sum()) > R // 2
    out2, gx2, grads2, _, _ = step()                                    # second forward + backward: the same bits
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(gx), _bits(gx2))
    for a_, b_ in zip((gb, ga, gr), grads2):
        assert torch.equal(_bits(a_), _bits(b_))


@pytest.mark.timeout(90)
@pytest.mark.parametrize('N,R,d_in,d_out,nb,fwd,bwd', [
    (8192, 70, 128, 128, 32, 'rows_s', 'rows_s'),                     # large_kgroup path (32 bases)
    (8192, 100, 64, 64, 5, 'rows_s', 'rows_s'),
    (8192, 200, 32, 32, 32, 'rows', 'rows'),
    (8192, 70, 96, 96, 17, 'rows', 'rows'),                           # table padded to a 64-float stride
    (8192, 100, 32, 64, 8, 'dest', 'rows_s'),
    (8192, 130, 48, 48, 8, 'dest', 'csr'),
    (8192, 130, 40, 50, 8, 'dest', 'gather_sum'),                     # d_out % 4 != 0: no CSR rows
    (8192, 70, 40, 252, 8, 'dest', 'csr'),                            # the widest CSR rows (d_out <= 256)
    (65536, 40, 32, 32, 8, 'rows', 'rows'),                           # per-lane form at its 16-bit node limit
    (65537, 40, 32, 32, 8, 'dest', 'csr'),                            # one node past it
])
def test_large_route_matrix_vs_fp64(N, R, d_in, d_out, nb, fwd, bwd):
    _run_case(N, R, d_in, d_out, nb, fwd, bwd, seed=N + R + d_in + d_out)


@pytest.mark.timeout(90)
def test_large_route_y_segmented_gather_vs_fp64(monkeypatch):
    """The forward pass through Y with the segmented gather plan (dest_products switched off), last segment partial."""
    monkeypatch.setenv('TIPK_NO_DEST_FWD', '1')
    _run_case(8192, 130, 48, 48, 8, 'Y', 'csr', seed=7)


@pytest.mark.timeout(90)
def test_large_route_rows_s_fused_relu_vs_fp64():
    _run_case(8192, 100, 64, 64, 5, 'rows_s', 'rows_s', seed=11, fuse_relu=True)


@pytest.mark.timeout(90)
@pytest.mark.parametrize('N,R,d_in,d_out,nb,fwd,bwd', [(8192, 100, 64, 64, 5, 'rows_s', 'rows_s'), (8192, 200, 32, 32, 8, 'rows', 'rows')])
def test_large_route_inf_upstream_vs_fp64(N, R, d_in, d_out, nb, fwd, bwd):
    """An Inf row in `up`: exactly the gradient elements whose fp64 value is non-finite are non-finite (the row sums of the
    backward pass carry it into no other row), the rest match."""
    _run_case(N, R, d_in, d_out, nb, fwd, bwd, seed=13, inf_up=True)


@pytest.mark.timeout(90)
def test_large_route_past_the_widest_gather_is_an_error():
    """40 -> 260: past the CSR rows' 256 floats, no multiple of 32, and past `gather_sum`'s 256: the forward pass (dest) is
    correct and the backward pass raises -- there is no kernel for it, and no quiet fall-back."""
    from tip_amd._lib import TipkError
    from tip_amd.layers import MyRGCNConv2
    N, R = 8192, 70
    ei_c, et_c, rg_c = _graph(N, R, 3)
    torch.manual_seed(3)
    m = MyRGCNConv2(40, 260, R, 8, after_relu=False).to(DEV)
    x_c = torch.randn(N, 40, generator=torch.Generator().manual_seed(4))
    x = x_c.to(DEV).requires_grad_(True)
    out, lf = _labels(lambda: m(x, ei_c.to(DEV), et_c.to(DEV), rg_c.to(DEV)))
    _assert_route(lf, 'dest', 'forward')
    want, _ = O.rgcn_fwd(x_c.double(), ei_c, rg_c, *(p.detach().double().cpu() for p in (m.basis, m.att, m.root)))
    _close(out, want, 1e-5)
    with pytest.raises(TipkError, match='unsupported'):
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
