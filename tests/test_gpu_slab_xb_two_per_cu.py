"""-m gpu: the hand-over kernel between the two R-GCN layers (`tipk_sum_slabs_xb`, tip_amd/csrc/tipk_slab_xb.hip) after it was
brought under 64 VGPRs: the weights of an output column come as two halves of 16, the first requested before the slabs, and
d_out = 16 / 32 are compile-time strides (any other d_out walks one offset register).

    x1     bit-equal to `ops.sum_slabs` on the same slabs (same 16 slab lanes, lane order, k order, same epilogue; below 32
           slabs `sum_slabs` would pick 4 lanes, so there it gets the slabs padded with zeros: `sixteen_lane_form`);
    XB2, x1 root2   against fp64 products of the x1 the kernel wrote, within the bound tests/test_gpu_kernels.py holds the
                    kernel to: rtol 2e-5, atol 2e-5 max|want|;
    columns at or beyond d_out of the XB rows, and rows beyond n_rows, keep their sentinel; a second launch repeats the bits.

n_rows 1, 2, 5 (odd: the last workgroup owns one row), 1 / 15 / 16 / 17 / 81 slabs (fewer slabs than slab lanes, one per lane,
one lane with two, the four-in-flight loop with a tail), relu on / off, with / without addend and row_scale.  n_bases = 32
with d_out = 32 is 1 056 output columns: 32 threads take a second column, whose weights cannot be requested ahead.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 7.0


@pytest.fixture(scope='module')
def ops():
    from tip_amd import ops as o
    return o


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def close(got, want, rtol, atol):
    torch.testing.assert_close(got.detach().cpu().double(), want, rtol=rtol, atol=atol)


def sixteen_lane_form(slabs):
    """The same slabs in the form `ops.sum_slabs` adds with 16 slab lanes, as the hand-over kernel always does: from 32 slabs on
    it takes them as they are; below that it would take 4 lanes (another order of the same additions), so zero slabs are
    appended up to 32 -- lane j still adds slabs j, j + 16, ... in order and a trailing + 0 changes no bit of a sum that
    started from + 0."""
    s = slabs.shape[0]
    if s >= 32:
        return slabs
    return torch.cat([slabs, torch.zeros((32 - s,) + tuple(slabs.shape[1:]), device=slabs.device)], 0).contiguous()


@pytest.mark.parametrize('n_bases', [32, 3])
@pytest.mark.parametrize('d_out', [16, 32, 24])
@pytest.mark.parametrize('n_rows', [1, 2, 5])
def test_hand_over_at_row_slab_and_width_edges(ops, n_rows, d_out, n_bases):
    g = torch.Generator().manual_seed(n_rows * 100 + d_out + n_bases)
    basis = torch.randn(n_bases, 32, d_out, generator=g).to(DEV)
    root = torch.randn(32, d_out, generator=g).to(DEV)
    scale = (torch.rand(n_rows, generator=g) + 0.5).to(DEV)
    addend = torch.randn(n_rows, 32, generator=g).to(DEV)
    n_pad = -(-n_rows // 8) * 8
    for n_slabs in (1, 15, 16, 17, 81):
        slabs = torch.randn(n_slabs, n_rows, 32, generator=g).to(DEV)
        for relu in (True, False):
            for rs, ad in ((scale, addend), (None, None), (scale, None), (None, addend)):
                what = 'rows=%d slabs=%d d_out=%d bases=%d relu=%s scale=%s addend=%s' % (
                    n_rows, n_slabs, d_out, n_bases, relu, rs is not None, ad is not None)
                xb = torch.full((n_pad, n_bases, 32), SENTINEL, device=DEV)
                x = torch.full((n_rows, 32), float('nan'), device=DEV)
                xroot = ops.sum_slabs_xb(slabs, rs, ad, relu, x, basis, root, xb)
                want_x = ops.sum_slabs(sixteen_lane_form(slabs), row_scale=rs, addend=ad, relu=relu)
                assert torch.equal(bits(x), bits(want_x)), what + ': x1 differs from sum_slabs'
                x64 = x.double().cpu()
                want_r = x64 @ root.double().cpu()
                want_b = torch.einsum('ni,bio->nbo', x64, basis.double().cpu())
                close(xroot, want_r, rtol=2e-5, atol=2e-5 * float(want_r.abs().max()))
                close(xb[:n_rows, :, :d_out], want_b, rtol=2e-5, atol=2e-5 * float(want_b.abs().max()))
                assert bool((xb[:n_rows, :, d_out:] == SENTINEL).all()) and bool((xb[n_rows:] == SENTINEL).all()), what
                xb2 = torch.full((n_pad, n_bases, 32), SENTINEL, device=DEV)
                x2 = torch.empty(n_rows, 32, device=DEV)
                xroot2 = ops.sum_slabs_xb(slabs, rs, ad, relu, x2, basis, root, xb2)
                assert torch.equal(bits(xroot2), bits(xroot)) and torch.equal(bits(xb2), bits(xb)) and torch.equal(bits(x2), bits(x)), what


def test_hand_over_products_are_exact_on_integers(ops):
    """Integers: every product and every sum is exact in any order -- XB2 and x1 root2 equal the fp64 products bit for bit, at the
    step's shape (more than one round of workgroups at one per CU: 323 of them)."""
    g = torch.Generator().manual_seed(5)
    n_rows, n_slabs, n_bases, d_out = 645, 17, 32, 16
    slabs = torch.randint(-3, 4, (n_slabs, n_rows, 32), generator=g).float().to(DEV)
    addend = torch.randint(-3, 4, (n_rows, 32), generator=g).float().to(DEV)
    basis = torch.randint(-3, 4, (n_bases, 32, d_out), generator=g).float().to(DEV)
    root = torch.randint(-3, 4, (32, d_out), generator=g).float().to(DEV)
    xb = torch.full((648, n_bases, 32), SENTINEL, device=DEV)
    x = torch.empty(n_rows, 32, device=DEV)
    xroot = ops.sum_slabs_xb(slabs, None, addend, True, x, basis, root, xb)
    x64 = torch.relu(slabs.double().sum(0) + addend.double()).cpu()
    assert torch.equal(x.double().cpu(), x64)
    assert torch.equal(xroot.double().cpu(), x64 @ root.double().cpu())
    assert torch.equal(xb[:n_rows, :, :d_out].double().cpu(), torch.einsum('ni,bio->nbo', x64, basis.double().cpu()))
    assert bool((xb[:n_rows, :, d_out:] == SENTINEL).all()) and bool((xb[n_rows:] == SENTINEL).all())
