"""The whole-encoder entries of the C ABI (include/tipk.h section 10d) on the device: bit-identical to the Python schedule
(tip_amd/encoder.py `_EncoderStep`) at BioSNAP size, against the reference's goldens, recompute-safe, capturable, independent
per handle, and a host that is not the package."""
import os
import subprocess
import sys

import pytest
import torch

from tip_amd import encoder
from tip_amd.data import Data, build_data_dict
from tip_amd.layers import FMEncoder
from tip_amd.utils import sparse_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import c_abi_encoder_host as host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def biosnap():
    dd = build_data_dict()
    return dd, Data.from_dict(dd).to(DEV)


@pytest.fixture(scope='module')
def lib():
    return host.load_library()


def _dims(mod):
    return dict(prot_drug_dim=16, n_embed=48) if mod == 'cat' else dict(prot_drug_dim=64, n_embed=64)


def _module(dd, mod, seed=3):
    torch.manual_seed(seed)
    enc = FMEncoder(DEV, dd['n_drug'], dd['n_dd_et'], dd['n_prot'], dd['n_prot'], dd['n_drug'], num_base=32, n_hid1=32, n_hid2=16,
                    mod=mod, **_dims(mod)).to(DEV)
    for p in enc.parameters():                                  # visible magnitudes everywhere
        p.data.add_(0.01 * torch.randn_like(p))
    return enc


def _handle(lib, dd, d, mod, n_hid2=16):
    dm = _dims(mod)
    dims = host.Dims(dm['n_embed'], dm['prot_drug_dim'], 32, n_hid2, 32, int(mod == 'cat'))
    return host.Encoder(lib, d.pp_train_indices, d.dp_edge_index, d.dd_train_idx, d.dd_train_range, dd['n_prot'], dd['n_drug'], dims, DEV)


def _state(enc):
    """the 12 tensors as the module holds them (GCN weights stored [in, out]: lin_layout 1)."""
    sd = dict(enc.named_parameters())
    return {k: sd[s].detach() for k, s in zip(host.NAMES, host.STATE)}


def _python_step(enc, d, up):
    enc.zero_grad()
    args = (sparse_id(d.n_drug).to(DEV), d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, sparse_id(d.n_prot).to(DEV),
            d.pp_train_indices, d.dp_edge_index, None)
    z = enc(*args)
    assert enc.last_route == 'encoder_step'
    z.backward(up)
    grads = dict(enc.named_parameters())
    return z.detach(), {k: grads[s].grad.clone() for k, s in zip(host.NAMES, host.STATE)}


def _c_step(h, prm, layout, d_norm, up, flags=host.FROM_FWD, z=None, grads=None):
    p = h.params(prm, layout)
    z = torch.empty(up.shape, device=DEV) if z is None else z
    grads = {k: torch.empty_strided(v.shape, v.stride(), device=DEV) for k, v in prm.items()} if grads is None else grads
    assert h.forward(p, d_norm, z) == 0
    assert h.backward(p, d_norm, up, grads, flags) == 0
    return z, grads


@pytest.mark.parametrize('mod', ['cat', 'add'])
def test_bitwise_equal_to_the_python_schedule_at_biosnap_size(biosnap, lib, mod):
    """The C entry against `_EncoderStep` on the same graphs, parameters and upstream gradient: the same bits for z and all 12
    gradients (d embed is the gradient of the identity drug features).  The reference's row-major GCN weights (lin_layout 0) give
    the same bits as the transposed storage (lin_layout 1)."""
    dd, d = biosnap
    enc = _module(dd, mod)
    xd, plans = enc.fused_plans(sparse_id(d.n_drug).to(DEV), d.dd_train_idx, d.dd_train_range, d.d_norm, sparse_id(d.n_prot).to(DEV),
                                d.pp_train_indices, d.dp_edge_index)
    assert encoder.usable(plans, xd, enc.hgcn.weight, d.d_norm, enc.pp_encoder.conv2.lin.weight, enc.pp_encoder.conv1.bias,
                          enc.pp_encoder.conv2.bias, enc.rgcn1.basis, enc.rgcn1.att, enc.rgcn2.basis, enc.rgcn2.att)
    up = torch.randn(dd['n_drug'], 16, device=DEV)
    z_py, g_py = _python_step(enc, d, up)
    h = _handle(lib, dd, d, mod)
    assert h.status == 0
    try:
        for layout in (1, 0):
            prm = _state(enc) if layout else {k: v.contiguous() for k, v in _state(enc).items()}
            z, grads = _c_step(h, prm, layout, d.d_norm, up)
            torch.cuda.synchronize()
            assert torch.equal(z, z_py), layout
            for k in host.NAMES:
                assert torch.equal(grads[k], g_py[k]), (layout, k)
    finally:
        h.close()


def test_training_objective_through_the_handle(biosnap, lib):
    """TIP's training step with the DistMult objective (src/layers.py:335-340) on the fused shapes: encoder forward through
    `tipk_encoder_fwd`, the fused objective (`tipk_distmult_loss`) on its output, `tipk_encoder_bwd` from d z -- the loss, the
    decoder's gradient and all 12 encoder gradients bit for bit as the PyTorch modules' autograd gives them."""
    from tip_amd.layers import MultiInnerProductDecoder
    dd, d = biosnap
    enc = _module(dd, 'cat', seed=11)
    dec = MultiInnerProductDecoder(16, dd['n_dd_et']).to(DEV)
    # random negative pairs, one per positive (the objective takes any; the package's sampler keeps a process-wide cache of
    # positive-key tables that other tests warm up, so this test leaves it alone)
    gen = torch.Generator(device=DEV).manual_seed(7)
    neg = torch.randint(0, dd['n_drug'], tuple(d.dd_train_idx.shape), generator=gen, device=DEV)
    enc.zero_grad()
    z = enc(sparse_id(d.n_drug).to(DEV), d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, sparse_id(d.n_prot).to(DEV),
            d.pp_train_indices, d.dp_edge_index, None)
    assert enc.last_route == 'encoder_step'
    loss_py = dec.objective(z, d.dd_train_idx, neg, d.dd_train_et)
    loss_py.backward()
    g_py = {k: p.grad.clone() for k, p in zip(host.NAMES, [dict(enc.named_parameters())[s] for s in host.STATE])}
    g_dec_py = dec.weight.grad.clone()
    dec.zero_grad()
    h = _handle(lib, dd, d, 'cat')
    assert h.status == 0
    try:
        prm = _state(enc)
        p = h.params(prm, 1)
        z_c = torch.empty(dd['n_drug'], 16, device=DEV)
        assert h.forward(p, d.d_norm, z_c) == 0
        z_leaf = z_c.clone().requires_grad_(True)
        loss_c = dec.objective(z_leaf, d.dd_train_idx, neg, d.dd_train_et)
        loss_c.backward()
        grads = {k: torch.empty_strided(v.shape, v.stride(), device=DEV) for k, v in prm.items()}
        assert h.backward(p, d.d_norm, z_leaf.grad.contiguous(), grads) == 0
        torch.cuda.synchronize()
        assert torch.equal(loss_c.detach(), loss_py.detach())
        assert torch.equal(dec.weight.grad, g_dec_py)
        for k in host.NAMES:
            assert torch.equal(grads[k], g_py[k]), k
    finally:
        h.close()


@pytest.mark.parametrize('name', ['encoder_fast_cat_sym', 'encoder_fast_add_sym', 'encoder_fast_cat_directed'])
def test_against_reference_goldens(lib, name):
    host.check_golden(lib, os.path.join(ROOT, 'tests', 'golden', name + '.npz'), DEV)


def test_backward_without_from_fwd_recomputes_the_same_bits(biosnap, lib):
    """flags 0: the backward pass forms XB and the pair cells of both layers again from the parameters it is given (what
    `_EncoderStep.backward` does when another forward pass rewrote the graph's buffers) -- the same bits as the buffers the forward
    pass left.  The forward pass of OTHER parameters in between rewrites those buffers; the right forward pass then restores the
    activations, and the flags-0 backward pass must not depend on which parameters last touched the cells."""
    dd, d = biosnap
    h = _handle(lib, dd, d, 'cat')
    assert h.status == 0
    try:
        right = {k: v.contiguous() for k, v in _state(_module(dd, 'cat', seed=5)).items()}
        other = {k: v.contiguous() for k, v in _state(_module(dd, 'cat', seed=6)).items()}
        up = torch.randn(dd['n_drug'], 16, device=DEV)
        z_ref, g_ref = _c_step(h, right, 0, d.d_norm, up)
        for first in (other, right):
            z = torch.empty_like(z_ref)
            assert h.forward(h.params(first, 0), d.d_norm, z) == 0
            assert h.forward(h.params(right, 0), d.d_norm, z) == 0
            grads = {k: torch.empty_like(v) for k, v in right.items()}
            assert h.backward(h.params(right, 0), d.d_norm, up, grads, 0) == 0
            torch.cuda.synchronize()
            assert torch.equal(z, z_ref)
            for k in host.NAMES:
                assert torch.equal(grads[k], g_ref[k]), k
    finally:
        h.close()


def test_graph_capture_replays_the_same_bits(biosnap, lib):
    dd, d = biosnap
    h = _handle(lib, dd, d, 'cat')
    assert h.status == 0
    try:
        prm = _state(_module(dd, 'cat'))
        up = torch.randn(dd['n_drug'], 16, device=DEV)
        z_e, g_e = _c_step(h, prm, 1, d.d_norm, up)
        z_e2, g_e2 = _c_step(h, prm, 1, d.d_norm, up)
        torch.cuda.synchronize()
        assert torch.equal(z_e, z_e2) and all(torch.equal(g_e[k], g_e2[k]) for k in host.NAMES)
        z = torch.empty_like(z_e)
        grads = {k: torch.empty_like(v) for k, v in g_e.items()}
        p = h.params(prm, 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            graph.capture_begin()
            st = host.P(s.cuda_stream)
            rc = (h.forward(p, d.d_norm, z, st), h.backward(p, d.d_norm, up, grads, host.FROM_FWD, st))
            graph.capture_end()
        assert rc == (0, 0)
        for _ in range(3):
            z.zero_()
            for v in grads.values():
                v.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(z, z_e)
            for k in host.NAMES:
                assert torch.equal(grads[k], g_e[k]), k
    finally:
        h.close()


def test_two_handles_on_two_streams(biosnap, lib):
    dd, d = biosnap
    enc = _module(dd, 'cat')
    prm = _state(enc)
    prm8 = dict(prm)                                            # (a second layer width: 32 columns)
    torch.manual_seed(9)
    prm8['basis2'] = torch.randn(32, 32, 32, device=DEV) * 0.1
    prm8['root2'] = torch.randn(32, 32, device=DEV) * 0.1
    h16, h8 = _handle(lib, dd, d, 'cat', 16), _handle(lib, dd, d, 'cat', 32)
    assert h16.status == 0 and h8.status == 0
    try:
        up16, up8 = torch.randn(dd['n_drug'], 16, device=DEV), torch.randn(dd['n_drug'], 32, device=DEV)
        want16, want8 = _c_step(h16, prm, 1, d.d_norm, up16), _c_step(h8, prm8, 1, d.d_norm, up8)
        torch.cuda.synchronize()
        outs = []
        streams = (torch.cuda.Stream(), torch.cuda.Stream())
        for _ in range(2):
            for h, pr, up, s in ((h16, prm, up16, streams[0]), (h8, prm8, up8, streams[1])):
                z = torch.empty(up.shape, device=DEV)
                grads = {k: torch.empty_strided(v.shape, v.stride(), device=DEV) for k, v in pr.items()}
                p = h.params(pr, 1)
                st = host.P(s.cuda_stream)
                s.wait_stream(torch.cuda.current_stream())
                assert h.forward(p, d.d_norm, z, st) == 0
                assert h.backward(p, d.d_norm, up, grads, host.FROM_FWD, st) == 0
                outs.append((z, grads))
        torch.cuda.synchronize()
        for i, (z, grads) in enumerate(outs):
            wz, wg = want16 if i % 2 == 0 else want8
            assert torch.equal(z, wz)
            for k in host.NAMES:
                assert torch.equal(grads[k], wg[k]), k
    finally:
        h16.close()
        h8.close()


def test_unsupported_shape_leaves_outputs_untouched(biosnap, lib):
    dd, d = biosnap
    dims = host.Dims(48, 16, 48, 16, 32, 1)                                     # n_hid1 = 48: no fused kernel
    h = host.P()
    keep = [t.to(torch.int64).contiguous() for t in (d.pp_train_indices, d.dp_edge_index, d.dd_train_idx, d.dd_train_range)]
    import ctypes as C
    st = lib.tipk_encoder_build(keep[0].data_ptr(), keep[0].shape[1], keep[1].data_ptr(), keep[1].shape[1], keep[2].data_ptr(),
                                keep[2].shape[1], keep[3].data_ptr(), keep[3].shape[0], 8, dd['n_prot'], dd['n_drug'], C.byref(dims),
                                C.byref(h))
    assert st == host.TIPK_EUNSUPPORTED and not h.value
    # a handle that exists, called with what it does not take (dense drug features): refused before any launch
    good = _handle(lib, dd, d, 'cat')
    assert good.status == 0
    try:
        prm = _state(_module(dd, 'cat'))
        z = torch.full((dd['n_drug'], 16), 7.0, device=DEV)
        xd = torch.randn(dd['n_drug'], 10, device=DEV)
        p = good.params(prm, 1)
        rc = lib.tipk_encoder_fwd(good.h, C.byref(p), xd.data_ptr(), 10, d.d_norm.data_ptr(), z.data_ptr(), 16, good.ws.data_ptr(),
                                  good.ws.numel(), host.stream_of(DEV))
        torch.cuda.synchronize()
        assert rc == host.TIPK_EUNSUPPORTED
        assert bool((z == 7.0).all())
    finally:
        good.close()


def test_host_that_is_not_the_package():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'c_abi_encoder_host.py')], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'C-ABI encoder ok' in out.stdout
