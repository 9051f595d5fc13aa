#!/usr/bin/env python3
"""A host that is NOT the tip_amd package: the whole FMEncoder forward + backward through the encoder entries of the C ABI.

    python examples/c_abi_encoder_host.py [fixture.npz ...]   (default: tests/golden/encoder_fast_{cat_sym,add_sym,cat_directed}.npz)

What a maintainer of the reference would write to route `FMEncoder.forward` (src/layers.py:520-550) and its autograd to
libtipk.so from any language with a C FFI (include/tipk.h section 10d): `tipk_encoder_build` once with the three graphs as the
reference holds them, a workspace of `tipk_encoder_workspace_bytes` prepared by `tipk_encoder_workspace_init`, then `tipk_encoder_fwd` / `tipk_encoder_bwd` per
step, `tipk_encoder_destroy` at the end.  The parameters are the reference's state_dict tensors as they are (row-major GCN
weights: lin_layout 0).  Only ctypes + torch-for-device-memory are used: no module of the package is imported (asserted at the
end).  The fixtures are outputs and autograd gradients of the reference's own FMEncoder (oracle/make_golden.py).

tests/golden/tip_add_small.npz (3 bases, 8-wide layers) is outside what the fused kernels take: the handle must refuse it with
TIPK_EUNSUPPORTED -- there is no other route behind it.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L = C.c_void_p, C.c_int, C.c_int64
TIPK_EUNSUPPORTED = -2
FROM_FWD = 1
NAMES = ('embed', 'pp_w1', 'pp_b1', 'pp_w2', 'pp_b2', 'hgcn_w', 'basis1', 'att1', 'root1', 'basis2', 'att2', 'root2')
STATE = ('embed', 'pp_encoder.conv1.lin.weight', 'pp_encoder.conv1.bias', 'pp_encoder.conv2.lin.weight', 'pp_encoder.conv2.bias',
         'hgcn.weight', 'rgcn1.basis', 'rgcn1.att', 'rgcn1.root', 'rgcn2.basis', 'rgcn2.att', 'rgcn2.root')


class Dims(C.Structure):
    _fields_ = [('n_embed', I), ('prot_drug_dim', I), ('n_hid1', I), ('n_hid2', I), ('num_base', I), ('cat', I)]


class Params(C.Structure):
    _fields_ = [(k, P) for k in NAMES] + [('lin_layout', I)]


class Grads(C.Structure):
    _fields_ = [(k, P) for k in NAMES]


def load_library():
    lib = C.CDLL(os.path.join(ROOT, 'tip_amd', 'libtipk.so'))
    lib.tipk_encoder_build.restype = I
    lib.tipk_encoder_build.argtypes = [P, L, P, L, P, L, P, L, I, L, L, P, C.POINTER(P)]
    lib.tipk_encoder_workspace_bytes.restype = L
    lib.tipk_encoder_workspace_bytes.argtypes = [P]
    lib.tipk_encoder_workspace_init.restype = I
    lib.tipk_encoder_workspace_init.argtypes = [P, P, L, P]
    lib.tipk_encoder_fwd.restype = I
    lib.tipk_encoder_fwd.argtypes = [P, P, P, L, P, P, L, P, L, P]
    lib.tipk_encoder_bwd.restype = I
    lib.tipk_encoder_bwd.argtypes = [P, P, P, L, P, P, L, P, P, L, I, P, L, P]
    lib.tipk_encoder_destroy.restype = I
    lib.tipk_encoder_destroy.argtypes = [P]
    return lib


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream_of(dev):
    return P(torch.cuda.current_stream(dev).cuda_stream)


class Encoder(object):
    """One handle + its workspace.  graphs: pp [2, E], dp [2, E], dd [2, E], dd_range [R, 2] (any integer type, any device),
    handed over as int64 (idx_bytes 8) or int32 (idx_bytes 4)."""

    def __init__(self, lib, pp, dp, dd, dd_range, n_prot, n_drug, dims, dev, idx_bytes=8):
        self.lib, self.dev, self.n_drug, self.dims = lib, dev, n_drug, dims
        self.h = P()
        keep = [t.to(dev).to(torch.int64 if idx_bytes == 8 else torch.int32).contiguous() for t in (pp, dp, dd, dd_range)]
        self.status = lib.tipk_encoder_build(ptr(keep[0]), keep[0].shape[1], ptr(keep[1]), keep[1].shape[1], ptr(keep[2]), keep[2].shape[1],
                                             ptr(keep[3]), keep[3].shape[0], idx_bytes, n_prot, n_drug, C.byref(dims), C.byref(self.h))
        if self.status == 0:
            self.ws = torch.empty(lib.tipk_encoder_workspace_bytes(self.h), dtype=torch.uint8, device=dev)
            assert lib.tipk_encoder_workspace_init(self.h, ptr(self.ws), self.ws.numel(), stream_of(dev)) == 0

    def params(self, tensors, layout):
        p = Params(*[ptr(tensors[k]) for k in NAMES], layout)
        return p

    def forward(self, p, d_norm, z, stream=None):
        return self.lib.tipk_encoder_fwd(self.h, C.byref(p), None, 0, ptr(d_norm), ptr(z), z.shape[1], ptr(self.ws), self.ws.numel(),
                                         stream if stream is not None else stream_of(self.dev))

    def backward(self, p, d_norm, gz, grads, flags=FROM_FWD, stream=None):
        g = Grads(*[ptr(grads[k]) for k in NAMES])
        return self.lib.tipk_encoder_bwd(self.h, C.byref(p), None, 0, ptr(d_norm), ptr(gz), gz.shape[1], C.byref(g), None, 0, flags,
                                         ptr(self.ws), self.ws.numel(), stream if stream is not None else stream_of(self.dev))

    def close(self):
        if self.h:
            assert self.lib.tipk_encoder_destroy(self.h) == 0
            self.h = P()


def check_golden(lib, path, dev):
    z_ = np.load(path)
    g = {k: z_[k] for k in z_.files}
    cfg = {k[4:]: int(v) for k, v in g.items() if k.startswith('cfg.')}
    mod = str(g['mod'])
    dims = Dims(cfg['n_embed'], cfg['prot_drug_dim'], cfg['n_hid1'], cfg['n_hid2'], cfg['num_base'], int(mod == 'cat'))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n_drug, n_prot = int(g['n_drug']), int(g['n_prot'])
    enc = Encoder(lib, t(g['pp_idx']), t(g['dp_idx']), t(g['dd_idx']), t(g['dd_range']), n_prot, n_drug, dims, dev)
    assert enc.status == 0, 'tipk_encoder_build: %d' % enc.status
    try:
        prm = {k: t(g[s]).to(dev).float().contiguous() for k, s in zip(NAMES, STATE)}
        p = enc.params(prm, 0)
        d_norm = t(g['d_norm']).to(dev).float()
        z = torch.empty(n_drug, cfg['n_hid2'], device=dev)
        assert enc.forward(p, d_norm, z) == 0
        grads = {k: torch.empty_like(v) for k, v in prm.items()}
        assert enc.backward(p, d_norm, t(g['upstream']).to(dev).float(), grads) == 0
        torch.cuda.synchronize(dev)
        want = t(g['z'])
        worst = float((z.cpu() - want).abs().max() / want.abs().max())
        torch.testing.assert_close(z.cpu(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
        for k, s in zip(NAMES, STATE):
            ref = t(g['grad.' + s])
            torch.testing.assert_close(grads[k].cpu(), ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))
            worst = max(worst, float((grads[k].cpu() - ref).abs().max() / max(1e-30, float(ref.abs().max()))))
        return worst
    finally:
        enc.close()


def check_refused(lib, path, dev):
    """A shape the fused kernels do not take: TIPK_EUNSUPPORTED, no handle."""
    z_ = np.load(path)
    pre = 'encoder.'
    nb, d_in, d1 = z_[pre + 'rgcn1.basis'].shape
    d2 = z_[pre + 'rgcn2.basis'].shape[2]
    ne, q = z_[pre + 'embed'].shape[1], z_[pre + 'hgcn.weight'].shape[1]
    dims = Dims(int(ne), int(q), int(d1), int(d2), int(nb), int(d_in == ne + q))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    enc = Encoder(lib, t(z_['pp_train_indices']), t(z_['dp_edge_index']), t(z_['dd_train_idx']), t(z_['dd_train_range']),
                  int(z_['n_prot']), int(z_['n_drug']), dims, dev)
    assert enc.status == TIPK_EUNSUPPORTED and not enc.h.value, enc.status
    return enc.status


def main():
    dev = torch.device('cuda:0')
    lib = load_library()
    gold = os.path.join(ROOT, 'tests', 'golden')
    paths = sys.argv[1:] or [os.path.join(gold, 'encoder_fast_%s.npz' % n) for n in ('cat_sym', 'add_sym', 'cat_directed')]
    for path in paths:
        print('%-28s max error %.2e of max|want|' % (os.path.basename(path), check_golden(lib, path, dev)))
    if not sys.argv[1:]:
        st = check_refused(lib, os.path.join(gold, 'tip_add_small.npz'), dev)
        print('%-28s refused with %d (TIPK_EUNSUPPORTED: 3 bases, 8-wide layers)' % ('tip_add_small.npz', st))
    assert not any(m == 'tip_amd' or m.startswith('tip_amd.') for m in sys.modules), 'the host imported the package'
    print('C-ABI encoder ok')


if __name__ == '__main__':
    main()
