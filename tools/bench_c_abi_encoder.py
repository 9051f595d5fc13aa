"""The whole encoder through the encoder entries of the C ABI (include/tipk.h section 10d) at BioSNAP size: FMEncoder (cat,
64 -> 32 -> 16, 32 bases, R = 1 097) forward + backward as `tipk_encoder_fwd` + `tipk_encoder_bwd`, captured into one hipGraph
and replayed -- next to the same steps stitched from the per-layer entries (tools/bench_c_abi.py `whole_encoder`).

    python tools/bench_c_abi_encoder.py [--steps 50]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import c_abi_encoder_host as host                              # noqa: E402  (ctypes signatures + the handle wrapper)
from tip_amd.data import build_data_dict                        # noqa: E402  (the synthetic BioSNAP-shaped graph only)

LAUNCHES = 16                                                   # encoder.py: 8 forward + 8 backward (lin_layout 1)


def encoder_entry(lib, dd, dev, steps):
    n_d, n_p, r = dd['n_drug'], dd['n_prot'], dd['n_dd_et']
    dims = host.Dims(48, 16, 32, 16, 32, 1)
    t0 = time.perf_counter()
    enc = host.Encoder(lib, dd['pp_train_indices'], dd['dp_edge_index'], dd['dd_train_idx'], dd['dd_train_range'], n_p, n_d, dims, dev)
    build_s = time.perf_counter() - t0
    assert enc.status == 0, enc.status
    torch.manual_seed(1)
    mk = lambda *s: (torch.randn(*s, device=dev) * 0.1).contiguous()
    prm = {'embed': mk(n_d, 48), 'pp_w1': mk(n_p, 32).t(), 'pp_b1': mk(32), 'pp_w2': mk(32, 16).t(), 'pp_b2': mk(16), 'hgcn_w': mk(16, 16),
           'basis1': mk(32, 64, 32), 'att1': mk(r, 32), 'root1': mk(64, 32), 'basis2': mk(32, 32, 16), 'att2': mk(r, 32), 'root2': mk(32, 16)}
    grads = {k: torch.empty_strided(v.shape, v.stride(), device=dev) for k, v in prm.items()}
    p = enc.params(prm, 1)                                      # GCN weights stored [in, out]: the 16-launch schedule
    d_norm = torch.ones(n_d, device=dev)
    z, gz = torch.empty(n_d, 16, device=dev), mk(n_d, 16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st = C.c_void_p(s.cuda_stream)

        def step():
            assert enc.forward(p, d_norm, z, st) == 0
            assert enc.backward(p, d_norm, gz, grads, host.FROM_FWD, st) == 0
        for _ in range(3):
            step()
        s.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            step()
    for _ in range(5):
        gr.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gr.replay()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert bool(torch.isfinite(z).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    del gr
    enc.close()
    return {'ms_per_step': ms, 'launches': LAUNCHES, 'encoder_build_s': build_s,
            'what': 'FMEncoder (cat) forward + backward, tipk_encoder_fwd + tipk_encoder_bwd, hipGraph replay'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = host.load_library()
    dd = build_data_dict()
    rec = {'workload': 'FMEncoder 64 -> 32 -> 16, 32 bases, N = %d, R = %d' % (dd['n_drug'], dd['n_dd_et'])}
    rec['encoder_entry'] = encoder_entry(lib, dd, dev, args.steps)
    # the same step stitched from the per-layer entries
    import bench_c_abi
    plib = bench_c_abi.host.load_library()
    ei, rg = dd['dd_train_idx'].to(dev), dd['dd_train_range'].to(dev)
    gd = bench_c_abi.host.build_graph(plib, ei, None, rg, dd['n_drug'], dd['n_dd_et'])
    rec['per_layer_entries'] = bench_c_abi.whole_encoder(plib, dd, gd, dev, args.steps)
    rec['ms_per_step'] = rec['encoder_entry']['ms_per_step']
    rec['launches'] = LAUNCHES
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
