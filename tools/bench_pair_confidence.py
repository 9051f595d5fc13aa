"""Time the confidence top-k (`tipk_distmult_pair_conf_topk`, include/tipk.h section 4p) on the device, next to the torch
composition of the same question on the same GPU in the same run, and `TIP.decoder_posterior` for all side effects.

  python tools/bench_pair_confidence.py              the bundled BioSNAP graph (645 drugs, 1 097 relations, dim 16), k = 10,
                                                     P = 1, 64, 4 096 and 65 536 random pairs; the model's posterior at
                                                     l2 = 1e-4; both key modes; then `decoder_posterior` for all rows
  python tools/bench_pair_confidence.py --skip-baseline

The torch composition: phi = z[u] * z[v]; y = einsum('pj,rij->pri', phi, W); var = (y * y).sum(-1); s = phi @ w^T; key; a
masked `topk`.  Its [P, R, dim] temporary is 4.6 GB at P = 65 536, so it runs in chunks of `--chunk` pairs (default 8 192,
0.6 GB), which is said in the output line.

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`), triples/s and the
fraction of the fp32 matrix-core peak (157.3 TF) at 2 dim (dim + 1) FLOP per triple.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

PEAK_FP32 = 157.3e12
DEV = 'cuda:0'


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def torch_composition(z, w, w_log, pairs, k, mode, c, chunk):
    keys, rels = [], []
    for p0 in range(0, pairs.shape[1], chunk):
        u, v = pairs[0, p0:p0 + chunk], pairs[1, p0:p0 + chunk]
        phi = z[u] * z[v]
        y = torch.einsum('pj,rij->pri', phi, w_log)
        var = (y * y).sum(-1)
        s = phi @ w.t()
        key = s / torch.sqrt(1.0 + (math.pi / 8) * var) if mode == 0 else s + c * torch.sqrt(var)
        top = torch.topk(key, k, dim=1)
        keys.append(top.values)
        rels.append(top.indices)
    return torch.cat(keys), torch.cat(rels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--skip-baseline', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_pair_confidence times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting
    t = time.time()
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z = model.embeddings.detach()
    dim = z.shape[1]

    t0 = time.time()
    post = model.decoder_posterior()
    torch.cuda.synchronize()
    first = time.time() - t0
    t0 = time.time()
    post = model.decoder_posterior()
    torch.cuda.synchronize()
    print(json.dumps({'case': 'decoder_posterior_all_rows', 'rows': R, 'first_call_s': round(first, 3),
                      'second_call_s': round(time.time() - t0, 3)}), flush=True)
    fp = ops.fit_pairs_csr(model_pairs(model), n)
    ms = timed(lambda: ops.distmult_posterior(z, post.weight, fp, 1e-4), 3, 1)
    print(json.dumps({'case': 'ops_distmult_posterior_all_rows', 'rows': R, 'ms': round(ms, 3)}), flush=True)
    hess = ops.distmult_fit_stats(z, post.weight, fp, 1e-4)[2]
    scale = fp.n_pairs.double().rsqrt().float().to(DEV)
    ms = timed(lambda: ops.spd_factor(hess, scale), args.reps, args.warmup)
    print(json.dumps({'case': 'spd_factor_all_rows', 'rows': R, 'ms': round(ms, 4)}), flush=True)

    w, w_fac = post.weight, post.factor
    w_log = w_fac.transpose(1, 2).contiguous()
    known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n)
    g = torch.Generator().manual_seed(1)
    for P in (1, 64, 4096, 65536):
        pairs = torch.randint(0, n, (2, P), generator=g).to(DEV)
        flops = 2.0 * dim * (dim + 1) * P * R
        for name, mode, c, kn in (('moderated', 0, 0.0, None), ('lower_1.645', 1, -1.645, None), ('moderated_exclude_train', 0, 0.0, known)):
            ms = timed(lambda: ops.distmult_pair_conf_topk(z, w, w_fac, pairs, args.k, mode, c, kn), args.reps, args.warmup)
            print(json.dumps({'case': 'fused_%s' % name, 'pairs': P, 'k': args.k, 'ms': round(ms, 4),
                              'triples_per_s': P * R / (ms * 1e-3), 'fraction_of_fp32_mfma_peak': round(flops / PEAK_FP32 / (ms * 1e-3), 4)}),
                  flush=True)
        if not args.skip_baseline:
            ms = timed(lambda: torch_composition(z, w, w_log, pairs, args.k, 0, 0.0, args.chunk), max(1, args.reps // 3), 1)
            print(json.dumps({'case': 'torch_composition_moderated', 'pairs': P, 'k': args.k, 'ms': round(ms, 4),
                              'chunk': args.chunk, 'chunks': -(-P // args.chunk)}), flush=True)
    print(json.dumps({'wall_s': round(time.time() - t, 1)}), flush=True)


def model_pairs(model):
    from tip_amd.layers import _training_pairs_of
    return _training_pairs_of(model.data, torch.arange(model.data.n_dd_et))


if __name__ == '__main__':
    main()
