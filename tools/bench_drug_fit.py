"""Time the new-drug fit (`tipk_distmult_drug_fit_stats`, `tipk_distmult_drug_fit`, include/tipk.h section 4q) on the device, next
to the torch composition of the same objective in fp32 on the same GPU in the same run.

  python tools/bench_drug_fit.py                     BioSNAP size (645 drugs, 1 097 side effects, dim 16), M = 1 and 64 new
                                                     drugs with P = 50 planted reports each, l2 = 1e-4
  python tools/bench_drug_fit.py --skip-baseline

The torch composition works from the definition: the features F = z[v] * rel_w[r] of all n R cells by broadcasting (formed once,
outside the timed window), S = F X^T, dense per-cell coefficient tables [n R, M], g = C^T F and H = F^T diag(sigma') F per drug
through the [M, n R, dim] temporary, and the step rule of section 4m with a batched Cholesky.  Its fit runs as many evaluations
for every drug as the slowest drug of the fused fit needed (it has no active mask).

Prints one JSON line per measurement: ms per call (device events around enough calls to fill `--window` seconds, after a
warm-up; two rounds, fused and composition alternating), the launches one fit enqueues, and for the statistics the achieved
share of the fp32 matrix-core peak (157.3 TF) at the algorithmic count n R (dim^2 + 2 dim) 2 FLOP per drug.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

PEAK_FP32 = 157.3e12
DEV = 'cuda:0'
U = 2.0 ** -24


def timed(fn, window, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.time()
    fn()
    torch.cuda.synchronize()
    reps = int(min(2000, max(3, window / max(time.time() - t, 1e-6))))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, reps


def planted_cells(z, rel_w, count, seed):
    """The `count` cells a hidden row scores highest under unit Gumbel noise (as tests/drug_fit_cases.py)."""
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(z.shape[1], generator=g).double() * 2.0
    s = ((z.double() * hidden) @ rel_w.double().t()).reshape(-1)
    noise = -torch.log(-torch.log(torch.rand(s.shape, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)))
    top = torch.topk(s + noise, count).indices
    return list(zip((top // rel_w.shape[0]).tolist(), (top % rel_w.shape[0]).tolist()))


def coefficient_tables(fl, cells, n_rel):
    """cpos, cneg fp32 [n R, M] on the device: the per-cell weights of the definition."""
    m = fl.dense_w.numel()
    drug = torch.repeat_interleave(torch.arange(m), fl.ptr[1:] - fl.ptr[:-1])
    cell = fl.v.long() * n_rel + fl.r.long()
    cpos = torch.zeros((cells, m))
    cpos[cell, drug] = fl.wpos
    cneg = fl.dense_w[None, :].repeat(cells, 1)
    cneg[cell, drug] = 0.0
    return cpos.to(DEV), cneg.to(DEV)


def torch_stats(feat, x, cpos, cneg, l2):
    s = feat @ x.t()                                                     # [n R, M]
    sp = torch.nn.functional.softplus
    sig = torch.sigmoid(s)
    loss = (cpos * sp(-s) + cneg * sp(s)).sum(0) + 0.5 * l2 * (x * x).sum(1)
    grad = (cneg * sig - cpos * (1 - sig)).t() @ feat + l2 * x
    cf = ((cpos + cneg) * sig * (1 - sig)).t()[:, :, None] * feat[None]   # the [M, n R, dim] temporary
    hess = cf.transpose(1, 2) @ feat + l2 * torch.eye(x.shape[1], device=x.device)
    return loss, grad, hess


def torch_fit(feat, cpos, cneg, l2, evaluations):
    m, dim = cpos.shape[1], feat.shape[1]
    x = torch.zeros((m, dim), device=DEV)
    trial, loss, grad, p, t = x, None, None, None, torch.ones(m, device=DEV)
    for it in range(evaluations):
        lt, gt, ht = torch_stats(feat, trial, cpos, cneg, l2)
        if it == 0:
            accept = torch.ones(m, dtype=torch.bool, device=DEV)
            loss, grad, p = lt, gt, torch.zeros_like(gt)
        else:
            accept = lt <= loss + 1e-4 * t * (grad * p).sum(1) + 16 * U * loss.abs()
        x = torch.where(accept[:, None], trial, x)
        loss, grad = torch.where(accept, lt, loss), torch.where(accept[:, None], gt, grad)
        newton = -torch.cholesky_solve(gt[:, :, None], torch.linalg.cholesky_ex(ht)[0])[:, :, 0]
        p = torch.where(accept[:, None], newton, p)
        t = torch.where(accept, torch.ones_like(t), t / 2)
        trial = x + t[:, None] * p
    return x, loss, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=645)
    ap.add_argument('--n-rel', type=int, default=1097)
    ap.add_argument('--dim', type=int, default=16)
    ap.add_argument('--reports', type=int, default=50)
    ap.add_argument('--max-iter', type=int, default=16)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_drug_fit times the device: no GPU visible'
    wall = time.time()
    n, n_rel, dim, l2 = args.n, args.n_rel, args.dim, 1e-4
    g = torch.Generator().manual_seed(0)
    z_h = (torch.randn((n, dim), generator=g) * (2.0 / dim ** 0.5)).float()
    w_h = torch.randn((n_rel, dim), generator=g).float()
    z, rel_w = z_h.to(DEV), w_h.to(DEV)
    feat = None
    for m in (1, 64):
        lists = [planted_cells(z_h, w_h, args.reports, 100 + i) for i in range(m)]
        fl = ops.drug_fit_csr(lists, n, n_rel)
        fl = fl._replace(**{k: getattr(fl, k).to(DEV) for k in ('ptr', 'v', 'r', 'wpos', 'wneg', 'dense_w')})   # no copy inside
        x = (torch.randn((m, dim), generator=g) * 0.5).float().to(DEV)
        fit = ops.distmult_drug_fit(z, rel_w, fl, None, l2, None, args.max_iter)
        torch.cuda.synchronize()
        info = fit[3].cpu()
        evaluations = int(info[:, 1].max())
        launches = 1 + 3 * (args.max_iter + 1) + 2                       # init; (dense, finish, step) pairs; the Hessian pair
        flops = 2.0 * n * n_rel * (dim * dim + 2 * dim) * m
        if not args.skip_baseline:
            if feat is None:
                feat = (z[:, None, :] * rel_w[None, :, :]).reshape(n * n_rel, dim).contiguous()
            cpos, cneg = coefficient_tables(ops.drug_fit_csr(lists, n, n_rel), n * n_rel, n_rel)
            ref = torch_stats(feat, x, cpos, cneg, l2)
            got = ops.distmult_drug_fit_stats(z, rel_w, x, fl, None, l2)
            far = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref)]
            xt = torch_fit(feat, cpos, cneg, l2, evaluations)[0]
            print(json.dumps({'case': 'agreement', 'drugs': m, 'stats_max_rel_diff': far,
                              'fit_max_abs_diff': float((xt - fit[0]).abs().max())}), flush=True)
        for rnd in range(2):
            ms, reps = timed(lambda: ops.distmult_drug_fit_stats(z, rel_w, x, fl, None, l2), args.window, args.warmup)
            print(json.dumps({'case': 'fused_stats', 'drugs': m, 'round': rnd, 'ms': round(ms, 4), 'reps': reps, 'launches': 2,
                              'fraction_of_fp32_mfma_peak': round(flops / PEAK_FP32 / (ms * 1e-3), 4)}), flush=True)
            if not args.skip_baseline:
                ms, reps = timed(lambda: torch_stats(feat, x, cpos, cneg, l2), args.window, args.warmup)
                print(json.dumps({'case': 'torch_stats', 'drugs': m, 'round': rnd, 'ms': round(ms, 4), 'reps': reps}), flush=True)
            ms, reps = timed(lambda: ops.distmult_drug_fit(z, rel_w, fl, None, l2, None, args.max_iter), args.window, args.warmup)
            print(json.dumps({'case': 'fused_fit', 'drugs': m, 'round': rnd, 'ms': round(ms, 4), 'reps': reps, 'launches': launches,
                              'max_iter': args.max_iter, 'status': sorted(set(info[:, 0].tolist())),
                              'evaluations_min_max': [int(info[:, 1].min()), evaluations]}), flush=True)
            if not args.skip_baseline:
                ms, reps = timed(lambda: torch_fit(feat, cpos, cneg, l2, evaluations), args.window, args.warmup)
                print(json.dumps({'case': 'torch_fit', 'drugs': m, 'round': rnd, 'ms': round(ms, 4), 'reps': reps,
                                  'evaluations': evaluations}), flush=True)
    print(json.dumps({'wall_s': round(time.time() - wall, 1)}), flush=True)


if __name__ == '__main__':
    main()
