"""Time the per-relation calibration (`tipk_distmult_calibrate_stats`, `tipk_distmult_calibrate`, include/tipk.h section 4r) on the
device, next to a chunked torch composition of the same objective in fp32 on the same GPU in the same run, and measure the noise
floor of the fp32 gradient that the default `gtol` of `TIP.calibrate` rests on.

  python tools/bench_calibration.py                  BioSNAP size (645 drugs, dim 16): 1 097, 64 and 1 side effects, each with
                                                     about 4 200 training pairs and 1 090 planted held-out pairs, l2 = 1e-6
  python tools/bench_calibration.py --skip-baseline

The torch composition works from the definition: the features F = z[u] * z[v] of all n (n - 1) / 2 cells (formed once, outside
the timed window), per chunk of 64 side effects the logits S = F W^T, t = a s + b, dense per-cell weight tables [cells, R] for
the POS and the NEG class, and the six sums; its fit is the step rule of section 4m with a closed-form 2 x 2 solve, run for as
many evaluations as the slowest side effect of the fused fit needed (it has no active mask).

The noise floor: the fp64 optimum of every side effect (Newton in fp64 on the composition, started at the fused result), then
max |g32| of the device statistics at that optimum rounded to fp32.

Prints one JSON line per measurement: ms per call (device events around enough calls to fill `--window` seconds, after a
warm-up; two rounds, fused and composition alternating) and the launches one fit enqueues; for the statistics also the cells per
second and the share of the fp32 vector peak (157.3 TF) at the count of 2 dim + 60 FLOP per cell (the fma chain and about 60
operations of the transform, the latter an instruction-count ESTIMATE).
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
CHUNK = 64


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


def planted_triples(z, w, n_train, plant, seed):
    """(train, given) triples of all side effects, made on the device: per side effect about n_train random training cells
    and every other cell given with probability sigma(a* s + b*)."""
    g = torch.Generator(device=z.device).manual_seed(seed)
    n = z.shape[0]
    iu, iv = torch.triu_indices(n, n, 1, device=z.device)
    feat = z[iu] * z[iv]
    cells = iu.numel()
    tr, gv = [], []
    for r0 in range(0, w.shape[0], CHUNK):
        s = feat @ w[r0:r0 + CHUNK].t()                                   # [cells, chunk]
        is_train = torch.rand(s.shape, generator=g, device=z.device) < n_train / cells
        is_pos = (torch.rand(s.shape, generator=g, device=z.device) < torch.sigmoid(plant[0] * s + plant[1])) & ~is_train
        for mask, out in ((is_train, tr), (is_pos, gv)):
            c, r = torch.nonzero(mask, as_tuple=True)
            out.append(torch.stack([iu[c], iv[c], r + r0]))
    tr, gv = torch.cat(tr, 1).cpu(), torch.cat(gv, 1).cpu()
    return (tr[:2], tr[2]), (gv[:2], gv[2]), feat


def weight_tables(cl, n, dtype):
    """cpos, cneg [cells, Q] on the device: the per-cell weights of the definition (1/M on POS | NEG cells, 0 on TRAIN)."""
    q = cl.dense_w.numel()
    iu, iv = torch.triu_indices(n, n, 1)
    row = torch.full((n, n), -1, dtype=torch.int64)
    row[iu, iv] = torch.arange(iu.numel())
    query = torch.repeat_interleave(torch.arange(q), cl.ptr[1:] - cl.ptr[:-1])
    cell = row[cl.u.long(), cl.v.long()]
    inv_m = cl.dense_w.double()
    cneg = inv_m[None, :].repeat(iu.numel(), 1)
    cneg[cell, query] = 0.0
    cpos = torch.zeros((iu.numel(), q), dtype=torch.float64)
    cpos[cell, query] = cl.wpos.double()
    return cpos.to(DEV, dtype), cneg.to(DEV, dtype)


def torch_stats(feat, w, ab, cpos, cneg, l2):
    """loss [Q], g [Q, 2], H [Q, 3] = (aa, ab, bb) in the dtype of `feat`, in chunks of 64 side effects."""
    sp = torch.nn.functional.softplus
    out = []
    for r0 in range(0, w.shape[0], CHUNK):
        a, b = ab[r0:r0 + CHUNK, 0], ab[r0:r0 + CHUNK, 1]
        cp, cn = cpos[:, r0:r0 + CHUNK], cneg[:, r0:r0 + CHUNK]
        s = feat @ w[r0:r0 + CHUNK].t()
        t = a * s + b
        sig = torch.sigmoid(t)
        c1 = cn * sig - cp * (1 - sig)
        c2 = (cp + cn) * sig * (1 - sig)
        c2s = c2 * s
        da = a - 1
        out.append(torch.stack([(cp * sp(-t) + cn * sp(t)).sum(0) + 0.5 * l2 * da * da, (c1 * s).sum(0) + l2 * da, c1.sum(0),
                                (c2s * s).sum(0) + l2, c2s.sum(0), c2.sum(0)], 1))
    o = torch.cat(out)
    return o[:, 0], o[:, 1:3], o[:, 3:6]


def newton2(g, h):
    """-H^-1 g of the 2 x 2 systems h = (aa, ab, bb)."""
    det = h[:, 0] * h[:, 2] - h[:, 1] * h[:, 1]
    return -torch.stack([h[:, 2] * g[:, 0] - h[:, 1] * g[:, 1], h[:, 0] * g[:, 1] - h[:, 1] * g[:, 0]], 1) / det[:, None]


def torch_fit(feat, w, start, cpos, cneg, l2, evaluations):
    x = start.clone()
    trial, loss, grad, p, t = x, None, None, None, torch.ones(x.shape[0], device=x.device, dtype=x.dtype)
    for it in range(evaluations):
        lt, gt, ht = torch_stats(feat, w, trial, cpos, cneg, l2)
        if it == 0:
            accept = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
            loss, grad, p = lt, gt, torch.zeros_like(gt)
        else:
            accept = lt <= loss + 1e-4 * t * (grad * p).sum(1) + 16 * U * loss.abs()
        x = torch.where(accept[:, None], trial, x)
        loss, grad = torch.where(accept, lt, loss), torch.where(accept[:, None], gt, grad)
        p = torch.where(accept[:, None], newton2(gt, ht), p)
        t = torch.where(accept, torch.ones_like(t), t / 2)
        trial = x + t[:, None] * p
    return x, loss, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=645)
    ap.add_argument('--n-rel', type=int, default=1097)
    ap.add_argument('--dim', type=int, default=16)
    ap.add_argument('--train-pairs', type=int, default=4200)
    ap.add_argument('--max-iter', type=int, default=32)
    ap.add_argument('--gtol', type=float, default=1e-6)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_calibration times the device: no GPU visible'
    wall = time.time()
    n, n_rel, dim, l2 = args.n, args.n_rel, args.dim, 1e-6
    g = torch.Generator().manual_seed(0)
    z = (torch.randn((n, dim), generator=g) * (2.0 / dim ** 0.5)).float().to(DEV)
    rel_w = torch.randn((n_rel, dim), generator=g).float().to(DEV)
    train, given, feat = planted_triples(z, rel_w, args.train_pairs, (1.5, -6.5), 1)
    cells = n * (n - 1) // 2
    for q in sorted({n_rel, min(64, n_rel), 1}, reverse=True):
        rel = torch.arange(q)
        cl = ops.calibration_lists(train, given, n, n_rel, rel)
        start = torch.stack([torch.ones(q, dtype=torch.float64), torch.log((cl.n_pos.double() + .5) / (cl.n_neg.double() + .5))],
                            1).float().to(DEV)
        dcl = cl._replace(**{k: getattr(cl, k).to(DEV) for k in ('ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w', 'q_rel')})   # no copy inside
        fit = ops.distmult_calibrate(z, rel_w, dcl, l2, start, args.max_iter, args.gtol)
        torch.cuda.synchronize()
        info = fit[3].cpu()
        evaluations = int(info[:, 1].max())
        launches = 1 + 3 * (args.max_iter + 1)                           # init; (dense, finish, step) per evaluation
        splits = _lib.lib().tipk_distmult_calibrate_splits(n, dim, q)
        print(json.dumps({'case': 'shape', 'side_effects': q, 'cells': cells, 'parts': splits, 'listed_cells': int(cl.ptr[-1]),
                          'n_pos_mean': float(cl.n_pos.double().mean()), 'scale_min_max': [float(fit[0][:, 0].min()),
                                                                                          float(fit[0][:, 0].max())],
                          'status': sorted(set(info[:, 0].tolist())), 'evaluations_min_max': [int(info[:, 1].min()), evaluations]}),
              flush=True)
        wq = rel_w[:q].contiguous()
        if not args.skip_baseline:
            cpos, cneg = weight_tables(cl, n, torch.float32)
            ref = torch_stats(feat, wq, start, cpos, cneg, l2)
            got = ops.distmult_calibrate_stats(z, rel_w, start, dcl, l2)
            h3 = torch.stack([got[2][:, 0, 0], got[2][:, 0, 1], got[2][:, 1, 1]], 1)
            far = [float((a - b).abs().max() / b.abs().max()) for a, b in zip((got[0], got[1], h3), ref)]
            xt = torch_fit(feat, wq, start, cpos, cneg, l2, evaluations)[0]
            print(json.dumps({'case': 'agreement', 'side_effects': q, 'stats_max_rel_diff': far,
                              'fit_max_abs_diff': float((xt - fit[0]).abs().max())}), flush=True)
            # the noise floor of the fp32 gradient: at the fp64 optimum, rounded to fp32
            cp64, cn64, f64, w64 = cpos.double(), cneg.double(), feat.double(), wq.double()
            x = fit[0].double()
            for _ in range(6):
                _, g64, h64 = torch_stats(f64, w64, x, cp64, cn64, l2)
                x = x + newton2(g64, h64)
            _, g64, _ = torch_stats(f64, w64, x, cp64, cn64, l2)
            x32 = x.float()
            g32 = ops.distmult_calibrate_stats(z, rel_w, x32, dcl, l2)[1]
            _, g64_at32, _ = torch_stats(f64, w64, x32.double(), cp64, cn64, l2)
            floor = float(g32.abs().max())
            print(json.dumps({'case': 'gradient_noise_floor', 'side_effects': q, 'max_abs_g64_at_fp64_optimum': float(g64.abs().max()),
                              'max_abs_g32_at_rounded_optimum': floor,
                              'max_abs_g64_at_rounded_optimum': float(g64_at32.abs().max()),
                              'max_abs_g32_minus_g64': float((g32.double() - g64_at32).abs().max()),
                              'gtol_rule_max_1e-6_8x': max(1e-6, 8 * floor)}), flush=True)
            del cp64, cn64, f64
        for rnd in range(2):
            ms, reps = timed(lambda: ops.distmult_calibrate_stats(z, rel_w, start, dcl, l2), args.window, args.warmup)
            rate = q * cells / (ms * 1e-3)
            print(json.dumps({'case': 'fused_stats', 'side_effects': q, 'round': rnd, 'ms': round(ms, 4), 'reps': reps, 'launches': 2,
                              'cells_per_s': round(rate, -6),
                              'fraction_of_fp32_vector_peak_estimate': round(rate * (2 * dim + 60) / PEAK_FP32, 4)}), flush=True)
            if not args.skip_baseline:
                ms, reps = timed(lambda: torch_stats(feat, wq, start, cpos, cneg, l2), args.window, args.warmup)
                print(json.dumps({'case': 'torch_stats', 'side_effects': q, 'round': rnd, 'ms': round(ms, 4), 'reps': reps}), flush=True)
            ms, reps = timed(lambda: ops.distmult_calibrate(z, rel_w, dcl, l2, start, args.max_iter, args.gtol), args.window,
                             args.warmup)
            print(json.dumps({'case': 'fused_fit', 'side_effects': q, 'round': rnd, 'ms': round(ms, 4), 'reps': reps,
                              'launches': launches, 'max_iter': args.max_iter, 'evaluations_max': evaluations}), flush=True)
            if not args.skip_baseline:
                ms, reps = timed(lambda: torch_fit(feat, wq, start, cpos, cneg, l2, evaluations), args.window, args.warmup)
                print(json.dumps({'case': 'torch_fit', 'side_effects': q, 'round': rnd, 'ms': round(ms, 4), 'reps': reps,
                                  'evaluations': evaluations}), flush=True)
        if not args.skip_baseline:
            del cpos, cneg
    print(json.dumps({'wall_s': round(time.time() - wall, 1)}), flush=True)


if __name__ == '__main__':
    main()
