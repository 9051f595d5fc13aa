"""Time the DistMult screen (`tipk_distmult_screen`, include/tipk.h section 4c) on the device.

  python tools/bench_screen.py --case biosnap      full relation screen (1 097 queries) + 645 drug queries at BioSNAP size
                                                   (N = 645, dim 16, k = 100, training positives excluded), bitmap and
                                                   forced search route
  python tools/bench_screen.py --case torch        the same relation screen in torch: chunked bmm, mask, topk
  python tools/bench_screen.py --case config5      N = 10 000, dim 128, 4 relations with ~1e5 known pairs each, k = 100

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`), candidates/s and
the share of the scoring FLOP bound (2 FLOP per candidate and column at the 157.3 TF fp32 peak).  Run each case under its
own time limit.  BioSNAP inputs: random z and w of the trained model's shapes, the bundled graph's training positives.
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


def report(name, ms, queries, n, dim, extra=None):
    cand = sum(n * (n - 1) // 2 if u < 0 else n - 1 for _, u in queries)
    flops = 2.0 * cand * dim
    line = {'case': name, 'ms': round(ms, 4), 'queries': len(queries), 'candidates': cand,
            'candidates_per_s': cand / (ms * 1e-3), 'flop_bound_ms': round(flops / PEAK_FP32 * 1e3, 4),
            'fraction_of_flop_bound': round(flops / PEAK_FP32 / (ms * 1e-3), 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def biosnap_inputs():
    from tip_amd.data import build_data_dict
    from tip_amd.neg_sampling import _cached_keys
    dd = build_data_dict()
    n, R, dim = dd['n_drug'], dd['n_dd_et'], 16
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(n, dim, generator=g) / 2).to(DEV)
    w = (torch.randn(R, dim, generator=g) / 2).to(DEV)
    idx = dd['dd_train_idx'].to(DEV)
    keys, ptr = _cached_keys(idx, n, dd['dd_train_range'])[:2]
    return z, w, (keys, ptr), n, R, dim


def case_biosnap(args):
    z, w, known, n, R, dim = biosnap_inputs()
    rel_q = [[r, -1] for r in range(R)]
    drug_q = [[(7 * u) % R, u] for u in range(n)]
    for route in ('bitmap', 'search'):
        _lib.set_option('screen_search', int(route == 'search'))
        try:
            qt = torch.tensor(rel_q)
            ms = timed(lambda: ops.distmult_screen(z, w, qt, args.k, known), args.reps, args.warmup)
            report('biosnap_relation_screen_' + route, ms, rel_q, n, dim, {'k': args.k})
            qd = torch.tensor(drug_q)
            ms = timed(lambda: ops.distmult_screen(z, w, qd, args.k, known), args.reps, args.warmup)
            report('biosnap_drug_screen_' + route, ms, drug_q, n, dim, {'k': args.k})
        finally:
            _lib.set_option('screen_search', 0)


def torch_screen(z, w, known, n, k, chunk=64):
    """The relation screen in torch: logits of a chunk of relations by bmm, pairs u >= v and known pairs set to -inf,
    topk over the flattened n x n matrix."""
    keys, ptr = known
    R = w.shape[0]
    rel = torch.repeat_interleave(torch.arange(R, device=DEV), ptr[1:] - ptr[:-1])
    lower = ~torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), 1)
    vals, ids = [], []
    for r0 in range(0, R, chunk):
        r1 = min(R, r0 + chunk)
        s = torch.bmm(z[None] * w[r0:r1, :, None].transpose(1, 2), z.t()[None].expand(r1 - r0, -1, -1))
        s.masked_fill_(lower[None], float('-inf'))
        sel = (rel >= r0) & (rel < r1)
        kr, kk = rel[sel] - r0, keys[sel]
        flat = s.view(r1 - r0, -1)
        flat[kr, kk] = float('-inf')
        flat[kr, (kk % n) * n + kk // n] = float('-inf')
        top = torch.topk(flat, k, dim=1)
        vals.append(top.values)
        ids.append(top.indices)
    return torch.cat(vals), torch.cat(ids)


def case_torch(args):
    z, w, known, n, R, dim = biosnap_inputs()
    ms = timed(lambda: torch_screen(z, w, known, n, args.k), max(1, args.reps // 4), 1)
    report('biosnap_relation_screen_torch', ms, [[r, -1] for r in range(R)], n, dim, {'k': args.k})


def case_config5(args):
    n, dim, R = 10000, 128, 4
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(n, dim, generator=g) / dim ** 0.25).to(DEV)
    w = (torch.randn(R, dim, generator=g) / dim ** 0.25).to(DEV)
    keys, ptr = [], [0]
    for _ in range(R):
        a = torch.randint(0, n, (100000,), generator=g)
        b = torch.randint(0, n, (100000,), generator=g)
        ks = torch.unique(a[a != b] * n + b[a != b])
        keys.append(ks)
        ptr.append(ptr[-1] + ks.numel())
    known = (torch.cat(keys).to(DEV), torch.tensor(ptr, dtype=torch.int64, device=DEV))
    q = [[r, -1] for r in range(R)]
    qt = torch.tensor(q)
    ms = timed(lambda: ops.distmult_screen(z, w, qt, args.k, known), max(1, args.reps // 4), 1)
    report('config5_relation_screen_search', ms, q, n, dim, {'k': args.k})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=['biosnap', 'torch', 'config5'], required=True)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_screen times the device: no GPU visible'
    t = time.time()
    {'biosnap': case_biosnap, 'torch': case_torch, 'config5': case_config5}[args.case](args)
    print(json.dumps({'case': args.case, 'wall_s': round(time.time() - t, 1)}), flush=True)


if __name__ == '__main__':
    main()
