"""Time the pair top-k (`tipk_distmult_pair_topk` / `tipk_pair_table_pair_topk`, include/tipk.h section 4d) on the device,
next to `TIP.pred_topk` on the same pairs in the same run.

  python tools/bench_pair_topk.py                  all 207 690 unordered pairs of the bundled BioSNAP graph (645 drugs,
                                                   1 097 relations, dim 16), k = 10: the op with and without the training
                                                   side effects excluded, on the LDS route and the forced streamed route;
                                                   the NN decoder's tables; `TIP.side_effects` end to end; `TIP.pred_topk`
  python tools/bench_pair_topk.py --skip-baseline  without the `pred_topk` baseline

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`), triples/s and the
share of the scoring FLOP bound (2 FLOP per triple and column at the 157.3 TF fp32 peak; the table variant has one add per
triple).  Inputs: the model as constructed (initial embeddings, initial decoder weights), the graph's training edges.
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


def report(name, ms, n_pairs, n_rel, flop_per_triple, extra=None):
    triples = n_pairs * n_rel
    flops = float(flop_per_triple) * triples
    line = {'case': name, 'ms': round(ms, 4), 'pairs': n_pairs, 'triples': triples, 'triples_per_s': triples / (ms * 1e-3),
            'flop_bound_ms': round(flops / PEAK_FP32 * 1e3, 4), 'fraction_of_flop_bound': round(flops / PEAK_FP32 / (ms * 1e-3), 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_pair_topk times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting
    t = time.time()
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    dim = z.shape[1]
    pairs = torch.triu_indices(n, n, 1).to(DEV)
    P = pairs.shape[1]
    known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n)
    extra = {'k': args.k, 'known_pairs': known[0].numel(), 'known_entries': known[2].numel()}

    for route in ('lds', 'stream'):
        _lib.set_option('pair_topk_stream', int(route == 'stream'))
        try:
            assert _lib.lib().tipk_distmult_pair_topk_lds_route(dim, R) == int(route == 'lds')
            ms = timed(lambda: ops.distmult_pair_topk(z, w, pairs, args.k), args.reps, args.warmup)
            report('biosnap_pair_topk_%s_unfiltered' % route, ms, P, R, 2 * dim, {'k': args.k})
            ms = timed(lambda: ops.distmult_pair_topk(z, w, pairs, args.k, known), args.reps, args.warmup)
            report('biosnap_pair_topk_%s_exclude_train' % route, ms, P, R, 2 * dim, extra)
        finally:
            _lib.set_option('pair_topk_stream', 0)

    g = torch.Generator().manual_seed(1)
    s1, s2 = torch.randn(n, R, generator=g).to(DEV), torch.randn(n, R, generator=g).to(DEV)
    ms = timed(lambda: ops.pair_table_pair_topk(s1, s2, pairs, args.k), args.reps, args.warmup)
    report('biosnap_pair_topk_table_unfiltered', ms, P, R, 1, {'k': args.k})
    ms = timed(lambda: ops.pair_table_pair_topk(s1, s2, pairs, args.k, known), args.reps, args.warmup)
    report('biosnap_pair_topk_table_exclude_train', ms, P, R, 1, extra)

    ms = timed(lambda: model.side_effects(pairs, k=args.k, exclude='train'), args.reps, args.warmup)
    report('biosnap_side_effects_exclude_train', ms, P, R, 2 * dim, extra)
    ms = timed(lambda: model.side_effects(pairs, k=args.k), args.reps, args.warmup)
    report('biosnap_side_effects_unfiltered', ms, P, R, 2 * dim, {'k': args.k})

    if not args.skip_baseline:
        ms = timed(lambda: model.pred_topk(pairs, k=args.k), max(1, args.reps // 10), 1)
        report('biosnap_pred_topk_unfiltered', ms, P, R, 2 * dim, {'k': args.k})
    print(json.dumps({'wall_s': round(time.time() - t, 1)}), flush=True)


if __name__ == '__main__':
    main()
