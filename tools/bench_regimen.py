"""Time the regimen top-k (`tipk_distmult_regimen_topk` / `tipk_pair_table_regimen_topk`, include/tipk.h section 4e) on the
device, next to a torch composition that materialises the pair x relation logits and reduces them, in the same run.

  python tools/bench_regimen.py            10 000 random regimens of 8 drugs and 1 000 of 32 drugs over the bundled BioSNAP
                                           graph's model (645 drugs, 1 097 relations, dim 16), k = 10: both aggregates, with
                                           and without the training side effects excluded, the LDS-image route and the forced
                                           global route, the NN decoder's tables, and the torch composition
  python tools/bench_regimen.py --random   random z / rel_w of that shape and no known lists (no data set needed)

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`), triples/s and the
share of the scoring FLOP bound (2 FLOP per triple and column at the 157.3 TF fp32 peak; the table variant has one add per
triple).
"""
import argparse
import json
import os
import sys

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


def report(name, ms, n_reg, m, n_rel, flop_per_triple, extra=None):
    triples = n_reg * (m * (m - 1) // 2) * n_rel
    flops = float(flop_per_triple) * triples
    line = {'case': name, 'ms': round(ms, 4), 'regimens': n_reg, 'drugs': m, 'triples': triples,
            'triples_per_s': triples / (ms * 1e-3), 'flop_bound_ms': round(flops / PEAK_FP32 * 1e3, 4),
            'fraction_of_flop_bound': round(flops / PEAK_FP32 / (ms * 1e-3), 5)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def torch_composition(z, w, drugs, n_reg, m, k, aggregate, chunk=2000):
    """The same answer from torch ops: every pair's logits [G, P, R] materialised (in chunks of regimens), reduced over the
    pairs, top k.  No known filter, no driver pair."""
    iu = torch.triu_indices(m, m, 1, device=z.device)
    d = drugs.view(n_reg, m).long()
    out = []
    for g0 in range(0, n_reg, chunk):
        dg = d[g0:g0 + chunk]
        logits = (z[dg[:, iu[0]]] * z[dg[:, iu[1]]]) @ w.t()
        agg = logits.amax(1) if aggregate == 'max' else torch.nn.functional.softplus(logits).sum(1)
        out.append(torch.topk(agg, k, dim=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--random', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_regimen times the device: no GPU visible'
    g = torch.Generator().manual_seed(1)
    known = None
    if args.random:
        n, R, dim = 645, 1097, 16
        z, w = (torch.randn(n, dim, generator=g) / 2).to(DEV), (torch.randn(R, dim, generator=g) / 2).to(DEV)
    else:
        from tip_amd.layers import TIP, Setting
        torch.manual_seed(0)
        model = TIP(Setting(), torch.device(DEV), data_path=None)
        d = model.data
        n, R = d.n_drug, d.n_dd_et
        z, w = model.embeddings.detach(), model.decoder.weight.detach()
        dim = z.shape[1]
        known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n)
    s1, s2 = torch.randn(n, R, generator=g).to(DEV), torch.randn(n, R, generator=g).to(DEV)

    for n_reg, m in ((10000, 8), (1000, 32)):
        drugs = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(n_reg)]).sort(1).values
        drugs = drugs.reshape(-1).to(torch.int32).to(DEV)
        ptr = (m * torch.arange(n_reg + 1)).to(DEV)
        tag = '%dx%d' % (n_reg, m)
        for agg in ('max', 'noisy_or'):
            for route in ('lds', 'global'):
                _lib.set_option('regimen_global', int(route == 'global'))
                try:
                    assert _lib.lib().tipk_distmult_regimen_topk_lds_route(dim, R) == int(route == 'lds')
                    for kn, what in ((None, 'unfiltered'), (known, 'exclude_train')):
                        if what == 'exclude_train' and known is None:
                            continue
                        ms = timed(lambda: ops.distmult_regimen_topk(z, w, drugs, ptr, args.k, agg, kn), args.reps, args.warmup)
                        report('regimen_%s_%s_%s_%s' % (tag, agg, route, what), ms, n_reg, m, R, 2 * dim, {'k': args.k})
                finally:
                    _lib.set_option('regimen_global', 0)
            for kn, what in ((None, 'unfiltered'), (known, 'exclude_train')):
                if what == 'exclude_train' and known is None:
                    continue
                ms = timed(lambda: ops.pair_table_regimen_topk(s1, s2, drugs, ptr, args.k, agg, kn), args.reps, args.warmup)
                report('regimen_%s_%s_table_%s' % (tag, agg, what), ms, n_reg, m, R, 1, {'k': args.k})
            ms = timed(lambda: torch_composition(z, w, drugs, n_reg, m, args.k, agg), max(1, args.reps // 3), 1)
            report('regimen_%s_%s_torch_composition_unfiltered' % (tag, agg), ms, n_reg, m, R, 2 * dim, {'k': args.k})


if __name__ == '__main__':
    main()
