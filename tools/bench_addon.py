"""Time the add-on burden (`tipk_distmult_addon_burden` / `tipk_pair_table_addon_burden`, include/tipk.h section 4i) on the
device, next to the same quantity from chunked torch ops, in the same run.

  python tools/bench_addon.py              1 query x all 645 drugs and 256 queries x all 645 drugs, contexts of 5 and of 20
                                           drugs, over the bundled BioSNAP graph's model (645 drugs, 1 097 relations, dim 16),
                                           k = 10: both aggregates, with and without the training side effects excluded, the
                                           LDS-image route and the forced global route, the NN decoder's tables, and the torch
                                           composition
  python tools/bench_addon.py --random     random z / rel_w of that shape and no known lists (no data set needed)

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`; a case is repeated
until the timed window holds at least `--min-ms` of work), triples/s, the share of the scoring FLOP bound (2 FLOP per triple
and column at the 157.3 TF fp32 peak; the table variant has one add per triple) and, for the torch composition, the largest
difference of its burdens from the kernel's.
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


def timed(fn, reps, warmup, min_ms):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        total = t0.elapsed_time(t1)
        if total >= min_ms or reps >= 1 << 14:
            return total / reps, reps
        reps *= 4


def report(name, ms, reps, n_q, n_cand, m, n_rel, flop_per_triple, extra=None):
    triples = n_q * n_cand * m * n_rel
    flops = float(flop_per_triple) * triples
    line = {'case': name, 'ms': round(ms, 4), 'reps': reps, 'queries': n_q, 'candidates': n_cand, 'context': m,
            'triples': triples, 'triples_per_s': triples / (ms * 1e-3), 'flop_bound_ms': round(flops / PEAK_FP32 * 1e3, 5),
            'fraction_of_flop_bound': round(flops / PEAK_FP32 / (ms * 1e-3), 5)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def torch_composition(z, w, ctx, cand, k, aggregate, chunk=16):
    """The same quantity from torch ops: the [queries x candidates x context x relations] logits materialised in chunks of
    queries, reduced over the context, turned into probabilities and summed over the relations; NaN for a candidate inside
    its context; the k lowest.  No known filter, no weights."""
    zc = z[cand.long()]
    out = []
    for q0 in range(0, ctx.shape[0], chunk):
        s = ctx[q0:q0 + chunk].long()                                    # [g, m]
        h = zc[None, :, None, :] * z[s][:, None, :, :]                   # [g, C, m, dim]
        logits = h @ w.t()                                               # [g, C, m, R]
        if aggregate == 'max':
            p = torch.sigmoid(logits.amax(2))
        else:
            p = -torch.expm1(-torch.nn.functional.softplus(logits).sum(2))
        b = p.sum(2)
        member = (cand.long()[None, :, None] == s[:, None, :]).any(2)
        out.append(torch.where(member, torch.full_like(b, float('nan')), b))
    burden = torch.cat(out)
    best = torch.topk(torch.where(torch.isnan(burden), torch.full_like(burden, float('inf')), burden), k, dim=1, largest=False)
    return burden, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--random', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_addon times the device: no GPU visible'
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
    cand = torch.arange(n, dtype=torch.int32, device=DEV)
    weights = (3 * torch.rand(R, generator=g)).to(DEV)

    for n_q in (1, 256):
        for m in (5, 20):
            ctx = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(n_q)]).sort(1).values.to(DEV)
            drugs, ptr = ctx.reshape(-1).to(torch.int32), (m * torch.arange(n_q + 1)).to(DEV)
            tag = '%dx%d_ctx%d' % (n_q, n, m)
            for agg in ('noisy_or', 'max'):
                ref = None
                for route in ('lds', 'global'):
                    _lib.set_option('addon_global', int(route == 'global'))
                    try:
                        assert _lib.lib().tipk_distmult_addon_burden_lds_route(dim, R) == int(route == 'lds')
                        for kn, wts, what in ((None, None, 'unfiltered'), (known, weights, 'exclude_train_weighted')):
                            if kn is None and wts is not None:
                                continue
                            fn = lambda: ops.distmult_addon_burden(z, w, drugs, ptr, cand, None, args.k, agg, wts, kn)
                            ms, reps = timed(fn, args.reps, args.warmup, args.min_ms)
                            report('addon_%s_%s_%s_%s' % (tag, agg, route, what), ms, reps, n_q, n, m, R, 2 * dim, {'k': args.k})
                            if what == 'unfiltered':
                                ref = fn()[0]
                    finally:
                        _lib.set_option('addon_global', 0)
                fn = lambda: ops.pair_table_addon_burden(s1, s2, drugs, ptr, cand, None, args.k, agg)
                ms, reps = timed(fn, args.reps, args.warmup, args.min_ms)
                report('addon_%s_%s_table_unfiltered' % (tag, agg), ms, reps, n_q, n, m, R, 1, {'k': args.k})
                fn = lambda: torch_composition(z, w, ctx, cand, args.k, agg)
                ms, reps = timed(fn, max(1, args.reps // 2), 1, args.min_ms)
                got = fn()[0]
                same_nan = bool((torch.isnan(got) == torch.isnan(ref)).all())
                diff = float((got - ref).abs().nan_to_num(0.0).max())
                report('addon_%s_%s_torch_composition_unfiltered' % (tag, agg), ms, reps, n_q, n, m, R, 2 * dim,
                       {'k': args.k, 'max_abs_diff_from_kernel': diff, 'same_nan': same_nan})


if __name__ == '__main__':
    main()
