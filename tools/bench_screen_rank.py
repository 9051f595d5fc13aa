"""Time the screen rank (`tipk_distmult_screen_rank`, include/tipk.h section 4h) on the held-out triples of the bundled
BioSNAP graph, next to the torch composition that answers the same question without the kernel.

  python tools/bench_screen_rank.py                  filter 'all': the launches alone on the bitmap route and the forced
                                                     search route, the unfiltered launches, `TIP.rank_pairs` end to end,
                                                     and the torch composition
  python tools/bench_screen_rank.py --skip-baseline  without the torch composition
  python tools/bench_screen_rank.py --write profiles/screen_rank.md   also write the table

Prints one JSON line per measurement: the median, minimum and maximum over `--repeats` timings, each the ms per call of
`--reps` calls between two device events, after `--warmup` calls.  Inputs: the model after `--steps` training steps (dim 16),
the graph's train and test edges.  The torch composition takes one relation at a time: the dense fp32 logits
(z * w_r) @ z.T (its own summation order: its ranks need not agree with the kernel's where logits are within rounding), the
upper triangle gathered, the relation's known pairs masked out through a boolean [n * n] table, one sort of the remaining
logits and a `searchsorted` of the targets' logits in it (it counts the strictly higher logits and leaves ties alone)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps, warmup, repeats):
    """[ms per call] of `repeats` timings"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return out


def torch_ranks(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, known):
    """Filtered ranks by the torch composition: rank int64 [T] in the grouped order of `ops.targets_by_relation`."""
    n = z.shape[0]
    keys, kptr = known
    iu = torch.triu_indices(n, n, 1, device=z.device)
    key_all = iu[0] * n + iu[1]
    out = torch.empty(tgt_u.numel(), dtype=torch.int64, device=z.device)
    ptr, kp = tgt_ptr.tolist(), kptr.tolist()
    a, b = torch.minimum(tgt_u, tgt_v).long(), torch.maximum(tgt_u, tgt_v).long()
    for qi, r in enumerate(q_rel.tolist()):
        L = (z * w[r]) @ z.t()
        ks = keys[kp[r]:kp[r + 1]]
        listed = torch.zeros(n * n, dtype=torch.bool, device=z.device)
        listed[ks] = True
        listed[(ks % n) * n + torch.div(ks, n, rounding_mode='floor')] = True
        cand = torch.sort(-L[iu[0], iu[1]][~listed[key_all]]).values
        t = slice(ptr[qi], ptr[qi + 1])
        out[t] = 1 + torch.searchsorted(cand, -L[a[t], b[t]].contiguous(), right=False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3, help='training steps before the measurement')
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None, help='write the measurements as a markdown table to this file')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_screen_rank times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting, _screen_known
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for _ in range(args.steps):
        opt.zero_grad()
        model().backward()
        opt.step()
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    dim = z.shape[1]
    q_rel, tgt_ptr, tgt_u, tgt_v, order = ops.targets_by_relation(d.dd_test_idx, d.dd_test_et, R)
    known = _screen_known(d, 'all')
    per = tgt_ptr[1:] - tgt_ptr[:-1]
    shape = {'triples': tgt_u.numel(), 'queries': q_rel.numel(), 'most_targets_of_a_query': int(per.max()), 'drugs': n,
             'relations': R, 'dim': dim, 'known_keys': known[0].numel(), 'training_steps': args.steps,
             'chunk': int(_lib.lib().tipk_distmult_screen_rank_chunk())}
    print(json.dumps(shape), flush=True)
    lines = []

    def report(name, ms, extra=None):
        line = {'case': name, 'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4),
                'ms_max': round(max(ms), 4)}
        line.update(extra or {})
        lines.append(line)
        print(json.dumps(line), flush=True)

    def launch(kn=known):
        return ops.distmult_screen_rank(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, kn)

    got = {}
    for route in ('bitmap', 'search'):
        _lib.set_option('screen_search', int(route == 'search'))
        try:
            assert _lib.lib().tipk_distmult_screen_bitmap_route(n) == int(route == 'bitmap')
            got[route] = launch()
            report('screen_rank_%s_filter_all' % route, timed(launch, args.reps, args.warmup, args.repeats))
        finally:
            _lib.set_option('screen_search', 0)
    assert torch.equal(got['bitmap'][0], got['search'][0])
    report('screen_rank_unfiltered', timed(lambda: launch(None), args.reps, args.warmup, args.repeats))
    report('rank_pairs_filter_all', timed(lambda: model.rank_pairs(filter='all'), args.reps, args.warmup, args.repeats))
    rep = model.rank_pairs(filter='all')
    print(json.dumps({'mrr': rep.mrr, 'hits': rep.hits, 'macro_mrr': rep.macro_mrr, 'unranked': rep.unranked}), flush=True)

    ratio = same = None
    if not args.skip_baseline:
        base = torch_ranks(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, known)
        ranked = got['bitmap'][0] > 0
        same = float((base == got['bitmap'][0].long())[ranked].double().mean())
        ms = timed(lambda: torch_ranks(z, w, q_rel, tgt_ptr, tgt_u, tgt_v, known), 1, 1, max(2, args.repeats // 2))
        report('torch_composition_filter_all', ms, {'ranks_equal_to_kernel': round(same, 6)})
        ratio = statistics.median(ms) / lines[0]['ms_median']
        print(json.dumps({'torch_composition_over_kernel': round(ratio, 1)}), flush=True)
    if args.write:
        with open(args.write, 'w') as f:
            f.write('# Screen rank: held-out triples of the bundled BioSNAP graph (tools/bench_screen_rank.py)\n\n')
            f.write('Measured on an MI355X, library build %s: %d timings of %d calls each between two device events, after %d '
                    'warm-up calls; median (min .. max) of the timings.\n' % (_lib.build_id(), args.repeats, args.reps, args.warmup))
            f.write('Shape: %s.\n\n| case | ms per call, median | min .. max |\n|---|---|---|\n' % json.dumps(shape))
            for ln in lines:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (ln['case'], ln['ms_median'], ln['ms_min'], ln['ms_max']))
            f.write('\nFiltered MRR %.5f, Hits %s, macro MRR %.5f, unranked %d (self pairs of the held-out set).\n'
                    % (rep.mrr, json.dumps(rep.hits), rep.macro_mrr, rep.unranked))
            if ratio is not None:
                f.write('\nTorch composition over the launches (filter all, bitmap route), medians of this run: %.1f x; share of '
                        'its ranks equal to the kernel\'s: %.6f (it sums each logit in its own order and leaves ties alone).\n'
                        % (ratio, same))


if __name__ == '__main__':
    main()
