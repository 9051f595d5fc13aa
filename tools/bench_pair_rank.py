"""Time the pair rank (`tipk_distmult_pair_rank`, include/tipk.h section 4f) on the held-out triples of the bundled BioSNAP
graph, next to what the code could do before it: dense scoring through `model.decoder` plus torch filtering, as `pred_topk`
scores.

  python tools/bench_pair_rank.py                  filter 'all': the launch alone on the LDS route and the forced global
                                                   route, `TIP.rank_side_effects` end to end, and the dense baseline
  python tools/bench_pair_rank.py --skip-baseline  without the baseline
  python tools/bench_pair_rank.py --write profiles/pair_rank.md   also write the table

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`).  Inputs: the model
as constructed (initial embeddings, initial decoder weights), the graph's train and test edges.  The baseline scores all R
relations of every test pair in slices through the decoder kernel (fp32, its own arithmetic: its ranks need not agree with
the kernel's where logits are within rounding), masks the pair's known relations with one boolean [P_slice, R] matrix built
from the pair-major lists, and counts per triple the unmasked relations that beat it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

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


def dense_ranks(model, pairs, tgt_ptr, tgt_rel, known, n, max_triples=1 << 24):
    """Filtered ranks by dense scoring: rank int64 [T] in the grouped order of `ops.targets_by_pair`."""
    R = model.data.n_dd_et
    keys, kptr, krel = known
    et_all = torch.arange(R, device=pairs.device)
    ids = et_all[None, :]
    out = torch.empty(tgt_rel.numel(), dtype=torch.int64, device=pairs.device)
    step = max(1, max_triples // R)
    with torch.no_grad():
        for p0 in range(0, pairs.shape[1], step):
            sl = pairs[:, p0:p0 + step]
            m = sl.shape[1]
            s = model.decoder(model.embeddings, sl.repeat_interleave(R, dim=1), et_all.repeat(m)).view(m, R)
            # the pair's known relations as a mask
            pk = torch.minimum(sl[0], sl[1]) * n + torch.maximum(sl[0], sl[1])
            at = torch.searchsorted(keys, pk).clamp(max=keys.numel() - 1)
            rows = torch.nonzero(keys[at] == pk).reshape(-1)
            first, count = kptr[at[rows]], kptr[at[rows] + 1] - kptr[at[rows]]
            owner = torch.repeat_interleave(torch.arange(rows.numel(), device=pairs.device), count)
            within = torch.arange(owner.numel(), device=pairs.device) - torch.repeat_interleave(torch.cumsum(count, 0) - count, count)
            mask = torch.zeros((m, R), dtype=torch.bool, device=pairs.device)
            mask[rows[owner], krel[first[owner] + within].long()] = True
            s = s.masked_fill(mask, float('-inf'))
            # the slice's targets
            a, b = int(tgt_ptr[p0]), int(tgt_ptr[min(p0 + step, pairs.shape[1])])
            t = tgt_rel[a:b].long()
            row = torch.repeat_interleave(torch.arange(m, device=pairs.device), tgt_ptr[p0 + 1:p0 + m + 1] - tgt_ptr[p0:p0 + m])
            st = model.decoder(model.embeddings, sl[:, row], t)
            for c0 in range(0, t.numel(), 65536):                         # [targets, R] comparisons in slabs
                c = slice(c0, c0 + 65536)
                sr = s[row[c]]
                beat = (sr > st[c, None]) | ((sr == st[c, None]) & (ids < t[c, None]))
                beat.scatter_(1, t[c, None], False)
                out[a + c0:a + c0 + beat.shape[0]] = 1 + beat.sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None, help='write the measurements as a markdown table to this file')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_pair_rank times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    dim = z.shape[1]
    pairs, tgt_ptr, tgt_rel, order = ops.targets_by_pair(d.dd_test_idx, d.dd_test_et, n)
    known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, n, extra=(d.dd_test_idx, d.dd_test_range))
    shape = {'triples': tgt_rel.numel(), 'pairs': pairs.shape[1], 'relations': R, 'dim': dim,
             'known_pairs': known[0].numel(), 'known_entries': known[2].numel()}
    print(json.dumps(shape), flush=True)
    lines = []

    def report(name, ms, extra=None):
        line = {'case': name, 'ms': round(ms, 4), 'triples_per_s': round(tgt_rel.numel() / (ms * 1e-3))}
        line.update(extra or {})
        lines.append(line)
        print(json.dumps(line), flush=True)

    got = {}
    for route in ('lds', 'global'):
        _lib.set_option('pair_rank_stream', int(route == 'global'))
        try:
            assert _lib.lib().tipk_distmult_pair_rank_lds_route(dim, R) == int(route == 'lds')
            got[route] = ops.distmult_pair_rank(z, w, pairs, tgt_ptr, tgt_rel, known)
            report('pair_rank_%s_filter_all' % route,
                   timed(lambda: ops.distmult_pair_rank(z, w, pairs, tgt_ptr, tgt_rel, known), args.reps, args.warmup))
        finally:
            _lib.set_option('pair_rank_stream', 0)
    assert torch.equal(got['lds'][0], got['global'][0])
    report('pair_rank_lds_unfiltered', timed(lambda: ops.distmult_pair_rank(z, w, pairs, tgt_ptr, tgt_rel), args.reps, args.warmup))
    report('rank_side_effects_filter_all', timed(lambda: model.rank_side_effects(filter='all'), args.reps, args.warmup))
    rep = model.rank_side_effects(filter='all')
    print(json.dumps({'mrr': rep.mrr, 'hits': rep.hits, 'macro_mrr': rep.macro_mrr, 'unranked': rep.unranked}), flush=True)

    if not args.skip_baseline:
        base = dense_ranks(model, pairs, tgt_ptr, tgt_rel, known, n)
        same = float((base == got['lds'][0].long()).double().mean())
        ms = timed(lambda: dense_ranks(model, pairs, tgt_ptr, tgt_rel, known, n), max(1, args.reps // 10), 1)
        report('dense_decoder_and_torch_filter_all', ms, {'ranks_equal_to_kernel': round(same, 6)})
        ratio = ms / lines[0]['ms']
        print(json.dumps({'baseline_over_kernel': round(ratio, 1)}), flush=True)
    if args.write:
        with open(args.write, 'w') as f:
            f.write('# Pair rank: held-out triples of the bundled BioSNAP graph (tools/bench_pair_rank.py)\n\n')
            f.write('Measured on an MI355X, library build %s, %d reps after %d warm-up calls, device events.\n'
                    % (_lib.build_id(), args.reps, args.warmup))
            f.write('Shape: %s.\n\n| case | ms per call | triples/s |\n|---|---|---|\n' % json.dumps(shape))
            for ln in lines:
                f.write('| %s | %.4f | %d |\n' % (ln['case'], ln['ms'], ln['triples_per_s']))
            if not args.skip_baseline:
                f.write('\nBaseline over kernel (filter all, LDS route): %.1f x; share of baseline ranks equal to the '
                        'kernel\'s: %.6f (the baseline scores with the decoder kernel\'s own arithmetic).\n' % (ratio, same))


if __name__ == '__main__':
    main()
