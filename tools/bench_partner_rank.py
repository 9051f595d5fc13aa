"""Time the partner rank (`tipk_distmult_partner_rank`, include/tipk.h section 4g) on the held-out triples of the bundled
BioSNAP graph, next to the torch composition that answers the same question without the kernel.

  python tools/bench_partner_rank.py                  filter 'all': the launch alone on the LDS route and the forced global
                                                      route, the unfiltered launch, `TIP.rank_partners` end to end, and
                                                      the torch composition
  python tools/bench_partner_rank.py --skip-baseline  without the torch composition
  python tools/bench_partner_rank.py --write profiles/partner_rank.md   also write the table

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`).  Inputs: the model
as constructed (initial embeddings, initial decoder weights; dim 16), the graph's train and test edges.  The torch
composition forms the logits of a slice of queries as A @ z.T with A = z[u] * w[r] (fp32, its own summation order: its
ranks need not agree with the kernel's where logits are within rounding), masks each query's known partners -- forward and
reverse keys of its relation -- and the queried drug itself with one boolean [Q_slice, n] matrix built by searchsorted in the
relation-major keys, and counts per triple the unmasked drugs that beat it."""
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


def torch_ranks(z, w, q_rel, q_drug, tgt_ptr, tgt_node, known, max_logits=1 << 25):
    """Filtered ranks by the torch composition: rank int64 [T] in the grouped order of `ops.targets_by_query`."""
    n = z.shape[0]
    keys, kptr = known
    rel = torch.repeat_interleave(torch.arange(kptr.numel() - 1, device=z.device), kptr[1:] - kptr[:-1])
    comb = rel * (n * n) + keys                                           # ascending: relation-major, sorted inside
    ids = torch.arange(n, device=z.device)[None, :]
    out = torch.empty(tgt_node.numel(), dtype=torch.int64, device=z.device)
    step = max(1, max_logits // n)
    for q0 in range(0, q_rel.numel(), step):
        r, u = q_rel[q0:q0 + step].long(), q_drug[q0:q0 + step].long()
        m = r.numel()
        s = (z[u] * w[r]) @ z.t()                                         # [m, n]
        mask = ids == u[:, None]
        for probe in (u[:, None] * n + ids, ids * n + u[:, None]):
            probe = r[:, None] * (n * n) + probe
            at = torch.searchsorted(comb, probe).clamp(max=comb.numel() - 1)
            mask |= comb[at] == probe
        a, b = int(tgt_ptr[q0]), int(tgt_ptr[min(q0 + step, q_rel.numel())])
        t = tgt_node[a:b].long()
        row = torch.repeat_interleave(torch.arange(m, device=z.device), tgt_ptr[q0 + 1:q0 + m + 1] - tgt_ptr[q0:q0 + m])
        st = s[row, t]
        s = s.masked_fill(mask, float('-inf'))
        for c0 in range(0, t.numel(), 65536):                             # [targets, n] comparisons in slabs
            c = slice(c0, c0 + 65536)
            sr = s[row[c]]
            beat = (sr > st[c, None]) | ((sr == st[c, None]) & (ids < t[c, None]))
            beat.scatter_(1, t[c, None], False)
            out[a + c0:a + c0 + beat.shape[0]] = 1 + beat.sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None, help='write the measurements as a markdown table to this file')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_partner_rank times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting, _screen_known
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d = model.data
    n, R = d.n_drug, d.n_dd_et
    z, w = model.embeddings.detach(), model.decoder.weight.detach()
    dim = z.shape[1]
    q_rel, q_drug, tgt_ptr, tgt_node, order = ops.targets_by_query(d.dd_test_idx, d.dd_test_et, n)
    known = _screen_known(d, 'all')
    shape = {'triples': tgt_node.numel(), 'queries': q_rel.numel(), 'drugs': n, 'relations': R, 'dim': dim,
             'known_keys': known[0].numel()}
    print(json.dumps(shape), flush=True)
    lines = []

    def report(name, ms, extra=None):
        line = {'case': name, 'ms': round(ms, 4), 'triples_per_s': round(tgt_node.numel() / (ms * 1e-3))}
        line.update(extra or {})
        lines.append(line)
        print(json.dumps(line), flush=True)

    def launch(kn=known):
        return ops.distmult_partner_rank(z, w, q_rel, q_drug, tgt_ptr, tgt_node, kn)

    got = {}
    for route in ('lds', 'global'):
        _lib.set_option('partner_rank_global', int(route == 'global'))
        try:
            assert _lib.lib().tipk_distmult_partner_rank_lds_route(n, dim) == int(route == 'lds')
            got[route] = launch()
            report('partner_rank_%s_filter_all' % route, timed(launch, args.reps, args.warmup))
        finally:
            _lib.set_option('partner_rank_global', 0)
    assert torch.equal(got['lds'][0], got['global'][0])
    report('partner_rank_lds_unfiltered', timed(lambda: launch(None), args.reps, args.warmup))
    report('rank_partners_filter_all', timed(lambda: model.rank_partners(filter='all'), args.reps, args.warmup))
    rep = model.rank_partners(filter='all')
    print(json.dumps({'mrr': rep.mrr, 'hits': rep.hits, 'macro_mrr': rep.macro_mrr, 'unranked': rep.unranked}), flush=True)

    if not args.skip_baseline:
        base = torch_ranks(z, w, q_rel, q_drug, tgt_ptr, tgt_node, known)
        same = float((base == got['lds'][0].long()).double().mean())
        ms = timed(lambda: torch_ranks(z, w, q_rel, q_drug, tgt_ptr, tgt_node, known), max(1, args.reps // 5), 1)
        report('torch_composition_filter_all', ms, {'ranks_equal_to_kernel': round(same, 6)})
        ratio = ms / lines[0]['ms']
        print(json.dumps({'torch_composition_over_kernel': round(ratio, 1)}), flush=True)
    if args.write:
        with open(args.write, 'w') as f:
            f.write('# Partner rank: held-out triples of the bundled BioSNAP graph (tools/bench_partner_rank.py)\n\n')
            f.write('Measured on an MI355X, library build %s, %d reps after %d warm-up calls, device events.\n'
                    % (_lib.build_id(), args.reps, args.warmup))
            f.write('Shape: %s.\n\n| case | ms per call | triples/s |\n|---|---|---|\n' % json.dumps(shape))
            for ln in lines:
                f.write('| %s | %.4f | %d |\n' % (ln['case'], ln['ms'], ln['triples_per_s']))
            if not args.skip_baseline:
                f.write('\nTorch composition over kernel (filter all, LDS route), measured in this run: %.1f x; share of its '
                        'ranks equal to the kernel\'s: %.6f (it sums each logit in its own order).\n' % (ratio, same))


if __name__ == '__main__':
    main()
