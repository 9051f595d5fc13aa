"""Time the side-effect fit (`tipk_distmult_fit`, include/tipk.h section 4m) at BioSNAP size (645 drugs, dim 16), next to the
same Newton iteration composed from torch ops on the device -- the only baseline there is.

  python tools/bench_side_effect_fit.py                     n_fit = 1, 64, 1097 with 250, 4 000 and 30 000 listed pairs each
  python tools/bench_side_effect_fit.py --skip-baseline     without the torch composition
  python tools/bench_side_effect_fit.py --write profiles/side_effect_fit.md [--resources "<text>"] [--errlog <file>]
      writes the table, the per-row verdicts, the C_FIT section (with --errlog) and the resource lines (with --resources);
      whatever the file holds from the line "## Notes (written by hand ..." on is kept as it is

Prints one JSON line per measurement, microseconds (device events around `--reps` calls after `--warmup`; the torch
composition over max(reps / 5, 1) calls after one):
  evaluation   one (statistics, step) pair: (a fit of 8 iterations - a fit of 0 iterations) / 8 with gtol = 0, so that no
               relation goes inactive;
  fit          `ops.distmult_fit` with its defaults (max_iter 16, gtol 1e-5): all 17 pairs are enqueued, a relation that has
               converged costs its workgroups an early return.
The torch composition: the features F of the n (n + 1) / 2 unordered pairs and their outer products formed ONCE (not timed);
per evaluation the batched F @ w^T, sigmoid / softplus, the weighted sums for g and F^T diag(h) F for all relations, the
correction on the listed pairs by index_add_ (their outer products in slices of 2^20), then torch.linalg.cholesky / cholesky_solve and a full Newton step (no line
search: one test less than the fused step does).  It runs as many evaluations as the fused fit needed at most.  Lists: uniform
random pairs (the time depends on shapes and list lengths, not on the values); z seeded normal, std 0.5."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

DEV = 'cuda:0'
NOTES = '## Notes (written by hand'                      # --write keeps the file from this heading on
N, DIM, L2 = 645, 16, 1e-4
FITS, PAIRS = (1, 64, 1097), (250, 4000, 30000)
SLICE = 1 << 20


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
    return t0.elapsed_time(t1) * 1000.0 / reps


class TorchFit(object):
    """The composition: everything that does not depend on w is formed here, once."""

    def __init__(self, z, fp):
        iu, iv = torch.triu_indices(N, N, device=DEV)
        self.f = z[iu] * z[iv]                                           # [M, dim]
        self.ff = (self.f[:, :, None] * self.f[:, None, :]).reshape(-1, DIM * DIM)
        self.m = torch.where(iu == iv, 1.0, 2.0).to(DEV)
        self.dense = fp.dense_w.to(DEV)
        self.b = self.dense.numel()
        ptr = fp.ptr.to(DEV)
        self.rel = torch.repeat_interleave(torch.arange(self.b, device=DEV), ptr[1:] - ptr[:-1])
        self.fs = z[fp.u.to(DEV).long()] * z[fp.v.to(DEV).long()]
        self.wpos, self.wneg = fp.wpos.to(DEV), fp.wneg.to(DEV)
        self.eye = torch.eye(DIM, device=DEV)

    def stats(self, w):
        s = self.f @ w.t()                                               # [M, B]
        sg = torch.sigmoid(s)
        cm = self.m[:, None] * self.dense[None, :]
        loss = (cm * torch.nn.functional.softplus(s)).sum(0)
        g = (cm * sg).t() @ self.f
        h = (cm * sg * (1 - sg)).t() @ self.ff
        ss = (self.fs * w[self.rel]).sum(1)
        sgs = torch.sigmoid(ss)
        loss = loss.index_add(0, self.rel, self.wpos * torch.nn.functional.softplus(-ss) - self.wneg * torch.nn.functional.softplus(ss))
        g = g.index_add(0, self.rel, (-self.wpos * (1 - sgs) - self.wneg * sgs)[:, None] * self.fs)
        ch = (self.wpos - self.wneg) * sgs * (1 - sgs)
        for a in range(0, ss.numel(), SLICE):                            # the listed pairs' outer products, 2^20 at a time
            sl = slice(a, a + SLICE)
            h.index_add_(0, self.rel[sl], (ch[sl, None, None] * self.fs[sl, :, None] * self.fs[sl, None, :]).reshape(-1, DIM * DIM))
        return (loss + 0.5 * L2 * (w * w).sum(1), g + L2 * w, h.reshape(self.b, DIM, DIM) + L2 * self.eye)

    def fit(self, evaluations):
        w = torch.zeros((self.b, DIM), device=DEV)
        for _ in range(evaluations):
            loss, g, h = self.stats(w)
            w = w - torch.cholesky_solve(g[:, :, None], torch.linalg.cholesky(h))[:, :, 0]
        return w


def lists(b, count, gen):
    idx = torch.randint(0, N, (2, b * count), generator=gen)
    return idx, torch.arange(b + 1, dtype=torch.int64) * count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None)
    ap.add_argument('--resources', default=None)
    ap.add_argument('--errlog', default=None, help='the TIPK_ERRLOG file of a run of tests/test_gpu_side_effect_fit.py')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_side_effect_fit.py measures on the GPU; none is visible')
    gen = torch.Generator().manual_seed(1)
    z = (torch.randn(N, DIM, generator=gen) * 0.5).to(DEV)
    rows = []
    for b in FITS:
        for count in PAIRS:
            fp = ops.fit_pairs_csr(lists(b, count, gen), N)
            fp = fp._replace(**{k: getattr(fp, k).to(DEV) for k in ('ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w')})
            w, loss, grad, info = ops.distmult_fit(z, fp, L2)
            evals = int(info[:, 1].max())
            rec = {'n_fit': b, 'pairs_each': count, 'distinct_pairs': int(fp.u.numel()), 'evaluations_max': evals,
                   'converged': int((info[:, 0] == 1).sum())}
            t0 = timed(lambda: ops.distmult_fit(z, fp, L2, None, 0, 0.0), args.reps, args.warmup)
            t8 = timed(lambda: ops.distmult_fit(z, fp, L2, None, 8, 0.0), args.reps, args.warmup)
            rec['fused_evaluation_us'] = round((t8 - t0) / 8, 2)
            rec['fused_fit_us'] = round(timed(lambda: ops.distmult_fit(z, fp, L2), args.reps, args.warmup), 2)
            if not args.skip_baseline:
                tf = TorchFit(z, fp)
                probe = torch.randn(b, DIM, generator=gen).to(DEV) * 0.3
                for a, c, what in zip(ops.distmult_fit_stats(z, probe, fp, L2), tf.stats(probe), ('loss', 'grad', 'hess')):
                    torch.testing.assert_close(a, c, rtol=2e-3, atol=1e-5, msg=lambda s: '%s: launch and torch composition differ: %s' % (what, s))
                rec['rows_max_diff'] = float((tf.fit(evals) - w).abs().max())
                reps = max(args.reps // 5, 1)
                one = timed(lambda: tf.fit(1), reps, 1)
                rec['torch_evaluation_us'] = round(one, 2)
                rec['torch_fit_us'] = round(timed(lambda: tf.fit(evals), reps, 1), 2)
                del tf
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    if args.write:
        lines = ['# Side-effect fit at BioSNAP size (tools/bench_side_effect_fit.py)', '',
                 'Measured on an MI355X, library build %s, %d reps after %d warm-up calls (torch composition: %d after 1), device '
                 'events, one run on one device.' % (_lib.build_id(), args.reps, args.warmup, max(args.reps // 5, 1)),
                 'Shape: %d drugs, dim %d, l2 %g, uniform random lists; the fused figures include the Python op (argument checks, '
                 'five allocations).  "evaluation" = one (statistics, step) pair; "fit" = `ops.distmult_fit` with its defaults '
                 '(17 pairs enqueued) against as many torch Newton steps as the fused fit needed at most.' % (N, DIM, L2), '',
                 '| n_fit | pairs each | evaluations | fused evaluation us | torch evaluation us | fused fit us | torch fit us | faster (fit) |',
                 '|---|---|---|---|---|---|---|---|']
        for r in rows:
            t = 'torch_fit_us' in r
            lines.append('| %d | %d | %d | %.2f | %s | %.2f | %s | %s |' % (
                r['n_fit'], r['pairs_each'], r['evaluations_max'], r['fused_evaluation_us'],
                '%.2f' % r['torch_evaluation_us'] if t else 'not measured', r['fused_fit_us'],
                '%.2f' % r['torch_fit_us'] if t else 'not measured',
                ('fused' if r['fused_fit_us'] < r['torch_fit_us'] else 'TORCH') if t else ''))
        lines.append('')
        for r in rows:
            if 'torch_fit_us' in r:
                ev = 'fused' if r['fused_evaluation_us'] < r['torch_evaluation_us'] else 'torch'
                ft = 'fused' if r['fused_fit_us'] < r['torch_fit_us'] else 'torch'
                lines.append('n_fit = %d, %d pairs each: per evaluation the %s side is faster (%.2f us fused, %.2f us torch); per fit the '
                             '%s side (%.2f us fused, %.2f us torch); %d of %d relations converged.'
                             % (r['n_fit'], r['pairs_each'], ev, r['fused_evaluation_us'], r['torch_evaluation_us'], ft,
                                r['fused_fit_us'], r['torch_fit_us'], r['converged'], r['n_fit']))
        if args.errlog and os.path.exists(args.errlog):
            seen = [json.loads(line) for line in open(args.errlog) if line.strip()]
            seen = [s for s in seen if s.get('what') == 'fit stats c']
            if seen:
                worst = max(seen, key=lambda s: s['observed_c'])
                lines += ['', '## C_FIT (tests/fit_spec.py)', '',
                          'Largest excess (|X32 - X64| - T) / (U A) - D over the %d checks of tests/test_gpu_side_effect_fit.py with '
                          'TIPK_ERRLOG set: %.2f (case "%s", D = %d).' % (len(seen), worst['observed_c'], worst['case'], worst['d_chain']),
                          'A negative excess means the error stayed below D U A alone: the rule "at most 30 x the largest excess and '
                          'not below 4" gives C_FIT = %g.' % max(4.0, 30 * worst['observed_c'])]
        if args.resources:
            lines += ['', '## Kernel resources (tools/kernel_resources.sh)', '', '```', args.resources.strip(), '```']
        path = os.path.join(ROOT, args.write) if not os.path.isabs(args.write) else args.write
        if os.path.exists(path):
            old = open(path).read().rstrip('\n').split('\n')
            at = [i for i, line in enumerate(old) if line.startswith(NOTES)]
            if at:
                lines += [''] + old[at[0]:]
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
