"""Time the drug fold-in (`tipk_drug_fold_in`, include/tipk.h section 4k) at BioSNAP size, next to the same result composed from
torch ops on the device -- the only baseline there is.

  python tools/bench_fold_in.py                       M = 1, 64, 4096 new drugs with 3 targets and 0, 8 or 512 interactions each
  python tools/bench_fold_in.py --skip-baseline       without the torch composition
  python tools/bench_fold_in.py --write profiles/fold_in.md   also write the table (the kernel's resources are appended from
                                                      --resources "<text>", e.g. the line of tools/kernel_resources.sh)

Prints one JSON line per measurement: microseconds per call (device events around `--reps` calls after `--warmup`; the torch
composition is timed over max(reps / 5, 1) calls after one).  Inputs: seeded random tables and parameters at the widths of
tip.py (cat: 48 + 16 -> 32 -> 16, 32 bases) over 645 drugs, 1 097 relations and 19 081 proteins -- the launch's time depends
on the shapes and the lists, not on the values.  The torch composition, per layer: XB = table @ basis for all existing drugs
([N, B, d_out]), a gather XB[src] of the listed partners -- the [E_new, B, d_out] temporary --, einsum with att[rel],
`index_add_` into the new drugs' rows, the division by the degree and the root product; the edges go through it in slices of
at most 2^18 so that the temporary stays under 1.1 GB.  fp32 in its own summation order: it agrees with the launch to rounding,
which the tool checks before it times anything."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

DEV = 'cuda:0'
N, R, N_PROT, NE, PD, P, D1, D2, B = 645, 1097, 19081, 48, 16, 16, 32, 16, 32
SLICE = 1 << 18


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


def model_tables(gen):
    rn = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    d0 = NE + PD
    layer1 = (rn(B, d0, D1) / d0 ** 0.5, rn(R, B) / B ** 0.5, rn(d0, D1) / d0 ** 0.5)
    layer2 = (rn(B, D1, D2) * (2.0 / D1), rn(R, B) / B ** 0.5, rn(D1, D2) * (2.0 / D1))
    return rn(N_PROT, P), rn(P, PD) / P ** 0.5, rn(N, d0), torch.relu(rn(N, D1)), layer1, layer2


def new_drugs(m, n_targets, n_edges, gen):
    xd = torch.randn(m, NE, generator=gen).to(DEV)
    tgt = (torch.arange(m + 1, dtype=torch.int64) * n_targets, torch.randint(0, N_PROT, (m * n_targets,), generator=gen, dtype=torch.int32))
    inter = (torch.arange(m + 1, dtype=torch.int64) * n_edges, torch.randint(0, N, (m * n_edges,), generator=gen, dtype=torch.int32),
             torch.randint(0, R, (m * n_edges,), generator=gen, dtype=torch.int32))
    return xd, tuple(t.to(DEV) for t in tgt), tuple(t.to(DEV) for t in inter)


def torch_fold_in(h_prot, hgcn_w, x0, h1, layer1, layer2, xd, targets, interactions, rows_t, rows_e):
    """The same three tensors from torch ops; rows_t / rows_e: the new drug of every target / interaction entry (int64)."""
    m = xd.shape[0]
    t_cnt = (targets[0][1:] - targets[0][:-1]).clamp(min=1).to(torch.float32)
    deg = (interactions[0][1:] - interactions[0][:-1]).clamp(min=1).to(torch.float32)
    mean = torch.zeros(m, h_prot.shape[1], device=xd.device).index_add_(0, rows_t, h_prot[targets[1].long()]) / t_cnt[:, None]
    x0n = torch.cat([xd, mean @ hgcn_w], 1)
    src, rel = interactions[1].long(), interactions[2].long()

    def layer(table, own, basis, att, root):
        xb = torch.einsum('ni,bio->nbo', table, basis)
        out = torch.zeros(m, basis.shape[2], device=xd.device)
        for a in range(0, src.numel(), SLICE):
            sl = slice(a, a + SLICE)
            out.index_add_(0, rows_e[sl], torch.einsum('eb,ebo->eo', att[rel[sl]], xb[src[sl]]))
        return out / deg[:, None] + own @ root

    h1n = torch.relu(layer(x0, x0n, *layer1))
    return x0n, h1n, layer(h1, h1n, *layer2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None)
    ap.add_argument('--resources', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fold_in.py measures on the GPU; none is visible')
    gen = torch.Generator().manual_seed(1)
    tables = model_tables(gen)
    rows = []
    for m in (1, 64, 4096):
        for n_edges in (0, 8, 512):
            xd, tgt, inter = new_drugs(m, 3, n_edges, gen)
            call = lambda: ops.drug_fold_in(*tables, xd, tgt, inter, True)
            got = call()
            rec = {'case': 'fold_in_launch', 'new_drugs': m, 'targets_each': 3, 'interactions_each': n_edges,
                   'us_per_call': round(timed(call, args.reps, args.warmup), 2)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            if args.skip_baseline:
                continue
            rows_t = torch.arange(m, device=DEV).repeat_interleave(3)
            rows_e = torch.arange(m, device=DEV).repeat_interleave(n_edges)
            base = lambda: torch_fold_in(*tables, xd, tgt, inter, rows_t, rows_e)
            want = base()
            for a, b, what in zip(got, want, ('x0', 'h1', 'z')):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4, msg=lambda s: '%s: launch and torch composition differ: %s' % (what, s))
            rec = {'case': 'torch_composition', 'new_drugs': m, 'targets_each': 3, 'interactions_each': n_edges,
                   'us_per_call': round(timed(base, max(args.reps // 5, 1), 1), 2)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    if args.write:
        lines = ['# Drug fold-in at BioSNAP size (tools/bench_fold_in.py)', '',
                 'Measured on an MI355X, library build %s, %d reps after %d warm-up calls (torch composition: %d after 1), device '
                 'events, one run on one device.' % (_lib.build_id(), args.reps, args.warmup, max(args.reps // 5, 1)),
                 'Shape: %s.' % json.dumps({'drugs': N, 'relations': R, 'proteins': N_PROT, 'ne': NE, 'pd': PD, 'p': P, 'd1': D1,
                                            'd2': D2, 'bases': B, 'mod': 'cat'}), '',
                 '| new drugs | targets each | interactions each | launch us | torch composition us | torch / launch |', '|---|---|---|---|---|---|']
        by = {(r['case'], r['new_drugs'], r['interactions_each']): r['us_per_call'] for r in rows}
        for m in (1, 64, 4096):
            for n_edges in (0, 8, 512):
                k, t = by[('fold_in_launch', m, n_edges)], by.get(('torch_composition', m, n_edges))
                lines.append('| %d | 3 | %d | %.2f | %s | %s |' % (m, n_edges, k, '%.2f' % t if t else 'not measured',
                                                                   '%.2f' % (t / k) if t else ''))
        lines.append('')
        for n_edges in (0, 8, 512):
            k, t = by[('fold_in_launch', 4096, n_edges)], by.get(('torch_composition', 4096, n_edges))
            if t:
                lines.append('M = 4096, %d interactions each: the fused launch is %s than the torch composition (%.2f us against %.2f us).'
                             % (n_edges, 'FASTER' if k < t else 'NOT faster', k, t))
        if args.resources:
            lines += ['', '## Kernel resources (tools/kernel_resources.sh)', '', '```', args.resources.strip(), '```']
        with open(os.path.join(ROOT, args.write) if not os.path.isabs(args.write) else args.write, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
