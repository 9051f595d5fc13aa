"""Time the protein attribution (`tipk_protein_attribution`, include/tipk.h section 4o) on held-out triples of the bundled
BioSNAP graph, next to the torch composition that answers the same question without the kernels.

  python tools/bench_protein_attribution.py                  Q = 1, 256, 4 096 queries, k = 10: `ops.protein_attribution` (the
                                                             entry, pair cells and workspace allocation included),
                                                             `TIP.explain_proteins` end to end, and the torch composition
  python tools/bench_protein_attribution.py --skip-baseline  without the torch composition
  python tools/bench_protein_attribution.py --write profiles/protein_attribution.md   also write the table

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`; the torch composition
at Q > 1 is timed over ONE call after one warm-up call of 8 queries).  Inputs: the model as constructed (initial parameters),
the first Q held-out triples explained on side 'v'.  The torch composition runs the package's own R-GCN layers (their autograd
nodes, HIP kernels forward and backward) on x0 rebuilt with torch ops from the protein embeddings and the drug rows, ONE
forward pass, then per query one autograd backward of probe . z[v] through both layers and gradient x input summed per
protein, and `topk`: fp32 in autograd's summation order, so a listed value differs from the kernel's in the last bits."""
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


def torch_composition(model, h_prot, xe, nodes, probe, k, cand):
    """(contrib [Q, k], protein [Q, k], features [Q], proteins [Q]) by autograd through the package's layers."""
    d, enc = model.data, model.encoder
    n, n_prot = d.n_drug, d.n_prot
    prot, drug = d.dp_edge_index[0], d.dp_edge_index[1] - n_prot
    cnt = torch.bincount(drug, minlength=n).clamp(min=1).to(torch.float32)
    hp, x = h_prot.detach().clone().requires_grad_(), xe.detach().clone().requires_grad_()
    pd = torch.zeros(n, enc.hgcn.out_dim, device=hp.device).index_add_(0, drug, hp[prot] @ enc.hgcn.weight.detach()) / cnt[:, None]
    x0 = torch.cat([x, pd], 1) if enc.mod == 'cat' else x + pd
    hid = torch.relu(enc.rgcn1(x0, d.dd_train_idx, d.dd_train_et, d.dd_train_range))
    z = enc.rgcn2(hid, d.dd_train_idx, d.dd_train_et, d.dd_train_range)
    Q = nodes.numel()
    out_c = torch.empty((Q, k), device=hp.device)
    out_p = torch.empty((Q, k), dtype=torch.int64, device=hp.device)
    feat, total = torch.empty(Q, device=hp.device), torch.empty(Q, device=hp.device)
    for i in range(Q):
        g_hp, g_x = torch.autograd.grad((probe[i] * z[nodes[i]]).sum(), (hp, x), retain_graph=True)
        c = (g_hp * hp.detach()).sum(1)
        feat[i], total[i] = (g_x * x.detach()).sum(), c.sum()
        out_c[i], out_p[i] = torch.topk(torch.where(cand, c, torch.full_like(c, float('-inf'))), k)
    return out_c, out_p, feat, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--queries', type=int, nargs='+', default=[1, 256, 4096])
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None, help='write the measurements as a markdown table to this file')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_protein_attribution times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d, enc, k = model.data, model.encoder, args.k
    n, n_prot = d.n_drug, d.n_prot
    enc_args = (d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, d.p_feat, d.pp_train_indices,
                d.dp_edge_index, d.dp_range_list)
    with torch.no_grad():
        h_prot, x0, h = enc.fold_in_tables(*enc_args)
        z = enc.encode_layers(*enc_args)[1]
    r1, r2 = enc.rgcn1, enc.rgcn2
    ne, cat = enc.embed.shape[1], enc.mod == 'cat'
    assert cat, 'the bundled model is built in cat mode'
    xe = x0[:, :ne]
    layer1 = (r1.basis.detach(), r1.att.detach(), r1.root.detach())
    layer2 = (r2.basis.detach(), r2.att.detach(), r2.root.detach())
    pair = ops.in_edges_by_pair(d.dd_train_idx, d.dd_train_range, n)
    targets = ops.targets_by_protein(d.dp_edge_index, n_prot, n)
    cand = (targets[0][1:] - targets[0][:-1]) > 0
    B, d0, d1 = layer1[0].shape
    p = h_prot.shape[1]
    shape = {'drugs': n, 'proteins': n_prot, 'targeted_proteins': int(cand.sum()), 'p_d_edges': int(targets[1].numel()),
             'relations': d.n_dd_et, 'bases': B, 'd0': d0, 'd1': d1, 'd2': layer2[0].shape[2], 'p': p,
             'train_edges': int(pair[1].numel()), 'k': k,
             'workspace_MiB_at_256': round(ops.protein_attribution_workspace_bytes(n, B, d1, p, 256) / 2 ** 20, 1)}
    print(json.dumps(shape), flush=True)
    lines, words = [], []

    def report(name, q, ms, extra=None):
        line = {'case': name, 'queries': q, 'ms': round(ms, 4), 'us_per_query': round(ms * 1e3 / q, 3)}
        line.update(extra or {})
        lines.append(line)
        print(json.dumps(line), flush=True)

    for Q in args.queries:
        idx, et = d.dd_test_idx[:, :Q], d.dd_test_et[:Q]
        node, probe, _ = model.decoder.probe(z, idx, et, 'v')
        flop = 2 * Q * (n * n * B * d1 + n * d0 * (B * d1 + d1) + n * B * d1)

        def entry():
            return ops.protein_attribution(h_prot, enc.hgcn.weight.detach(), xe, h, layer1, layer2, pair, targets, cat, node, probe, k)

        got = entry()
        ms = timed(entry, args.reps, args.warmup)
        report('protein_attribution', Q, ms, {'gflops': round(flop / (ms * 1e-3) / 1e9, 1)})
        report('explain_proteins_end_to_end', Q, timed(lambda: model.explain_proteins((idx, et), k=k, side='v'), args.reps, args.warmup))
        if not args.skip_baseline:
            fn = lambda: torch_composition(model, h_prot, xe, node, probe, k, cand)
            torch_composition(model, h_prot, xe, node[:8], probe[:8], k, cand)           # warm-up: plans, allocator
            base = fn()
            scale = float(got[0].abs().max())
            off = float((base[0] - got[0]).abs().max())
            tot = float((base[2] + base[3] - got[3] - got[4]).abs().max())
            ms_b = timed(fn, args.reps if Q == 1 else 1, args.warmup if Q == 1 else 0)
            report('torch_composition', Q, ms_b, {'max_abs_difference_of_listed_values': off, 'largest_listed_value': scale,
                                                  'max_abs_difference_of_totals': tot})
            words.append('Q = %d: torch composition %.3f ms, entry (cells included) %.3f ms: the entry is %s (%.1f x).'
                         % (Q, ms_b, ms, 'not slower' if ms <= ms_b else 'SLOWER', ms_b / ms))
            print(json.dumps({'queries': Q, 'torch_composition_over_entry': round(ms_b / ms, 2)}), flush=True)
    if args.write:
        with open(args.write, 'w') as f:
            f.write('# Protein attribution: held-out triples of the bundled BioSNAP graph (tools/bench_protein_attribution.py)\n\n')
            f.write('Measured on an MI355X, library build %s, %d reps after %d warm-up calls (the torch composition at Q > 1: one '
                    'call), device events, one run on one device.  Every number in the table was measured in that run; nothing '
                    'else was (no counters, no per-kernel split).\n' % (_lib.build_id(), args.reps, args.warmup))
            f.write('Shape: %s.\n\n| case | queries | ms per call | us per query |\n|---|---|---|---|\n' % json.dumps(shape))
            for ln in lines:
                f.write('| %s | %d | %.4f | %.3f |\n' % (ln['case'], ln['queries'], ln['ms'], ln['us_per_query']))
            f.write('\n' + '\n'.join(words if words else ['The torch composition was not measured in this run.']) + '\n')


if __name__ == '__main__':
    main()
