"""Time the edge attribution (`tipk_rgcn_attribution`, include/tipk.h section 4j) on held-out triples of the bundled BioSNAP
graph, next to the torch composition that answers the same question without the kernel.

  python tools/bench_attribution.py                  Q = 1, 256, 16 384 queries, k = 10: the launch alone on the LDS route and
                                                     on the forced global route, `TIP.explain` end to end, and the torch
                                                     composition
  python tools/bench_attribution.py --skip-baseline  without the torch composition
  python tools/bench_attribution.py --write profiles/attribution.md   also write the table

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`; the torch
composition at Q > 1 is timed over `--reps` / 5 calls after one).  Inputs: the model as constructed (initial parameters; layer 2
is 32 -> 16 with 32 bases), the first Q held-out triples explained on side 'v'.  The torch composition does, per query,
W_r g for ALL relations by two matmuls (basis @ g, then att @ that), a gather of h[src] over the node's in-edges, a row-wise
dot with the gathered W_r g rows, the division by the degree and `topk`: fp32 in its own summation order, so a listed value
may differ from the kernel's in the last bits."""
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


def torch_attribution(h, basis, att, in_edges, ptr_host, nodes_host, probe, k):
    """The k largest contributions per query by the torch composition -> float32 [Q, k], padded with -inf."""
    _, in_src, in_rel = in_edges
    out = torch.full((len(nodes_host), k), float('-inf'), device=h.device)
    for i, v in enumerate(nodes_host):
        e0, e1 = ptr_host[v], ptr_host[v + 1]
        if e1 == e0:
            continue
        wg = att @ (basis @ probe[i])                                    # [R, d_in]: W_r g of every relation
        c = (h[in_src[e0:e1].long()] * wg[in_rel[e0:e1].long()]).sum(1) / (e1 - e0)
        m = min(k, e1 - e0)
        out[i, :m] = torch.topk(c, m)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--queries', type=int, nargs='+', default=[1, 256, 16384])
    ap.add_argument('--skip-baseline', action='store_true')
    ap.add_argument('--write', default=None, help='write the measurements as a markdown table to this file')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_attribution times the device: no GPU visible'
    from tip_amd.layers import TIP, Setting
    torch.manual_seed(0)
    model = TIP(Setting(), torch.device(DEV), data_path=None)
    d, k = model.data, args.k
    n, R = d.n_drug, d.n_dd_et
    with torch.no_grad():
        h, z = model.encoder.encode_layers(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, d.p_feat,
                                           d.pp_train_indices, d.dp_edge_index, d.dp_range_list)
    r2 = model.encoder.rgcn2
    basis, att, root = r2.basis.detach(), r2.att.detach(), r2.root.detach()
    in_edges = ops.in_edges_by_node(d.dd_train_idx, d.dd_train_range, n)
    ptr_host = in_edges[0].tolist()
    deg = in_edges[0][1:] - in_edges[0][:-1]
    n_bases, d_in, d_out = basis.shape
    shape = {'drugs': n, 'relations': R, 'bases': n_bases, 'd_in': d_in, 'd_out': d_out, 'train_edges': in_edges[1].numel(),
             'max_degree': int(deg.max()), 'k': k}
    print(json.dumps(shape), flush=True)
    lines = []

    def report(name, q, ms, extra=None):
        line = {'case': name, 'queries': q, 'ms': round(ms, 4), 'us_per_query': round(ms * 1e3 / q, 3)}
        line.update(extra or {})
        lines.append(line)
        print(json.dumps(line), flush=True)

    words = []
    for Q in args.queries:
        idx, et = d.dd_test_idx[:, :Q], d.dd_test_et[:Q]
        node, probe, _ = model.decoder.probe(z, idx, et, 'v')
        nodes_host = node.tolist()
        edges = int(deg[node].sum())
        flop = 2 * (Q * (n_bases * d_in * d_out + n * n_bases * d_in) + edges * n_bases)

        def launch():
            return ops.rgcn_edge_attribution(h, basis, att, root, in_edges, node, probe, k)

        got = {}
        for route in ('lds', 'global'):
            _lib.set_option('attribution_global', int(route == 'global'))
            try:
                assert _lib.lib().tipk_rgcn_attribution_lds_route(n, n_bases) == int(route == 'lds')
                got[route] = launch()
                ms = timed(launch, args.reps, args.warmup)
                report('attribution_%s' % route, Q, ms, {'edges': edges, 'gflops': round(flop / (ms * 1e-3) / 1e9, 1)})
            finally:
                _lib.set_option('attribution_global', 0)
        assert all(torch.equal(a, b) for a, b in zip(got['lds'], got['global']))
        report('explain_end_to_end', Q, timed(lambda: model.explain((idx, et), k=k, side='v'), args.reps, args.warmup))
        if not args.skip_baseline:
            fn = lambda: torch_attribution(h, basis, att, in_edges, ptr_host, nodes_host, probe, k)
            base = fn()
            listed = torch.isfinite(base)
            assert torch.equal(listed, torch.isfinite(got['lds'][0]))
            off = float((base[listed] - got['lds'][0][listed]).abs().max()) if bool(listed.any()) else 0.0
            ms = timed(fn, args.reps if Q == 1 else max(1, args.reps // 5), args.warmup if Q == 1 else 1)
            report('torch_composition', Q, ms, {'max_abs_difference_of_listed_values': off})
            kernel = next(ln['ms'] for ln in lines if ln['case'] == 'attribution_lds' and ln['queries'] == Q)
            words.append('Q = %d: torch composition %.4f ms, launch (LDS route) %.4f ms: the launch is %s (%.1f x).'
                         % (Q, ms, kernel, 'not slower' if kernel <= ms else 'SLOWER', ms / kernel))
            print(json.dumps({'queries': Q, 'torch_composition_over_kernel': round(ms / kernel, 2)}), flush=True)
    if args.write:
        with open(args.write, 'w') as f:
            f.write('# Edge attribution: held-out triples of the bundled BioSNAP graph (tools/bench_attribution.py)\n\n')
            f.write('Measured on an MI355X, library build %s, %d reps after %d warm-up calls, device events, one run on one '
                    'device.\n' % (_lib.build_id(), args.reps, args.warmup))
            f.write('Shape: %s.\n\n| case | queries | ms per call | us per query |\n|---|---|---|---|\n' % json.dumps(shape))
            for ln in lines:
                f.write('| %s | %d | %.4f | %.3f |\n' % (ln['case'], ln['queries'], ln['ms'], ln['us_per_query']))
            f.write('\n' + '\n'.join(words) + '\n')


if __name__ == '__main__':
    main()
