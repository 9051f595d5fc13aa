"""Time the combination burden (`tipk_distmult_combo_burden`, include/tipk.h section 4n) on the device, next to the same
quantity from chunked torch ops, in the same run, over the bundled BioSNAP graph's model (645 drugs, 1 097 relations, dim 16).

  python tools/bench_combination_risk.py             the four shapes below: the entry (default route, prefix reuse off, the
                                                     NN decoder's tables), `TIP.combination_risk` end to end and the torch
                                                     composition, the entry and the composition ALTERNATED in one loop
  python tools/bench_combination_risk.py --random    random z / rel_w of that shape (no data set needed; no end-to-end line)
  python tools/bench_combination_risk.py --only 4x16 --entry-only --calls 20
                                                     nothing but `--calls` entry calls of one shape: the program to put behind
                                                     `rocprofv3 --kernel-trace --stats --` for the time of each of the three launches

Shapes: deprescribe10 (ten slots [d, -1]: 1 024 combinations), 3x12 (3 slots of 12 alternatives + 4 fixed drugs), 4x16 (4
slots of 16 + 3 fixed: 65 536 combinations), 256x3x8 (256 queries of 3 slots of 8 + 2 fixed in one call).

Prints one JSON line per measurement: the median ms per call over `--rounds` rounds (device events around each call), the
spread (min, max), combinations per second and, for the entry, the bytes the burden launch reads per combination -- computed
from the shapes: rows read x n_rel x 4, with and without prefix reuse -- over the measured time as a share of the 34.5 TB/s
the L2s deliver (that time also holds the tables and the selection, so the share is a lower bound).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

L2_RATE = 34.5e12
DEV = 'cuda:0'


def shapes(n, g):
    p = lambda m: torch.randperm(n, generator=g)[:m].tolist()
    out = {}
    d = p(10)
    out['deprescribe10'] = [([], [[x, -1] for x in d])]
    d = p(40)
    out['3x12'] = [(d[36:40], [d[0:12], d[12:24], d[24:36]])]
    d = p(67)
    out['4x16'] = [(d[64:67], [d[16 * s:16 * s + 16] for s in range(4)])]
    qs = []
    for _ in range(256):
        d = p(26)
        qs.append((d[24:26], [d[8 * s:8 * s + 8] for s in range(3)]))
    out['256x3x8'] = qs
    return out


def lists_of(queries):
    fix, fptr, alt, aptr, sptr = [], [0], [], [0], [0]
    for fixed, slots in queries:
        fix += fixed
        fptr.append(len(fix))
        for s in slots:
            alt += s
            aptr.append(len(alt))
        sptr.append(len(aptr) - 1)
    return fix, fptr, alt, aptr, sptr


def rows_read(queries, run, prefix):
    """Workspace rows the burden launch reads, from the shapes: a combination reads 1 + S (S + 1) / 2 rows (fewer with -1
    alternatives or without fixed drugs: counted as if all were there), S when it continues a prefix."""
    total, g = 0, 0
    for fixed, slots in queries:
        S = len(slots)
        full, last, count = 1 + S * (S + 1) // 2, (len(slots[-1]) if S else 1), 1
        for s in slots:
            count *= len(s)
        if not prefix or S < 2:
            total += count * full
        else:
            for c in range(count):
                total += full if (c % last == 0 or (g + c) % run == 0) else S
        g += count
    return total


def composition(z, w, queries, chunk_bytes=1 << 28):
    """The same burdens from torch ops: per query the regimen of every combination, its pairs gathered, the logits
    [C_chunk, pairs, R] materialised in chunks, softplus summed over the pairs, 1 - exp(-A) summed over the relations; NaN
    where a drug is taken twice.  Noisy-or, no known filter, no weights."""
    out = []
    R = w.shape[0]
    for fixed, slots in queries:
        combos = torch.cartesian_prod(*[torch.tensor(s, device=DEV) for s in slots]).reshape(-1, len(slots)) if slots \
            else torch.zeros((1, 0), dtype=torch.int64, device=DEV)
        C, m = combos.shape[0], len(fixed)
        ids = torch.cat([torch.tensor(fixed, dtype=torch.int64, device=DEV)[None, :].expand(C, m), combos], 1)
        i, j = torch.triu_indices(ids.shape[1], ids.shape[1], offset=1, device=DEV)
        step = max(1, chunk_bytes // (max(i.numel(), 1) * R * 4))
        for c0 in range(0, C, step):
            a, b = ids[c0:c0 + step][:, i], ids[c0:c0 + step][:, j]
            there = (a >= 0) & (b >= 0)
            h = z[a.clamp(min=0)] * z[b.clamp(min=0)]                     # [c, P, dim]
            sp = torch.nn.functional.softplus(h @ w.t()) * there[:, :, None]
            burden = (-torch.expm1(-sp.sum(1))).sum(1)
            out.append(torch.where((there & (a == b)).any(1), torch.full_like(burden, float('nan')), burden))
    return torch.cat(out)


def one(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def measure(fns, rounds, warmup):
    """The contenders alternated: every round calls each once -> {name: (median, min, max) ms}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(one(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--entry-only', action='store_true')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--random', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_combination_risk times the device: no GPU visible'
    g = torch.Generator().manual_seed(1)
    model = None
    if args.random:
        n, R, dim = 645, 1097, 16
        z, w = (torch.randn(n, dim, generator=g) / 2).to(DEV), (torch.randn(R, dim, generator=g) / 2).to(DEV)
    else:
        from tip_amd.layers import TIP, Setting
        torch.manual_seed(0)
        model = TIP(Setting(), torch.device(DEV), data_path=None)
        n, R = model.data.n_drug, model.data.n_dd_et
        z, w = model.embeddings.detach(), model.decoder.weight.detach()
        dim = z.shape[1]
    s1, s2 = torch.randn(n, R, generator=g).to(DEV), torch.randn(n, R, generator=g).to(DEV)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count

    for name, queries in shapes(n, g).items():
        if args.only and name != args.only:
            continue
        plan = ops.combo_plan(*lists_of(queries), DEV)
        entry = lambda: ops.distmult_combo_burden(z, w, plan, args.k, 'noisy_or')
        if args.entry_only:
            for _ in range(args.calls):
                entry()
            torch.cuda.synchronize()
            print(json.dumps({'case': name, 'calls': args.calls, 'combinations': plan.n_comb, 'table_rows': plan.n_rows}))
            continue

        def no_prefix():
            _lib.set_option('combo_no_prefix', 1)
            try:
                return ops.distmult_combo_burden(z, w, plan, args.k, 'noisy_or')
            finally:
                _lib.set_option('combo_no_prefix', 0)

        fns = {'entry': entry, 'entry_no_prefix': no_prefix,
               'entry_k0': lambda: ops.distmult_combo_burden(z, w, plan, 0, 'noisy_or'),
               'entry_max': lambda: ops.distmult_combo_burden(z, w, plan, args.k, 'max'),
               'entry_tables_nn': lambda: ops.pair_table_combo_burden(s1, s2, plan, args.k, 'noisy_or'),
               'torch_composition': lambda: composition(z, w, queries)}
        if model is not None:
            slots, fixed = [q[1] for q in queries], [q[0] for q in queries]
            fns['tip_combination_risk'] = lambda: model.combination_risk(slots, fixed=fixed, k=args.k)
        res = measure(fns, args.rounds, args.warmup)
        ref, got = entry()[0], composition(z, w, queries)
        run = min(64, max(1, -(-plan.n_comb // (4 * n_cu * 4))))
        for what, (med, lo, hi) in res.items():
            line = {'case': name, 'what': what, 'ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                    'rounds': args.rounds, 'queries': len(queries), 'combinations': plan.n_comb, 'table_rows': plan.n_rows,
                    'combinations_per_s': plan.n_comb / (med * 1e-3)}
            if what in ('entry', 'entry_no_prefix'):
                rows = rows_read(queries, run, what == 'entry')
                line.update({'run': run, 'bytes_read_per_combination': rows * R * 4 / plan.n_comb,
                             'share_of_l2_rate': rows * R * 4 / (med * 1e-3) / L2_RATE})
            if what == 'torch_composition':
                line.update({'max_abs_diff_from_entry': float((got - ref).abs().nan_to_num(0.0).max()),
                             'same_nan': bool((torch.isnan(got) == torch.isnan(ref)).all())})
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
