"""Time the partner sum (`tipk_distmult_partner_sum` / `tipk_pair_table_partner_sum`, include/tipk.h section 4l: what
`TIP.drug_profile` runs) on the device, next to the torch composition it replaces, in the same run.

  python tools/bench_drug_profile.py            1, 64 and all 645 queried drugs over the bundled BioSNAP graph's model (645 drugs,
                                                1 097 relations, dim 16), k = 10: with and without the training pairs excluded,
                                                the LDS-image route and the forced global route, the NN decoder's tables, and
                                                the composition: chunked `decoder(z, idx, et)` scores, the mask of the recorded
                                                pairs and a sum
  python tools/bench_drug_profile.py --random   random z / rel_w of that shape and random lists of BioSNAP density (no data set)

Prints one JSON line per measurement: ms per call (device events around `--reps` calls after `--warmup`; a case is repeated
until the timed window holds at least `--min-ms` of work), logits/s, the ratio to the lane-op floor -- every logit costs dim
fused multiply-adds and SIGMA_OPS further vector instructions per lane, over the chip's 78.6 T lane-ops/s (256 CUs x 4 SIMDs x
32 lanes x 2.4 GHz; the table variant: one add per logit) -- and, for the composition, its time over the kernel's and the
largest relative difference of its sums from the kernel's.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tip_amd import _lib, ops                            # noqa: E402

LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
SIGMA_OPS = 26          # vector instructions of sigma, the weight product and the add per logit in partner_sum_kernel (profiles/drug_profile.md)
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


def report(name, ms, reps, n_q, n, n_rel, ops_per_logit, extra=None):
    logits = n_q * n_rel * (n - 1)
    floor_ms = logits * float(ops_per_logit) / LANE_OPS_PER_S * 1e3
    line = {'case': name, 'ms': round(ms, 4), 'reps': reps, 'queried_drugs': n_q, 'logits': logits,
            'logits_per_s': logits / (ms * 1e-3), 'lane_op_floor_ms': round(floor_ms, 5), 'ratio_to_floor': round(ms / floor_ms, 2)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return line


def torch_composition(decoder, z, q, known, n, n_rel, chunk=16):
    """The same quantity from what existed before: the decoder's scores of every (queried drug, partner, relation) triple
    in chunks of queried drugs, the mask of the recorded pairs (forward keys of symmetric lists) and of the drug itself, and
    a sum over the partners -> (sum [Q, R], count [Q, R])."""
    c = torch.arange(n, device=z.device)
    et = torch.arange(n_rel, device=z.device).repeat(n)
    comb = None
    if known is not None:
        keys, kptr = known
        rel = torch.repeat_interleave(torch.arange(n_rel, device=z.device), kptr[1:] - kptr[:-1])
        comb = rel * (n * n) + keys
    sums, counts = [], []
    for q0 in range(0, q.numel(), chunk):
        u = q[q0:q0 + chunk].long()
        g = u.numel()
        idx = torch.stack([u.repeat_interleave(n * n_rel), c.repeat_interleave(n_rel).repeat(g)])
        score = decoder(z, idx, et.repeat(g)).view(g, n, n_rel)
        free = (c[None, :] != u[:, None])[:, :, None].expand(-1, -1, n_rel)
        if comb is not None:
            probe = et.view(1, n, n_rel) * (n * n) + (u[:, None] * n + c[None, :])[:, :, None]
            at = torch.searchsorted(comb, probe.reshape(-1)).clamp(max=comb.numel() - 1)
            free = free & (comb[at] != probe.reshape(-1)).view(g, n, n_rel)
        sums.append((score * free).sum(1))
        counts.append(free.sum(1))
    return torch.cat(sums), torch.cat(counts)


def random_lists(n, n_rel, g, per_rel=4200):
    uv = torch.randint(0, n, (n_rel, per_rel // 2, 2), generator=g)
    rel = torch.arange(n_rel)[:, None].expand(-1, per_rel // 2)
    ok = uv[..., 0] != uv[..., 1]
    comb = torch.unique(torch.cat([(rel * n * n + uv[..., 0] * n + uv[..., 1])[ok], (rel * n * n + uv[..., 1] * n + uv[..., 0])[ok]]))
    kptr = torch.zeros(n_rel + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(torch.bincount(torch.div(comb, n * n, rounding_mode='floor'), minlength=n_rel), 0)
    return (comb % (n * n)).to(DEV), kptr.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--random', action='store_true')
    args = ap.parse_args()
    _lib.ensure_built()
    assert torch.cuda.is_available(), 'bench_drug_profile times the device: no GPU visible'
    from tip_amd.layers import MultiInnerProductDecoder
    g = torch.Generator().manual_seed(1)
    if args.random:
        n, R, dim = 645, 1097, 16
        z, w = (torch.randn(n, dim, generator=g) / 2).to(DEV), (torch.randn(R, dim, generator=g) / 2).to(DEV)
        known = random_lists(n, R, g)
    else:
        from tip_amd.layers import TIP, Setting, _screen_known
        torch.manual_seed(0)
        model = TIP(Setting(), torch.device(DEV), data_path=None)
        d = model.data
        n, R = d.n_drug, d.n_dd_et
        z, w = model.embeddings.detach(), model.decoder.weight.detach()
        dim = z.shape[1]
        known = ops.symmetric_known(_screen_known(d, 'train'), n)
    decoder = MultiInnerProductDecoder(dim, R).to(DEV)
    decoder.weight.data = w.clone()
    s1t, s2t = torch.randn(R, n, generator=g).to(DEV), torch.randn(R, n, generator=g).to(DEV)

    for n_q in (1, 64, n):
        q = torch.randperm(n, generator=g)[:n_q].to(DEV)
        kernel_ms = {}
        for route in ('lds', 'global'):
            _lib.set_option('partner_sum_global', int(route == 'global'))
            try:
                assert _lib.lib().tipk_distmult_partner_sum_lds_route(n, dim) == int(route == 'lds')
                for kn, what in ((None, 'unfiltered'), (known, 'exclude_train')):
                    fn = lambda: ops.distmult_partner_sum(z, w, q, args.k, None, None, kn)
                    ms, reps = timed(fn, args.reps, args.warmup, args.min_ms)
                    report('profile_%d_%s_%s' % (n_q, route, what), ms, reps, n_q, n, R, dim + SIGMA_OPS, {'k': args.k})
                    if route == 'lds':
                        kernel_ms[what] = (ms, fn())
            finally:
                _lib.set_option('partner_sum_global', 0)
        for kn, what in ((None, 'unfiltered'), (known, 'exclude_train')):
            fn = lambda: ops.pair_table_partner_sum(s1t, s2t, q, args.k, None, None, kn)
            ms, reps = timed(fn, args.reps, args.warmup, args.min_ms)
            report('profile_%d_table_%s' % (n_q, what), ms, reps, n_q, n, R, 1 + SIGMA_OPS, {'k': args.k})
        with torch.no_grad():
            for kn, what in ((None, 'unfiltered'), (known, 'exclude_train')):
                fn = lambda: torch_composition(decoder, z, q, kn, n, R)
                ms, reps = timed(fn, 1, 1, args.min_ms)
                got, cnt = fn()
                k_ms, ref = kernel_ms[what]
                rel_diff = float(((got - ref[0]).abs() / ref[0].abs().clamp(min=1e-30)).max())
                report('profile_%d_torch_composition_%s' % (n_q, what), ms, reps, n_q, n, R, dim + SIGMA_OPS,
                       {'times_the_kernel': round(ms / k_ms, 1), 'max_rel_diff_from_kernel': rel_diff,
                        'same_counts': bool(torch.equal(cnt, ref[1].long()))})


if __name__ == '__main__':
    main()
