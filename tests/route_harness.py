"""TEST INFRASTRUCTURE: what the layer-level R-GCN route tests share (tests/test_gpu_large_routes.py,
tests/test_gpu_rgcn_routes.py): graphs with deliberate edge cases, the launch labels of a pass, route assertions and the
comparison with the fp64 oracle.  Plain functions, no fixtures; nothing here touches the GPU unless asked to run something."""
import torch

# the LARGE-graph routes (tests/test_gpu_large_routes.py): route -> a label its pass launches
ROUTE_LABELS = {'rows_s': 'row_products_s[', 'rows': 'row_products[', 'dest': 'dest_products[', 'csr': 'gather_rows_csr[',
                'Y': 'gather_sum[dd.fwd', 'gather_sum': 'gather_sum[dd.bwd'}


def _graph(N, R, seed, n_random=120000):
    """LARGE graphs: edge_index [2, E], edge_type [E], range_list [R, 2] (relation-major, as the reference's data has them)."""
    g = torch.Generator().manual_seed(seed)
    used = list(range(1, 32)) + list(range(64, R - 1)) if R >= 66 else list(range(1, R - 1))
    used = torch.tensor(used)
    quiet = 64                                                          # nodes 0 .. 63: no in-edges; N - 64 .. N - 1: no out-edges
    src = torch.randint(0, N - quiet, (n_random,), generator=g)
    dst = torch.randint(quiet, N, (n_random,), generator=g)
    hub_src = torch.randint(0, N - quiet, (10000,), generator=g)      # the hub is node N - 1 (edges that touch node N - 1)
    loops = torch.arange(quiet, N - quiet, max(1, (N - 2 * quiet) // 200))
    src = torch.cat([src, hub_src, loops, src[:500]])
    dst = torch.cat([dst, torch.full((10000,), N - 1), loops, dst[:500]])
    rel = used[torch.randint(0, used.numel(), (src.numel(),), generator=g)]
    rel[-500:] = rel[:500]                                              # duplicates: same (source, destination, relation)
    order = torch.sort(rel, stable=True).indices
    src, dst, rel = src[order], dst[order], rel[order]
    cnt = torch.bincount(rel, minlength=R)
    assert int(cnt[0]) == 0 and int(cnt[R - 1]) == 0
    end = torch.cumsum(cnt, 0)
    rg = torch.stack([end - cnt, end], 1)
    return torch.stack([src, dst]), rel, rg


def _next_pow2(n):
    return 1 << (int(n) - 1).bit_length()


def small_graph(N, R, seed, kind='dir', pow2=False):
    """Small and mid-size graphs (N <= a few thousand) -> (edge_index [2, E], edge_type [E], range_list [R, 2]), relation-major.

    kind: 'dir' (directed), 'sym' (u -> v in relation r iff v -> u in r, duplicates and self-loops included), 'near' ('sym' plus
    ONE directed edge whose mirror is absent).  Every graph with N >= 8 and R >= 4 has: relations 0 and R - 1 without edges,
    relation 1 with exactly one edge (a self-loop in the symmetric kinds), nodes without in-edges and nodes without out-edges
    (isolated nodes in the symmetric kinds), a hub (node N - 1), duplicate (source, destination, relation) triples and
    self-loops.  pow2: every in-degree (over all relations) is 0 or a power of two -- 1 / deg is exact in fp32 -- padded with
    self-loops (symmetric kinds) or edges from random sources (directed)."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g)
    if N < 8:
        # the degenerate node count (N = 1): a self-loop per node, node 0's twice, in relation min(1, R - 1)
        assert kind != 'near'
        src = torch.cat([torch.arange(N), torch.zeros(1, dtype=torch.int64)])
        return _finish(src, src.clone(), torch.full((src.numel(),), min(1, R - 1)), N, R)
    # R < 4 (R = 1): every relation carries random edges, no empty / one-edge relation
    one = R >= 4
    used = torch.arange(2, R - 1) if one else torch.arange(R)
    quiet = max(1, N // 12)
    hub = N - 1
    n_rand = max(4 * N, 400)
    n_hub = max(64, 8 * n_rand // N)                                # in-edges of the hub: > 4 x the mean in-degree
    if kind == 'dir':
        # nodes 0 .. quiet - 1: no in-edges; N - quiet - 1 .. N - 2 and the hub: no out-edges
        lo, hi = 0, N - quiet - 1
        src = torch.cat([ri(lo, hi, n_rand), ri(lo, hi, n_hub)])
        dst = torch.cat([ri(quiet, N - 1, n_rand), torch.full((n_hub,), hub)])
        loops = torch.arange(quiet, hi, max(1, (hi - quiet) // 24))
        src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
        rel = used[ri(0, used.numel(), src.numel())]
        src, dst, rel = torch.cat([src, src[:24]]), torch.cat([dst, dst[:24]]), torch.cat([rel, rel[:24]])     # duplicates
        if one:                                                     # relation 1: one edge
            src, dst, rel = torch.cat([src, src[:1]]), torch.cat([dst, dst[:1]]), torch.cat([rel, torch.ones(1, dtype=rel.dtype)])
        if pow2:
            deg = torch.bincount(dst, minlength=N)
            pad = torch.tensor([_next_pow2(d) - d if d > 0 else 0 for d in deg.tolist()])
            pd = torch.repeat_interleave(torch.arange(N), pad)
            src, dst = torch.cat([src, ri(lo, hi, pd.numel())]), torch.cat([dst, pd])
            rel = torch.cat([rel, used[ri(0, used.numel(), pd.numel())]])
        return _finish(src, dst, rel, N, R)
    # symmetric kinds: nodes N - quiet - 1 .. N - 2 are isolated; undirected edges among the others, hub N - 1
    m = N - quiet - 1
    a = torch.cat([ri(0, m, n_rand // 2), ri(0, m, n_hub)])
    b = torch.cat([ri(0, m, n_rand // 2), torch.full((n_hub,), hub)])
    loops = torch.arange(0, m, max(1, m // 24))
    a, b = torch.cat([a, loops]), torch.cat([b, loops])
    rel = used[ri(0, used.numel(), a.numel())]
    a, b, rel = torch.cat([a, a[:24]]), torch.cat([b, b[:24]]), torch.cat([rel, rel[:24]])                 # duplicates
    if one:                                                         # relation 1: one edge, a self-loop
        a, b, rel = torch.cat([a, loops[:1]]), torch.cat([b, loops[:1]]), torch.cat([rel, torch.ones(1, dtype=rel.dtype)])
    off = a != b
    src, dst, rel = torch.cat([a, b[off]]), torch.cat([b, a[off]]), torch.cat([rel, rel[off]])
    if kind == 'near':
        have = set(zip(src.tolist(), dst.tolist(), rel.tolist()))
        for _ in range(1000):
            u, v, r = int(ri(0, m, 1)), int(ri(0, m, 1)), int(used[int(ri(0, used.numel(), 1))])
            if u != v and (u, v, r) not in have:
                break
        assert u != v and (u, v, r) not in have and (v, u, r) not in have
        src, dst, rel = torch.cat([src, torch.tensor([u])]), torch.cat([dst, torch.tensor([v])]), torch.cat([rel, torch.tensor([r])])
    if pow2:
        deg = torch.bincount(dst, minlength=N)
        pad = torch.tensor([_next_pow2(d) - d if d > 0 else 0 for d in deg.tolist()])
        pl = torch.repeat_interleave(torch.arange(N), pad)                                  # self-loops keep the symmetry
        src, dst, rel = torch.cat([src, pl]), torch.cat([dst, pl]), torch.cat([rel, used[ri(0, used.numel(), pl.numel())]])
    return _finish(src, dst, rel, N, R)


def _finish(src, dst, rel, N, R):
    order = torch.sort(rel, stable=True).indices
    src, dst, rel = src[order], dst[order], rel[order]
    cnt = torch.bincount(rel, minlength=R)
    end = torch.cumsum(cnt, 0)
    return torch.stack([src, dst]), rel, torch.stack([end - cnt, end], 1)


def check_small_graph(ei, rel, N, R, kind, pow2):
    """Asserts the edge cases `small_graph` promises (the test must not silently lose them)."""
    src, dst = ei[0], ei[1]
    cnt = torch.bincount(rel, minlength=R)
    deg_in, deg_out = torch.bincount(dst, minlength=N), torch.bincount(src, minlength=N)
    if pow2:
        assert all(d == 0 or d & (d - 1) == 0 for d in deg_in.tolist())
    keys = ((rel * N + src) * N + dst)
    assert keys.unique().numel() < keys.numel(), 'no duplicate triples'
    assert bool((src == dst).any()), 'no self-loops'
    if N < 8:
        return
    if R >= 4:
        assert int(cnt[0]) == 0 and int(cnt[R - 1]) == 0 and int(cnt[1]) == 1
    assert bool((deg_in == 0).any()) and bool((deg_out == 0).any())
    assert int(deg_in[N - 1]) >= 4 * float(deg_in.float().mean()), 'no hub'
    fw = torch.sort(keys).values
    bw = torch.sort((rel * N + dst) * N + src).values
    assert bool(torch.equal(fw, bw)) == (kind == 'sym')
    if kind == 'near':                                              # exactly one triple without its mirror
        from collections import Counter
        cf, cb = Counter(fw.tolist()), Counter(bw.tolist())
        assert sum((cf - cb).values()) == 1 and sum((cb - cf).values()) == 1


def _labels(fn):
    from tip_amd import ops
    ops.timing_start()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        rec = ops.timing_stop()
    return out, ' '.join(sorted(rec))


def _assert_route(labels, want, pass_name):
    assert ROUTE_LABELS[want] in labels, (pass_name, want, labels)
    for other, lab in ROUTE_LABELS.items():
        if other != want and lab.split('[')[0] in ('row_products_s', 'row_products', 'dest_products', 'gather_rows_csr'):
            assert lab not in labels, (pass_name, want, other, labels)


def _close(got, want, rel_tol):
    want = want.to(torch.float64)
    got = got.detach().to('cpu', torch.float64)
    fw, fg = torch.isfinite(want), torch.isfinite(got)
    assert torch.equal(fw, fg), 'non-finite pattern differs at %d of %d elements' % (int((fw != fg).sum()), fw.numel())
    w = want[fw]
    scale = float(w.abs().max()) if w.numel() else 1.0
    torch.testing.assert_close(got[fw], w, rtol=rel_tol, atol=rel_tol * scale + 1e-12)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)
