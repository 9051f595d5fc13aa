"""-m gpu: the relation-SHARDED step on the LARGE-GRAPH route (more than 1024 drugs: segment-major forward plan,
CSR transposed pass, gather_sum finalize, Y / dY in HBM) -- the route BASELINE config 5 takes on every rank and the
one configuration VERDICT r2 listed as untested.  Ranks are processes sharing the one GPU of the test box over gloo
(8 x MI355X over RCCL is the driver's to run).

  * a 1 500-drug / 12-relation encoder (all three stages), 2 and 4 ranks: every rank's z and gradients against the
    CPU oracle of the UNSHARDED model (shard-local att rows against the matching rows);
  * config 5 at FULL size (10 000 drugs, 2 000 relations, 50 M edges, dim 128), 4 ranks: one R-GCN layer, sharded
    == unsharded for out / dX / d basis / d root / the local d att rows; the unsharded pass runs first in the parent
    process and hands its results and every rank's edge block over as files;
  * `bench.py --gpus 2 --oversubscribe` as a subprocess: the N-rank bench path end to end, JSON line parsed.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tip_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(target, world, args, timeout):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, ret) + tuple(args)) for r in range(world)]
    from conftest import start_ranks
    start_ranks(procs)
    for p in procs:
        p.join(timeout)
        assert p.exitcode == 0, 'rank process failed (exit code %r)' % p.exitcode
    assert dict(ret) == {r: True for r in range(world)}, dict(ret)


SMALL = dict(n_drug=1500, n_rel=12, n_edges=60000, seed=5, with_protein_graph=True, n_prot=700, pp_edges=4000, dp_edges=900)
SMALL_DIMS = dict(prot_drug_dim=16, n_embed=48, n_hid1=64, n_hid2=32, num_base=32)


def _encoder_worker(rank, world, port, ret):
    """One rank of the sharded ENCODER on a graph beyond the LDS-resident kernels, against the oracle of the
    unsharded model."""
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from tip_amd import ops
        from tip_amd.data import synthetic_data_dict, Data
        from tip_amd.dist import make_shard, shard_data_dict, attach_shard
        from tip_amd.layers import FMEncoder
        dd = synthetic_data_dict(**SMALL)
        N, R = dd['n_drug'], dd['n_dd_et']
        assert N > 1024 and ops.rel_gather_split(N, 64, False) == 0        # the large-graph route (layers.rgcn_graph: N > 1024)
        p = O.init_params(N, dd['n_prot'], R, mod='cat', seed=3, **SMALL_DIMS)
        shard = make_shard(dd['dd_train_range'], rank, world)
        ids = shard.rel_ids
        assert 0 < ids.numel() < R
        loc = shard_data_dict(dd, shard)
        enc = FMEncoder(DEV, N, len(ids), dd['n_prot'], dd['n_prot'], N, mod='cat', **SMALL_DIMS)
        sd = enc.state_dict()
        for k in sd:
            sd[k] = (p[k][ids] if k.endswith('.att') else p[k]).clone()
        enc.load_state_dict(sd)
        enc = enc.to(DEV)
        attach_shard(enc, shard)
        d = Data.from_dict(loc).to(DEV)
        z = enc(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, d.p_feat, d.pp_train_indices,
                d.dp_edge_index, d.dp_range_list)
        torch.manual_seed(2)
        up = torch.randn(N, SMALL_DIMS['n_hid2'])
        (z * up.to(DEV)).sum().backward()
        zo, saved = O.fm_encoder_fwd(p, dd, 'cat')
        go = O.fm_encoder_bwd(up, p, dd, saved, 'cat')
        ok = torch.allclose(z.detach().cpu().double(), zo.double(), rtol=1e-5, atol=1e-5 * float(zo.abs().max()))
        for k, prm in enc.named_parameters():
            want = go[k][ids] if k.endswith('.att') else go[k]
            good = torch.allclose(prm.grad.cpu().double(), want.double(), rtol=1e-4,
                                  atol=2e-5 * max(1e-3, float(go[k].abs().max())))
            if not good:
                print('rank', rank, 'gradient mismatch', k, float((prm.grad.cpu() - want).abs().max()), flush=True)
            ok = ok and good
        # the plans this rank used: generic / segmented forward, CSR transposed pass
        g1 = enc.rgcn1._cache.value
        ok = ok and g1.pair_fwd is None and g1.rs_bwd is None and g1._csr_bwd is not None and not callable(g1._csr_bwd)
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('world', [2, 4])
def test_sharded_encoder_large_graph_route_vs_oracle(world):
    _spawn(_encoder_worker, world, (), 500)


# ------------------------------------------------------------------------------------------------ config 5, full size
def _layer_params(d_in, d_out, n_rel, nb, seed):
    g = torch.Generator().manual_seed(seed)
    return {'basis': torch.randn(nb, d_in, d_out, generator=g) / d_in ** 0.5,
            'att': torch.randn(n_rel, nb, generator=g) / nb ** 0.5,
            'root': torch.randn(d_in, d_out, generator=g) / d_in ** 0.5}


def _config5_worker(rank, world, port, ret, tmp):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from tip_amd.dist import RelationShard
        from tip_amd.layers import MyRGCNConv2
        ref = torch.load(os.path.join(tmp, 'ref.pt'))
        mine = torch.load(os.path.join(tmp, 'rank%d.pt' % rank))
        N, R = ref['n_drug'], ref['n_rel']
        ids = mine['rel_ids']
        shard = RelationShard(ids, rank, world, n_relations=R)
        shard.in_degree = ref['in_degree']
        prm = _layer_params(128, 128, R, 32, 7)
        layer = MyRGCNConv2(128, 128, len(ids), 32, after_relu=False)
        layer.basis.data.copy_(prm['basis'])
        layer.root.data.copy_(prm['root'])
        layer.att.data.copy_(prm['att'][ids])
        layer = layer.to(DEV)
        layer.shard = shard
        x = ref['x'].to(DEV).requires_grad_(True)
        out = layer(x, mine['edge_index'].to(DEV), None, mine['range'].to(DEV))
        (out * ref['up'].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        graph = layer._cache.value
        ok = graph.pair_fwd is None and graph.rs_bwd is None                    # large-graph route on this rank
        ok = ok and graph.fwd.n_slots > 0                                      # segment-major plan: rows in pieces
        checks = (('out', out.detach(), ref['out'], 1e-4), ('dX', x.grad, ref['dx'], 2e-4),
                  ('d basis', layer.basis.grad, ref['dbasis'], 2e-4), ('d root', layer.root.grad, ref['droot'], 2e-4),
                  ('d att rows', layer.att.grad, ref['datt'][ids], 2e-4))
        for name, got, want, rtol in checks:
            good = torch.allclose(got.cpu(), want, rtol=rtol, atol=2e-5 * max(1e-6, float(want.abs().max())))
            if not good:
                print('rank', rank, name, 'differs by', float((got.cpu() - want).abs().max()), 'of', float(want.abs().max()), flush=True)
            ok = ok and good
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(2400)
def test_config5_full_size_sharded_over_four_ranks(tmp_path):
    """BASELINE config 5 at full size, relation-sharded over 4 ranks (sharing one GPU, gloo): each rank runs the
    large-graph route on ITS 12.5 M edges -- segment-major forward plan over its 2.5 GB of Y, finalize, the CSR
    transposed pass, dY products, flat-buffer all-reduces of the partial aggregate and of [dX | d basis] -- and
    reproduces the unsharded layer: out, dX, d basis, d root, and its own rows of d att."""
    from tip_amd.data import synthetic_data_dict
    from tip_amd.dist import partition_relations, shard_edges, _local_ranges
    from tip_amd.layers import MyRGCNConv2
    world = 4
    dd = synthetic_data_dict()                                            # config 5 defaults, seed 1111
    N, R = dd['n_drug'], dd['n_dd_et']
    assert N == 10000 and R == 2000 and dd['dd_train_idx'].shape[1] == 50_000_000
    prm = _layer_params(128, 128, R, 32, 7)
    layer = MyRGCNConv2(128, 128, R, 32, after_relu=False)
    for k, v in prm.items():
        getattr(layer, k).data.copy_(v)
    layer = layer.to(DEV)
    g = torch.Generator().manual_seed(11)
    x_c = torch.randn(N, 128, generator=g)
    up_c = torch.randn(N, 128, generator=g)
    x = x_c.to(DEV).requires_grad_(True)
    out = layer(x, dd['dd_train_idx'].to(DEV), None, dd['dd_train_range'].to(DEV))
    (out * up_c.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    tmp = str(tmp_path)
    torch.save({'n_drug': N, 'n_rel': R, 'x': x_c, 'up': up_c, 'out': out.detach().cpu(), 'dx': x.grad.cpu(),
                'dbasis': layer.basis.grad.cpu(), 'droot': layer.root.grad.cpu(), 'datt': layer.att.grad.cpu(),
                'in_degree': torch.bincount(dd['dd_train_idx'][1], minlength=N)}, os.path.join(tmp, 'ref.pt'))
    rg = dd['dd_train_range']
    parts = partition_relations((rg[:, 1] - rg[:, 0]).tolist(), world)
    for r in range(world):
        ei, _ = shard_edges(dd['dd_train_idx'], rg, parts[r])
        torch.save({'rel_ids': torch.tensor(parts[r]), 'edge_index': ei.contiguous(), 'range': _local_ranges(rg, parts[r])},
                   os.path.join(tmp, 'rank%d.pt' % r))
    del layer, x, out, dd
    torch.cuda.empty_cache()
    _spawn(_config5_worker, world, (tmp,), 1500)


# ------------------------------------------------------------------------------------------------ bench.py --gpus 2
@pytest.mark.timeout(900)
def test_bench_two_ranks_oversubscribed_subprocess():
    """`python bench.py --gpus 2 --oversubscribe --workload synthetic-small`: the self-launch path (children before
    any GPU call in the parent), relation sharding on the large-graph route, one JSON line with the contract's
    fields."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env['TIPK_COLLECTIVE'] = 'group'                                      # the process group only (no peer-mailbox exchange)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--oversubscribe', '--workload',
                          'synthetic-small', '--steps', '3', '--warmup', '1', '--no-cpu-baseline'],
                         env=env, capture_output=True, text=True, timeout=850)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['steps'] == 3 and rec['warmup'] == 1 and rec['unit'] == 'edges/s'
    assert rec['value'] > 0 and rec['ms_per_step'] > 0 and rec['higher_is_better'] is True
    assert 'relation-sharded x2' in rec['config']['parallelism'] and rec['config']['collective'] == 'gloo'
    assert np.isfinite(rec['value'])


@pytest.mark.timeout(900)
def test_bench_two_ranks_direct_exchange_and_timed_routes():
    """BioSNAP over 2 ranks sharing the GPU with TIPK_COLLECTIVE=direct: the step's five all-reduces go through the
    one-shot exchange (tip_amd/csrc/tipk_peer.hip), each layer's forward route (pair form | Y) is timed per rank."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env['TIPK_COLLECTIVE'] = 'direct'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--oversubscribe', '--steps', '3',
                          '--warmup', '1', '--no-cpu-baseline', '--no-kernel-table'], env=env, capture_output=True, text=True, timeout=850)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert rec['n_gpus'] == 2 and rec['config']['collective'] == 'direct' and rec['value'] > 0
    routes = rec['config']['forward_routes']
    assert len(routes) == 2 and all(r and r[0][0] in ('pair', 'y') and set(r[0][1]) == {'pair', 'y'} for r in routes)


@pytest.mark.timeout(1500)
def test_bench_four_ranks_oversubscribed_auto_collective():
    """`bench.py --gpus 4 --oversubscribe --full` on BioSNAP (the ranks share the one GPU, gloo; at most 6 processes may hold it:
    this one, bench.py's launcher and 4 ranks): the exchange is set up behind its self-test, both collectives are timed per
    message size and the faster kept, and the line carries what the first real 8-GPU run will be read by: per-rank step
    times, the collective's timings, the replicated stage and the Amdahl ceiling it implies."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.pop('TIPK_COLLECTIVE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--oversubscribe', '--steps', '3',
                          '--warmup', '1', '--full', '--no-cpu-baseline', '--no-kernel-table'], env=env, capture_output=True, text=True,
                         timeout=1400)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert rec['n_gpus'] == 4 and rec['value'] > 0 and 'relation-sharded x4' in rec['config']['parallelism']
    assert len(rec['per_rank_ms_per_step']) == 4 and all(v > 0 for v in rec['per_rank_ms_per_step'])
    assert abs(max(rec['per_rank_ms_per_step']) - rec['ms_per_step']) < 1e-3
    ct = rec['config']['collective_timing']
    assert ct and (('per_size' in ct and len(ct['per_size']) >= 3 and
                    all(v['chosen'] in ('direct', 'group') for v in ct['per_size'].values())) or 'why' in ct)
    rp = rec['replicated']
    assert rp['replicated_us'] > 10 and rp['amdahl_ceiling'] > 1.0
    assert rec['config']['rccl_ranks'] == 0                                # gloo here; 8 on a real node


@pytest.mark.timeout(900)
def test_bench_one_rank_rccl_in_the_captured_step():
    """RCCL under the driver: `TIPK_FORCE_SHARD=1 python bench.py --gpus 1 --full` runs the relation-SHARDED
    step on one rank -- `init_process_group('nccl', device_id=...)`, every all-reduce of the step issued through RCCL and
    captured into the step's hipGraph (no silent eager fallback), fd 1 kept clean of RCCL's banner -- and the replayed
    graph's outputs equal the oracle's (`parity_in_bench`)."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env['TIPK_FORCE_SHARD'] = '1'
    env.pop('TIPK_COLLECTIVE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2',
                          '--full', '--no-extras', '--no-pmc', '--cpu-seconds', '2'], env=env, capture_output=True, text=True, timeout=850)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), out.stdout[-2000:]         # ONE JSON line, no banner on stdout
    rec = json.loads(lines[0])
    assert rec['config']['rccl_ranks'] == 1 and rec['config']['collective'] == 'nccl'
    assert rec['config']['launch'].startswith('hipGraph'), rec['config']['launch']
    assert rec['parity_in_bench']['ok'] and rec['parity_in_bench']['what'].endswith('hipGraph')
    assert rec['n_gpus'] == 1 and rec['value'] > 0 and 'replicated' in rec
