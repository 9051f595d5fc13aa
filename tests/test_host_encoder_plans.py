"""The encoder plans that were built only in Python (tip_amd/layers.py `hier_graph` pd_csr with `drug_workgroups` /
`deal_rows_by_edges`, `gcn_norm_graph` with and without row pruning) against their C++ ports behind include/tipk.h section 10d,
element for element on the host; and the argument checks of `tipk_encoder_build` that answer before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch

from tip_amd import _lib
from tip_amd.layers import deal_rows_by_edges, gcn_norm_graph, hier_graph

TIPK_EINVAL, TIPK_EUNSUPPORTED = -1, -2


def _host_plan(fn, *args):
    h = C.c_void_p()
    st = fn(*args, C.byref(h))
    assert st == 0, st
    return h


def _array(h, name, dtype):
    data, count, eb = C.c_void_p(), C.c_int64(), C.c_int()
    assert _lib.lib().tipk_host_plan_array(h, name.encode(), C.byref(data), C.byref(count), C.byref(eb)) == 0, name
    assert eb.value == np.dtype(dtype).itemsize, (name, eb.value)
    if count.value == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(data, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (count.value,)).copy()


def _i64(t):
    return np.ascontiguousarray(t.numpy().astype(np.int64))


def _pd_graph(seed, n_prot=900, n_drug=300):
    """P -> D edges in the concatenated node space: one hub drug with > 512 targets, drugs without targets, proteins that no
    drug targets (every edge starts at a protein, so the compact source block is the set of targeted proteins)."""
    g = torch.Generator().manual_seed(seed)
    hub = torch.stack([torch.randperm(n_prot, generator=g)[:700], torch.full((700,), 3)])
    mid = torch.stack([torch.randint(0, n_prot // 2, (400,), generator=g), torch.randint(10, 14, (400,), generator=g)])
    rest = torch.stack([torch.randint(0, n_prot // 2, (1500,), generator=g), torch.randint(20, n_drug - 40, (1500,), generator=g)])
    ei = torch.cat([hub, mid, rest], 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    ei[1] += n_prot
    return ei, n_prot, n_drug


@pytest.mark.parametrize('seed', [0, 1])
def test_pd_csr_matches_hier_graph(seed):
    ei, n_prot, n_drug = _pd_graph(seed)
    rows = torch.unique(ei[0])
    assert rows.numel() < n_prot                                             # proteins outside every target list
    inv = torch.full((n_prot,), -1, dtype=torch.int64)
    inv[rows] = torch.arange(rows.numel())
    n_c = int(rows.numel())
    cei = torch.stack([inv[ei[0]], ei[1] - n_prot + n_c])                    # MyHierarchyConv.mean_sources(rows=...)
    ref = hier_graph(cei, n_c + n_drug, n_c, table_rows=n_c, d=16).pd_csr
    mr, me = C.c_int(), C.c_int()
    _lib.lib().tipk_pd_stage_bwd_limits(C.byref(mr), C.byref(me))
    src, dst = _i64(cei[0]), _i64(cei[1])
    h = _host_plan(_lib.lib().tipk_plan_hier_csr, src.ctypes.data, dst.ctypes.data, src.size, n_c + n_drug, n_c, n_c, mr.value, me.value)
    try:
        for k in ('fwd_ptr', 'fwd_src', 'fwd_order', 't_ptr', 't_dst'):
            np.testing.assert_array_equal(_array(h, k, np.int32), ref[k].numpy(), err_msg=k)
        np.testing.assert_array_equal(_array(h, 'fwd_wg', np.int32), ref['fwd_wg'].numpy().reshape(-1))
        for k in ('scale', 't_w'):
            assert np.array_equal(_array(h, k, np.float32).view(np.uint32), ref[k].numpy().view(np.uint32)), k
        counts = torch.bincount(cei[0], minlength=n_c).tolist()
        np.testing.assert_array_equal(_array(h, 't_wg', np.int32), np.array(deal_rows_by_edges(counts, mr.value, me.value)))
        assert _lib.lib().tipk_host_plan_scalar(h, b'n_src') == n_c
        wg = ref['fwd_wg'].numpy()
        assert (wg[:, 1] >> 8 == 16).sum() == 1                                # the hub has a workgroup to itself
        assert int(ref['fwd_ptr'][-1]) == ei.shape[1] and (np.diff(ref['fwd_ptr'].numpy()) == 0).any()    # drugs without targets
    finally:
        _lib.lib().tipk_host_plan_free(h)


def _gather_equal(h, pre, plan, w_edges):
    """plan arrays equal to the Python builder's; edge weights = w_edges (caller's edge order) in plan order."""
    np.testing.assert_array_equal(_array(h, pre + 'row_id', np.int32), plan.row_id.numpy())
    np.testing.assert_array_equal(_array(h, pre + 'items', np.int32), plan.items.numpy().reshape(-1))
    np.testing.assert_array_equal(_array(h, pre + 'perm', np.int64), plan.perm.numpy())
    assert np.array_equal(_array(h, pre + 'edge_w', np.float32).view(np.uint32), w_edges[plan.perm.numpy()].view(np.uint32))
    assert _lib.lib().tipk_host_plan_scalar(h, (pre + 'group_slots').encode()) == plan.group_slots


def _device_norm_weights(ei, n, rows):
    """A_hat's edge weights as FMEncoder forms them on the device: deg^-1/2 correctly rounded (torch's device pow(-0.5) -- its
    CPU pow rounds twice), the product in fp32; the edge list of `gcn_norm_graph` (self loops replaced, rows kept)."""
    row, col = ei[0].numpy(), ei[1].numpy()
    keep = row != col
    row = np.concatenate([row[keep], np.arange(n)])
    col = np.concatenate([col[keep], np.arange(n)])
    deg = np.bincount(col, minlength=n).astype(np.float64)
    dis = (1.0 / np.sqrt(deg)).astype(np.float32)
    w = dis[row] * dis[col]
    if rows is not None:
        inv = np.full(n, -1)
        inv[rows.numpy()] = np.arange(rows.numel())
        w = w[inv[col] >= 0]
    return w


@pytest.mark.parametrize('pruned', [False, True])
def test_gcn_norm_plans_match(pruned):
    g = torch.Generator().manual_seed(7)
    n = 1200
    ei = torch.randint(0, n, (2, 9000), generator=g)
    ei[:, :40] = torch.arange(40).repeat(2, 1)                              # existing self loops are replaced
    ei[0, 100:900] = 5                                                     # a hub row (split into pieces)
    rows = torch.unique(torch.randint(0, n, (300,), generator=g)) if pruned else None
    ref = gcn_norm_graph(ei, n, d=32, rows=rows)
    src, dst = _i64(ei[0]), _i64(ei[1])
    r = _i64(rows) if pruned else None
    h = _host_plan(_lib.lib().tipk_plan_gcn_norm, src.ctypes.data, dst.ctypes.data, src.size, n,
                   r.ctypes.data if pruned else None, r.size if pruned else 0, 32)
    try:
        w = _device_norm_weights(ei, n, rows)
        _gather_equal(h, 'fwd.', ref.fwd, w)
        _gather_equal(h, 'bwd.', ref.bwd, w)
        # ... and these are the weights of the device build, which differ from torch's CPU pow(-0.5) in the last bit here and there
        assert ref.fwd.edge_w.numel() == w.size
    finally:
        _lib.lib().tipk_host_plan_free(h)


def _build(pp, dp, dd, rng, n_prot, n_drug, dims, n_rel=None):
    enc = C.c_void_p()
    keep = [np.ascontiguousarray(a, dtype=np.int64) for a in (pp, dp, dd, rng)]
    st = _lib.lib().tipk_encoder_build(keep[0].ctypes.data, keep[0].shape[1], keep[1].ctypes.data, keep[1].shape[1], keep[2].ctypes.data,
                                       keep[2].shape[1], keep[3].ctypes.data, keep[3].shape[0] if n_rel is None else n_rel, 8, n_prot,
                                       n_drug, C.byref(dims) if dims is not None else None, C.byref(enc))
    if st == 0:
        _lib.lib().tipk_encoder_destroy(enc)
    assert not enc.value or st == 0
    return st


def _toy(n_prot=50, n_drug=20):
    pp = np.array([[0, 1, 2, 3], [1, 2, 3, 4]])
    dp = np.array([[0, 1, 2], [n_prot, n_prot + 1, n_prot + 5]])
    dd = np.array([[0, 1, 2, 3], [1, 0, 3, 2]])
    rng = np.array([[0, 2], [2, 4]])
    return pp, dp, dd, rng


def test_encoder_build_rejects_bad_arguments():
    dims = _lib.EncoderDims(48, 16, 32, 16, 32, 1)
    pp, dp, dd, rng = _toy()
    L = _lib.lib()
    assert L.tipk_encoder_build(None, 0, None, 0, None, 0, None, 0, 8, 50, 20, C.byref(dims), None) == TIPK_EINVAL
    assert _build(pp, dp, dd, rng, 50, 20, None) == TIPK_EINVAL                         # no dims
    assert _build(pp, dp, dd, rng, -1, 20, dims) == TIPK_EINVAL                         # negative node count
    assert _build(pp, dp, dd, rng, 50, 20, dims, n_rel=-1) == TIPK_EINVAL
    bad = _lib.EncoderDims(48, 16, 32, 16, 32, 0)                                         # add needs n_embed == prot_drug_dim
    assert _build(pp, dp, dd, rng, 50, 20, bad) == TIPK_EINVAL
    bad = _lib.EncoderDims(48, 16, 32, 16, 32, 2)
    assert _build(pp, dp, dd, rng, 50, 20, bad) == TIPK_EINVAL
    neg = _lib.EncoderDims(48, 16, 32, -16, 32, 1)
    assert _build(pp, dp, dd, rng, 50, 20, neg) == TIPK_EINVAL
    null_idx = L.tipk_encoder_build(None, 4, None, 0, None, 0, None, 0, 8, 50, 20, C.byref(dims), C.byref(C.c_void_p()))
    assert null_idx == TIPK_EINVAL                                                      # edges without an index array
    assert L.tipk_encoder_build(None, 0, None, 0, None, 0, None, 0, 3, 50, 20, C.byref(dims), C.byref(C.c_void_p())) == TIPK_EINVAL


def test_encoder_build_refuses_unsupported_shapes():
    pp, dp, dd, rng = _toy(n_drug=1025)
    assert _build(pp, dp, dd, rng, 50, 1025, _lib.EncoderDims(48, 16, 32, 16, 32, 1)) == TIPK_EUNSUPPORTED     # > 1 024 drugs
    pp, dp, dd, rng = _toy()
    assert _build(pp, dp, dd, rng, 50, 20, _lib.EncoderDims(48, 16, 48, 16, 32, 1)) == TIPK_EUNSUPPORTED       # n_hid1 = 48
