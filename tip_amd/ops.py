"""Python face of libtipk: thin launch wrappers + the `torch.autograd.Function`s of the TIP layers.

torch supplies device memory, the current HIP stream and autograd bookkeeping; every FLOP of the
path is executed by the HIP kernels in `tip_amd/csrc` through the C ABI (`include/tipk.h`).
Backward passes are explicit (no autograd tracing through E x d tensors): each Function saves
only N x d activations and the static graph plans.
"""
import collections
import os

import torch

from . import _lib, switches
from ._cache import DerivedCache, keyable
from ._lib import SlabSumDesc, GemmDesc, WgGemmDesc, check, lib, ptr, stream_ptr, require_device

def _f32c(t):
    """fp32, unit column stride (row stride free)."""
    if t.dtype != torch.float32:
        raise _lib.TipkError('tip_amd computes in fp32; got %s' % t.dtype)
    if t.dim() >= 1 and t.stride(-1) != 1 and t.shape[-1] != 1:
        t = t.contiguous()
    return t


# ---------------------------------------------------------------------------------------------
# optional per-kernel timing (bench.py): HIP events recorded on the launch stream around one launch
# ---------------------------------------------------------------------------------------------
_TIMING = None          # None (off) or dict: label -> list of (start_event, end_event)


def timing_start():
    global _TIMING
    _TIMING = {}


def timing_stop():
    """-> {label: (n_launches, mean_ms)}; call after a device synchronize."""
    global _TIMING
    rec, _TIMING = _TIMING or {}, None
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in rec.items()}


class _timed(object):
    def __init__(self, label):
        self.label = label

    def __enter__(self):
        if _TIMING is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *exc):
        if _TIMING is not None:
            self.ev[1].record()
            _TIMING.setdefault(self.label, []).append(self.ev)


# ---------------------------------------------------------------------------------------------
# launch wrappers (one C call each)
# ---------------------------------------------------------------------------------------------
def _row_id_ptr(plan):
    """The plan's edge ids; a graph WITHOUT edges has none and an empty tensor has no storage (NULL, which the C entries refuse
    next to a non-empty item list): every item of such a plan is empty and no id is ever read, so any device address serves."""
    return ptr(plan.row_id if plan.n_edges else plan.items)


def gather_sum_epilogue_supported(plan, d):
    """True if `gather_sum(..., gate=, colsum=True, riders=)` runs as ONE launch on this plan (grouped, 1024-thread workgroups)."""
    return bool(not plan.n_slots and plan.items.shape[0] > 0 and d % 4 == 0 and lib().tipk_gather_sum_riders_supported(d, plan.group_slots))


def gather_sum(plan, table, row_scale=None, bias=None, relu=False, out=None, riders=(), gate=None, colsum=False):
    """out[n_out, d] per `plan` over `table` [n_table, d] (include/tipk.h section 1).
    riders: up to 3 `slab_job`s that are ready now -- summed by further workgroups of the SAME launch when the plan's
    workgroups have 1024 threads (`tipk_gather_sum_riders`), by a grouped slab-sum launch of their own otherwise.
    gate [n_out, d]: out = gate > 0 ? out : 0;  colsum: also return the per-workgroup column sums of out as [W, 1, d] (both only
    where `gather_sum_epilogue_supported`)."""
    table = _f32c(table)
    require_device(table, plan.items)
    d = table.shape[1]
    assert table.shape[0] == plan.n_table, (table.shape, plan.n_table)
    if out is None:
        out = torch.empty((plan.n_out, d), dtype=torch.float32, device=table.device)
    riders = list(riders)
    st = stream_ptr(table.device)
    L = lib()
    one_launch = (riders or gate is not None or colsum) and len(riders) <= 3 and gather_sum_epilogue_supported(plan, d)
    assert one_launch or (gate is None and not colsum), 'gate / colsum need a grouped plan with 1024-thread workgroups'
    if one_launch:
        arr = (SlabSumDesc * max(1, len(riders)))(*[r.desc for r in riders])
        parts = None
        if colsum:
            parts = torch.empty((-(-plan.items.shape[0] // plan.group_slots), 1, d), dtype=torch.float32, device=table.device)
        if gate is not None:
            assert tuple(gate.shape) == tuple(out.shape) and gate.stride(1) == 1 and gate.dtype == torch.float32
        with _timed('gather_sum[%s,d=%d]+%d sums' % (plan.tag, d, len(riders))):
            check(L.tipk_gather_sum_riders(ptr(table), table.stride(0), table.shape[0], _row_id_ptr(plan), ptr(plan.edge_w),
                                           ptr(plan.items), plan.items.shape[0], ptr(out), out.stride(0), ptr(row_scale),
                                           ptr(bias), int(relu), d, plan.group_slots, ptr(gate),
                                           gate.stride(0) if gate is not None else 0, ptr(parts), arr, len(riders), st),
                  'tipk_gather_sum_riders')
        return (out, parts) if colsum else out
    partial = None
    if plan.n_slots:
        partial = torch.empty((plan.n_slots, d), dtype=torch.float32, device=table.device)
    with _timed('gather_sum[%s,d=%d]' % (plan.tag, d)):
        check(L.tipk_gather_sum(ptr(table), table.stride(0), table.shape[0], _row_id_ptr(plan), ptr(plan.edge_w), ptr(plan.items),
                                plan.items.shape[0], ptr(out), out.stride(0), ptr(partial), ptr(row_scale),
                                ptr(bias), int(relu), d, plan.group_slots, st), 'tipk_gather_sum')
    gather_sum_finish(plan, partial, out, row_scale, bias, relu)
    if riders:
        gemm_group([], riders)
    return out


def gather_sum_finish(plan, partial, out, row_scale=None, bias=None, relu=False):
    """Adds the pieces of the rows that a plan cut into several work items (slot order: deterministic)."""
    if plan.n_slots:
        d = out.shape[1]
        check(lib().tipk_gather_sum_finalize(ptr(partial), ptr(plan.split_rows), plan.split_rows.shape[0], ptr(out),
                                             out.stride(0), ptr(row_scale), ptr(bias), int(relu), d, plan.max_slots,
                                             stream_ptr(out.device)), 'tipk_gather_sum_finalize')


def gather_sum_lin_supported(d, d2, group_slots):
    return bool(lib().tipk_gather_sum_lin_supported(int(d), int(d2), int(group_slots)))


def gather_sum_occupancy(d, group_slots, weighted=False, map=0):
    """Workgroups of the grouped gather kernel resident on one CU for rows of width d (`tipk_gather_sum_occupancy`; launches
    nothing).  map: 0 plain / riders, -1 gate + column sums, d2 > 0 the fused linear map with d2 outputs."""
    import ctypes as C
    n = C.c_int(0)
    check(lib().tipk_gather_sum_occupancy(int(d), int(group_slots), int(bool(weighted)), int(map), C.byref(n)),
          'tipk_gather_sum_occupancy')
    return n.value


def sum_slabs_xb_occupancy(d_out):
    """Workgroups of the hand-over kernel (`sum_slabs_xb`) resident on one CU (`tipk_sum_slabs_xb_occupancy`; launches nothing)."""
    import ctypes as C
    n = C.c_int(0)
    check(lib().tipk_sum_slabs_xb_occupancy(int(d_out), C.byref(n)), 'tipk_sum_slabs_xb_occupancy')
    return n.value


def gather_sum_lin(plan, table, weight, bias=None, relu=False, row_scale=None):
    """(agg, out2): agg = the plan's row sums over `table` [n_table, d] (x row_scale), out2 = relu?(agg @ weight^T + bias) for
    weight [d2, d] (any strides), in ONE launch on a grouped plan (include/tipk.h `tipk_gather_sum_lin`)."""
    table = _f32c(table)
    require_device(table, plan.items, weight)
    d, d2 = table.shape[1], weight.shape[0]
    assert table.shape[0] == plan.n_table and weight.shape[1] == d and plan.group_slots > 0 and not plan.n_slots
    agg = torch.empty((plan.n_out, d), dtype=torch.float32, device=table.device)
    out2 = torch.empty((plan.n_out, d2), dtype=torch.float32, device=table.device)
    with _timed('gather_sum_lin[%s,d=%d->%d]' % (plan.tag, d, d2)):
        check(lib().tipk_gather_sum_lin(ptr(table), table.stride(0), table.shape[0], _row_id_ptr(plan), ptr(plan.edge_w),
                                        ptr(plan.items), plan.items.shape[0], ptr(agg), agg.stride(0), ptr(row_scale),
                                        ptr(weight), weight.stride(0), weight.stride(1), ptr(bias), int(relu), ptr(out2),
                                        out2.stride(0), d, d2, plan.group_slots, stream_ptr(table.device)), 'tipk_gather_sum_lin')
    return agg, out2


def gather_rows_csr(plan, table):
    """out[n_out, d] = per-row sums over a CsrPlan (include/tipk.h section 1c)."""
    table = _f32c(table)
    require_device(table, plan.row_ptr)
    d = table.shape[1]
    assert table.shape[0] == plan.n_table, (table.shape, plan.n_table)
    out = torch.empty((plan.n_out, d), dtype=torch.float32, device=table.device)
    with _timed('gather_rows_csr[%s,d=%d]' % (plan.tag, d)):
        check(lib().tipk_gather_rows_csr(ptr(table), table.stride(0), table.shape[0], ptr(plan.row_ptr), ptr(plan.row_id), plan.n_out,
                                         ptr(out), out.stride(0), d, stream_ptr(table.device)), 'tipk_gather_rows_csr')
    return out


def sum_slabs(slabs, out=None, alpha=1.0, accumulate=False, row_scale=None, addend=None, relu=False):
    """out = relu?(alpha * row_scale (.) sum_s slabs[s] + addend (+ out)): ordered, deterministic
    (include/tipk.h section 2).  slabs: [S, rows, cols]."""
    assert slabs.is_contiguous()
    n = slabs.shape[0]
    per = slabs[0].numel()
    if out is None:
        out = torch.empty(slabs.shape[1:], dtype=torch.float32, device=slabs.device)
    assert out.is_contiguous() and out.numel() == per
    if addend is not None:
        assert addend.is_contiguous() and addend.numel() == per
    with _timed('sum_slabs[%dx%d]' % (n, per)):
        check(lib().tipk_sum_slabs_ex(ptr(slabs), n, per, per, alpha, int(accumulate), ptr(row_scale), slabs.shape[-1],
                                      ptr(addend), int(relu), ptr(out), stream_ptr(slabs.device)), 'tipk_sum_slabs_ex')
    return out


def rel_gather_split(n_nodes, d, backward):
    """column blocks `tipk_rel_gather` would use for this shape; 0 = use the generic gather_sum."""
    if switches.on('TIPK_NO_RELLOCAL'):
        return 0
    return int(lib().tipk_rel_gather_supported(n_nodes, d, int(backward)))


def rel_gather_wgs(n_nodes, d, backward, n_cu):
    """workgroups per column block the relation-local plan of this shape should be built for:
    occupancy (1 or 2 workgroups per CU) * CUs / column blocks."""
    split = rel_gather_split(n_nodes, d, backward)
    if split == 0:
        return 0
    occ = int(lib().tipk_rel_gather_occupancy(n_nodes, d, int(backward)))
    return max(1, occ * n_cu // split)


def rel_gather_chunk(n_nodes, d, backward):
    return int(lib().tipk_rel_gather_chunk(n_nodes, d, int(backward)))


def rel_gather_usable(rp, n_nodes, d, backward):
    return rp is not None and rel_gather_split(n_nodes, d, backward) > 0


def rel_gather(rp, table, backward, row_scale=None, reduce=True):
    """LDS-resident D-D aggregation (include/tipk.h section 1b).  forward: table = Y [R*N, d] ->
    partial slabs [n_wg, N, d] (summed here unless reduce=False); backward: table = g [N, d]
    (optionally scaled per row while staged) -> dY [R*N, d]."""
    table = _f32c(table)
    require_device(table, rp.idx)
    d = table.shape[1]
    n, r = rp.n_nodes, rp.n_rel
    if backward:
        out = torch.empty((r * n, d), dtype=torch.float32, device=table.device)
    else:
        out = torch.empty((rp.n_wg, n, d), dtype=torch.float32, device=table.device)
    with _timed('rel_gather[%s,d=%d]' % ('dd.bwd' if backward else 'dd.fwd', d)):
        check(lib().tipk_rel_gather(int(backward), ptr(table), table.stride(0), n, d, rp.n_wg, ptr(rp.wg_rel_ptr),
                                    ptr(rp.unit_meta), ptr(rp.idx), rp.idx_unit, ptr(rp.runs), ptr(rp.node_at),
                                    ptr(row_scale) if backward else None, ptr(out), d, stream_ptr(table.device)),
              'tipk_rel_gather')
    if backward or not reduce:
        return out
    return sum_slabs(out)


def stream_gather_split(n_table, d, max_split=4):
    """column blocks `tipk_stream_gather` would use for a table [n_table, d]; 0 = it does not fit in LDS.
    max_split: 4 on the D-D passes, 16 for the P-P graph (2-column blocks of 8-byte rows)."""
    if switches.on('TIPK_NO_RELLOCAL'):                 # (test hook: the generic fabric-gather route on a small graph)
        return 0
    return int(lib().tipk_stream_gather_supported(n_table, d, max_split))


rel_stream_split = stream_gather_split


def rel_stream_piece():
    return int(lib().tipk_stream_gather_piece())


def dy_products_fused(r, nc, nb):
    """True when `dy_products` takes the fused one-pass kernel for this shape (it alone honours `row_used`)."""
    import ctypes as C
    s_c, s_r = C.c_int(0), C.c_int(0)
    if switches.on('TIPK_NO_DY_FUSED'):
        return False
    check(lib().tipk_rgcn_dy_products_plan(r, nc, nb, C.byref(s_c), C.byref(s_r)), 'tipk_rgcn_dy_products_plan')
    return s_c.value != 0


def stream_gather(sp, table, row_scale=None, write_zeros=True, out=None, label='stream_gather', kind=0, max_split=4,
                  out_scale=None, bias=None, relu=False):
    """out[row] = sum of table rows on a wave-stream plan (include/tipk.h section 1d), table [n_table, d] staged
    in LDS (scaled per row while staged).  write_zeros=False leaves the rows without edges UNTOUCHED: only for
    a consumer that masks them (`dy_products(row_used=...)`) or an `out` buffer that was zeroed once.
    Epilogue of a finished row: relu?(out_scale[row] * sum + bias)."""
    table = _f32c(table)
    require_device(table, sp.ids, row_scale, out_scale, bias)
    d = table.shape[1]
    split = stream_gather_split(sp.n_table, d, max_split)
    assert table.shape[0] == sp.n_table and split and (d // split) * 4 == sp.row_bytes, 'plan was built for another launch shape'
    assert table.stride(1) == 1
    if out is None:
        out = torch.empty((sp.n_rows, d), dtype=torch.float32, device=table.device)
    assert out.shape == (sp.n_rows, d) and out.is_contiguous()
    with _timed('%s[d=%d]' % (label, d)):
        check(lib().tipk_stream_gather(ptr(table), table.stride(0), sp.n_table, d, sp.n_wg, ptr(sp.wave_ptr), ptr(sp.cells),
                                       ptr(sp.ids), sp.idx_unit, ptr(sp.zero_ptr) if write_zeros else None,
                                       ptr(sp.zero_rows), ptr(row_scale), ptr(out), d, kind, max_split, ptr(out_scale),
                                       ptr(bias), int(bool(relu)), stream_ptr(table.device)),
              'tipk_stream_gather')
    return out


def stream_gather_two(sp, table0, table1, out0, out1, label='pair_cells2[dd.fwd]'):
    """out0[row] = sum of table0 rows, out1[row] = sum of table1 rows on ONE wave-stream plan in one launch
    (`tipk_stream_gather_two`): the pair cells of both R-GCN layers of an encoder.  Rows without edges stay untouched."""
    table0, table1 = _f32c(table0), _f32c(table1)
    require_device(table0, table1, sp.ids, out0, out1)
    d = table0.shape[1]
    assert table0.shape == table1.shape == (sp.n_table, d) and table0.stride() == table1.stride() and table0.stride(1) == 1
    assert out0.shape == out1.shape == (sp.n_rows, d) and out0.is_contiguous() and out1.is_contiguous()
    assert stream_gather_split(sp.n_table, d, 1) == 1 and d * 4 == sp.row_bytes, 'plan was built for another launch shape'
    with _timed('%s[d=%d]' % (label, d)):
        check(lib().tipk_stream_gather_two(ptr(table0), ptr(table1), table0.stride(0), sp.n_table, d, sp.n_wg, ptr(sp.wave_ptr),
                                           ptr(sp.cells), ptr(sp.ids), sp.idx_unit, ptr(out0), ptr(out1), d,
                                           stream_ptr(table0.device)), 'tipk_stream_gather_two')


def pair_cells_partner_ok(graph, att, graph2, att2, n):
    """True when the pair cells of a second layer (graph2, att2) can be gathered in the launch that gathers (graph, att)'s:
    the same plan shape (the layers share the D-D graph), att tables of one shape, one column block."""
    if switches.on('TIPK_NO_CELLS_TWO'):
        return False
    p1, p2 = graph.pair_fwd, graph2.pair_fwd
    if p1 is None or p2 is None or att.shape != att2.shape or att.stride() != att2.stride():
        return False
    r, nb = att.shape
    return (p1.n_table == p2.n_table == r and p1.n_rows == p2.n_rows == n * n and p1.n_bands == p2.n_bands and p1.n_wg == p2.n_wg
            and p1.lanes == p2.lanes and p1.idx_unit == p2.idx_unit and p1.symmetric == p2.symmetric
            and stream_gather_split(r, nb, 1) == 1 and nb // 4 == p1.lanes and nb >= 16)


def rel_stream_bwd(sp, table, row_scale=None, write_zeros=True):
    """Transposed D-D pass: table = g [N, d] -> dY (plan of `build_stream_plan`): [R * N, d], or -- compact plans --
    [n_rows + 1, d] node-major with a trailing zero row (a buffer kept ON THE PLAN per width: the zero row is written
    once, every call rewrites all the other rows; it lives exactly as long as the plan, i.e. as the layer's graph, so a
    captured hipGraph that baked its address in never sees it freed or handed to someone else)."""
    if sp.compact is None:
        return stream_gather(sp, table, row_scale, write_zeros, label='rel_stream[dd.bwd]')
    d = table.shape[1]
    key = (d, str(table.device))
    buf = sp.dyc.get(key)
    if buf is None:
        buf = sp.dyc[key] = torch.zeros((sp.n_rows + 1, d), dtype=torch.float32, device=table.device)
    stream_gather(sp, table, row_scale, write_zeros=False, out=buf[:sp.n_rows], label='rel_stream[dd.bwd]')
    return buf


def _strides3(t):
    """(batch stride, row stride, col stride) of a 2-D (batch stride 0) or 3-D tensor."""
    if t.dim() == 2:
        return 0, t.stride(0), t.stride(1)
    return t.stride(0), t.stride(1), t.stride(2)


def _tile_shape(m, n):
    """(BM, BN) the kernel picks (tip_amd/csrc/tipk_gemm.hip: 4x1, 1x4 or 2x2 waves of 32x32)."""
    if n <= 32:
        return 128, 32
    if m <= 32:
        return 32, 128
    return 64, 64


class GemmJob(object):
    """One product prepared for launch: the descriptor, the slab buffer of a split reduction and
    the ordered slab sum that finishes it.  `gemm` runs one job; `gemm_group` runs several
    independent jobs in one grouped launch (+ one grouped slab sum)."""
    __slots__ = ('desc', 'label', 'slabs', 'n_slabs', 'per', 'alpha', 'accumulate', 'out', 'keep', 'gate')


def gemm_job(a, b, out=None, c_in=None, relu=False, alpha=1.0, reduce_batch=False, ksplit=None, kgroup=None):
    """Prepare out = relu?(alpha * a @ b + c_in) on the matrix cores (include/tipk.h section 2).

    a: [M,K] or [Z,M,K]; b: [K,N] or [Z,K,N] -- arbitrary strides (transposed views are free).
    reduce_batch: sum the Z products into one [M,N] (the basis-sum of the R-GCN backward).
    ksplit: K slabs (None = automatic).  Products with few output tiles but a long reduction
    (dW = g^T h over 19 081 proteins, X^T g over 645 drugs, att^T dY over 1 097 relations) would
    run as a handful of serial workgroups; they are cut into slabs that fill the chip and the
    slabs are added in order by `tipk_sum_slabs` (deterministic, no atomics).
    kgroup (with reduce_batch): the Z batch terms are summed in groups of `kgroup` consecutive terms, one
    slab per group -- sum_z a[z] @ b[z] with Z in the hundreds (the pair-form D-D product: one term per
    source node), where one slab per term would be as large as the operands.
    """
    require_device(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise _lib.TipkError('gemm: fp32 only')
    z = max(a.shape[0] if a.dim() == 3 else 1, b.shape[0] if b.dim() == 3 else 1)
    batched = a.dim() == 3 or b.dim() == 3
    m, k = a.shape[-2], a.shape[-1]
    k2, n = b.shape[-2], b.shape[-1]
    assert k == k2, (a.shape, b.shape)
    a_sz, a_sm, a_sk = _strides3(a)
    b_sz, b_sk, b_sn = _strides3(b)
    reduce_batch = bool(reduce_batch and batched)
    oshape = (z, m, n) if (batched and not reduce_batch) else (m, n)
    dev = a.device
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=dev)
    assert tuple(out.shape) == oshape and out.stride(-1) == 1, (out.shape, oshape, out.stride())
    if c_in is not None:
        assert c_in.shape == out.shape and c_in.stride(-1) == 1

    bm, bn = _tile_shape(m, n)
    tiles = -(-m // bm) * -(-n // bn) * (1 if reduce_batch else z)
    plain = relu is False and (c_in is None or c_in.data_ptr() == out.data_ptr()) and out.is_contiguous()
    slab_mode = None                       # None | 'k' (split the k range) | 'q' (one slab per batch term) | 'g' (per group of terms)
    n_slabs = 0
    if kgroup:
        # (c_in == out: the slab sum accumulates on top of what `out` holds, as in mode 'q')
        assert reduce_batch and plain and z % kgroup == 0 and a.dim() == 3 and b.dim() == 3
        slab_mode, n_slabs = 'g', z // kgroup
    elif reduce_batch and plain and tiles * 2 <= 256 and z > 1:
        slab_mode, n_slabs = 'q', z
    elif ksplit is None:
        # a workgroup's K loop is a chain of dependent ~1.5 us load round trips: small products are cut
        # until a slab is one or two K tiles (the three constants were swept in rounds 2 and 3: all at their optimum)
        grain, wgs = 64, 512
        cap = 320                                               # (K = 19 081: 299 slabs of two K tiles; 128 slabs made five-tile chains)
        # (ceil: K = 645 -> 11 slabs of 64 = two K tiles each; 10 slabs made the chunk 96 = three tiles, three slabs empty)
        want = min(-(-k // grain), -(-wgs // tiles))
        if plain and not reduce_batch and want >= 2 and tiles < 256:
            slab_mode, n_slabs = 'k', int(min(cap, want))
    elif ksplit > 1:
        assert plain and not reduce_batch
        slab_mode, n_slabs = 'k', int(ksplit)

    g = GemmDesc()
    g.m, g.n, g.k = m, n, k
    g.a, g.b = a.data_ptr(), b.data_ptr()
    g.a_sm, g.a_sk, g.b_sk, g.b_sn = a_sm, a_sk, b_sk, b_sn
    g.ksplit = n_slabs if slab_mode == 'k' else 1
    if slab_mode == 'g':
        g.batch, g.kbatch = n_slabs, kgroup
        g.a_sq, g.b_sq, g.a_sz, g.b_sz = a_sz, b_sz, a_sz * kgroup, b_sz * kgroup
    elif reduce_batch and slab_mode != 'q':
        g.batch, g.kbatch = 1, z
        g.a_sq, g.b_sq, g.a_sz, g.b_sz = a_sz, b_sz, 0, 0
    else:
        g.batch, g.kbatch = (z if batched else 1), 1
        g.a_sq, g.b_sq, g.a_sz, g.b_sz = 0, 0, a_sz, b_sz
    slabs = None
    per = m * n * (z if (batched and not reduce_batch) else 1)       # floats of the final result
    if slab_mode == 'k':
        slabs = torch.empty((n_slabs,) + oshape, dtype=torch.float32, device=dev)
        g.c, g.c_sm, g.c_sz, g.c_ss = slabs.data_ptr(), n, m * n, per
    elif slab_mode in ('q', 'g'):
        slabs = torch.empty((n_slabs, m, n), dtype=torch.float32, device=dev)
        g.c, g.c_sm, g.c_sz, g.c_ss = slabs.data_ptr(), n, m * n, 0
    else:
        g.c, g.c_sm = out.data_ptr(), out.stride(-2)
        g.c_sz = out.stride(0) if out.dim() == 3 else 0
        g.c_ss = 0
    if c_in is not None and slab_mode is None:
        g.c_in, g.cin_sm = c_in.data_ptr(), c_in.stride(-2)
        g.cin_sz = c_in.stride(0) if c_in.dim() == 3 else 0
    else:
        g.c_in, g.cin_sm, g.cin_sz = None, 0, 0
    g.alpha, g.relu = (1.0 if slab_mode else alpha), int(relu)

    job = GemmJob()
    job.desc, job.slabs, job.n_slabs, job.per, job.alpha, job.out = g, slabs, n_slabs, per, alpha, out
    job.accumulate = c_in is not None
    job.gate = None                                                  # set by the caller: mask of the finished sum
    job.keep = (a, b, c_in)                                          # operands stay alive until launched
    job.label = '%dx%dx%d,z=%d%s' % (m, n, k, z, ',slabs=%s%d' % (slab_mode, n_slabs) if slab_mode else '')
    return job


def large_kgroup(m, z):
    """Batch-reduced products over a LARGE node set (config 5: [10 000 x 128] x [128 x 128] summed over 32 bases) have few
    output tiles (314) and a reduction of 4 096: four slabs of 8 bases each fill the chip (255 -> 169 us)."""
    return 8 if (m >= 4096 and z >= 16 and z % 8 == 0) else None


def gemm(a, b, out=None, c_in=None, relu=False, alpha=1.0, reduce_batch=False, ksplit=None, kgroup=None):
    """out = relu?(alpha * a @ b + c_in): one product, launched now (see `gemm_job`)."""
    job = gemm_job(a, b, out, c_in, relu, alpha, reduce_batch, ksplit, kgroup)
    st = stream_ptr(a.device)
    with _timed('gemm[%s]' % job.label):
        check(lib().tipk_gemm_f32(job.desc, st), 'tipk_gemm_f32')
        if job.slabs is not None:
            check(lib().tipk_sum_slabs(ptr(job.slabs), job.n_slabs, job.per, job.per, job.alpha,
                                       int(job.accumulate), ptr(job.out), st), 'tipk_sum_slabs')
    return job.out


def dy_products(g_y, att, xb2, row_used=None, n_nodes=0):
    """(d att, d XB) = (g_y @ xb2^T, att^T @ g_y) in ONE pass over g_y [R, N*out] (include/tipk.h
    section 2b); falls back to two grouped GEMMs for shapes the fused kernel does not take."""
    import ctypes as C
    r, nc = g_y.shape
    nb = att.shape[1]
    s_c, s_r = C.c_int(0), C.c_int(0)
    if not switches.on('TIPK_NO_DY_FUSED') and g_y.stride(1) == 1 and att.stride(1) == 1 and xb2.stride(1) == 1:
        check(lib().tipk_rgcn_dy_products_plan(r, nc, nb, C.byref(s_c), C.byref(s_r)), 'tipk_rgcn_dy_products_plan')
    if s_c.value == 0:
        assert row_used is None, 'the two-GEMM path reads every row of dY'
        g_att, g_xb = gemm_group([gemm_job(g_y, xb2.t()), gemm_job(att.t(), g_y)])
        return g_att, g_xb
    dev = g_y.device
    dxb_slabs = torch.empty((s_r.value, nb, nc), dtype=torch.float32, device=dev)
    datt_slabs = torch.empty((s_c.value, r, nb), dtype=torch.float32, device=dev)
    with _timed('dy_products[%dx%dx%d]' % (r, nc, nb)):
        check(lib().tipk_rgcn_dy_products(ptr(g_y), g_y.stride(0), ptr(att), att.stride(0), ptr(xb2), xb2.stride(0),
                                          r, nc, nb, ptr(row_used), n_nodes, ptr(dxb_slabs), ptr(datt_slabs), stream_ptr(dev)),
              'tipk_rgcn_dy_products')
    j_att = slab_job(datt_slabs)
    if s_r.value == 1:                                   # one row range: the slab IS d XB
        gemm_group([], [j_att])
        return j_att.out, dxb_slabs[0]
    j_xb = slab_job(dxb_slabs)
    gemm_group([], [j_xb, j_att])
    return j_att.out, j_xb.out


def node_products_slabs(n_nodes, d, n_rel, nb):
    """d att slabs `node_products` produces for this shape; 0 = shape not supported (dense `dy_products` then)."""
    import ctypes as C
    g = C.c_int(0)
    check(lib().tipk_rgcn_node_products_plan(n_nodes, d, n_rel, nb, C.byref(g)), 'tipk_rgcn_node_products_plan')
    return g.value


def node_products(dyc, cr, att, xb, xbt=None):
    """(pending slab sum of d att, d XB [bases, N, d]) from the COMPACT node-major dY (include/tipk.h section 2d):
    dyc [n_rows + 1, d] as written by `stream_gather` on a compact plan (last row zero), cr = plan.compact,
    xb [bases, N, d]; xbt (optional) the same values as a contiguous [N, d, bases] (read coalesced by the d att product).
    d XB is complete; the d att slabs are summed by the caller's next grouped slab sum."""
    n_rows, d = dyc.shape[0] - 1, dyc.shape[1]
    nb, n = xb.shape[0], xb.shape[1]
    r = att.shape[0]
    assert cr.n_rows == n_rows and xb.shape[2] == d and xb.stride(2) == 1 and att.stride(1) == 1 and dyc.is_contiguous()
    assert xb.stride(0) % 4 == 0 and xb.stride(1) % 4 == 0
    assert xbt is None or (tuple(xbt.shape) == (n, d, nb) and xbt.is_contiguous() and xbt.dtype == torch.float32)
    g = node_products_slabs(n, d, r, nb)
    assert g > 0
    dev = dyc.device
    dxb = torch.empty((nb, n, d), dtype=torch.float32, device=dev)
    datt_slabs = torch.empty((g, r, nb), dtype=torch.float32, device=dev)
    with _timed('node_products[%dx%dx%d,rows=%d]' % (r, n * d, nb, n_rows)):
        check(lib().tipk_rgcn_node_products(ptr(dyc), n_rows, d, ptr(cr.node_desc), ptr(cr.row_rel), ptr(cr.pos),
                                            n, r, ptr(att), att.stride(0), nb, ptr(xb), xb.stride(0),
                                            xb.stride(1), ptr(xbt), ptr(dxb), dxb.stride(0), dxb.stride(1), ptr(datt_slabs),
                                            stream_ptr(dev)), 'tipk_rgcn_node_products')
    return slab_job(datt_slabs), dxb


def dest_products_bits(n_nodes, n_rel, nb, d_in):
    """bits of the relation field of a destination-major edge word (`tipk_rgcn_dest_products`); 0 = shape not supported."""
    if switches.on('TIPK_NO_DEST_FWD'):
        return 0
    return int(lib().tipk_rgcn_dest_products_supported(int(n_nodes), int(n_rel), int(nb), int(d_in)))


def dest_products(dp, x, att):
    """T[b, v, :] = sum over the edges e -> v of att[r_e, b] * x[src_e, :]  (include/tipk.h section 2f) on a `plan.DestPlan`:
    x [N, d_in], att [R, bases] -> T [bases, N, d_in]."""
    x, att = _f32c(x), _f32c(att)
    require_device(x, att, dp.edges)
    n, d_in = x.shape
    r, nb = att.shape
    assert dp.n_nodes == n and dp.n_rel == r
    t = torch.empty((nb, n, d_in), dtype=torch.float32, device=x.device)
    with _timed('dest_products[%dx%dx%d,edges=%d]' % (n, nb, d_in, dp.n_edges)):
        check(lib().tipk_rgcn_dest_products(ptr(x), x.stride(0), d_in, ptr(att), att.stride(0), nb, n, r, ptr(dp.node_desc),
                                            ptr(dp.edges), ptr(t), t.stride(0), t.stride(1), stream_ptr(x.device)),
              'tipk_rgcn_dest_products')
    return t


def row_products_supported(n_nodes, n_rel, nb, channels):
    if switches.on('TIPK_NO_ROW_PRODUCTS'):
        return False
    return bool(lib().tipk_rgcn_row_products_supported(int(n_nodes), int(n_rel), int(nb), int(channels)))


def row_products_s_supported(n_nodes, n_rel, nb, channels):
    if switches.on('TIPK_NO_ROW_PRODUCTS_S'):
        return False
    return bool(lib().tipk_rgcn_row_products_s_supported(int(n_nodes), int(n_rel), int(nb), int(channels)))


def _row_plan(graph, transposed, n, r, nb, channels):
    """The graph's row-stream plan for a pass over rows of `channels` floats, or None.  The kernel's own support query is asked
    BEFORE the (lazily built) plan is touched: building the per-lane plan for a node count it does not take would raise
    (plan.build_row_stream_plan: 16-bit node field), where the pass should fall through to the CSR / gather_sum route."""
    if not graph.has_row_plans:
        return None
    if graph.row_plans_wave_uniform:
        if channels % 64 != 0 or not row_products_s_supported(n, r, nb, channels) or n * channels * 4 >= 2 ** 31:
            return None
    elif not row_products_supported(n, r, nb, channels):
        return None
    return graph.row_bwd if transposed else graph.row_fwd


def row_products(rp, table, att, xb2=None):
    if getattr(rp, 'ROW_BYTES', None) is not None:
        return _row_products_s(rp, table, att, xb2)
    return _row_products_v(rp, table, att, xb2)


def _row_products_s(rp, table, att, xb2=None):
    """`tipk_rgcn_row_products_s` on a `plan.RowStreamPlanS` (wave-uniform entries): same results as the form below."""
    table, att = _f32c(table), _f32c(att)
    require_device(table, att, rp.entries)
    n, ch = table.shape
    r, nb = att.shape
    assert rp.n_nodes == n and rp.n_rel == r and table.stride(1) == 1 and att.stride(1) == 1
    entries = rp.entries_for(table.stride(0) * 4)
    t = torch.empty((nb, n, ch), dtype=torch.float32, device=table.device)
    slabs = None
    if xb2 is not None:
        assert xb2.shape == (nb, n * ch) and xb2.stride(1) == 1
        slabs = torch.empty((-(-n // 8) * (ch // 64), r, nb), dtype=torch.float32, device=table.device)
    with _timed('row_products_s[%dx%dx%d,edges=%d,%s]' % (n, nb, ch, rp.n_edges, 'T+datt' if slabs is not None else 'T')):
        check(lib().tipk_rgcn_row_products_s(ptr(table), table.stride(0), n, ch, ptr(att), att.stride(0), r, nb, ptr(entries),
                                             ptr(rp.desc), ptr(xb2), xb2.stride(0) if xb2 is not None else 0, ptr(t), ptr(slabs),
                                             stream_ptr(table.device)), 'tipk_rgcn_row_products_s')
    if slabs is None:
        return t
    return slab_job(slabs), t


def _row_products_v(rp, table, att, xb2=None):
    """The (relation, node) row sums S = sum of table rows over a row's edges, assembled in LDS, and their products
    (`tipk_rgcn_row_products`, include/tipk.h section 2h) on a `plan.RowStreamPlan`:
    table [N, ch], att [R, bases] -> T [bases, N, ch] = sum_r att[r, b] S[(r, v)];  with xb2 [bases, N * ch] also the slab
    job of d att [R, bases] = sum_v <S[(r, v)], XB[b, v]>  (returns (job, T); the caller's grouped slab sum finishes it)."""
    table, att = _f32c(table), _f32c(att)
    require_device(table, att, rp.entries)
    n, ch = table.shape
    r, nb = att.shape
    assert rp.n_nodes == n and rp.n_rel == r and table.stride(1) == 1 and att.stride(1) == 1
    if table.stride(0) % 64 != 0:                        # (the kernel multiplies `other << 8` by row bytes / 256: rows of 64 k floats)
        wide = torch.empty((n, -(-ch // 64) * 64), dtype=torch.float32, device=table.device)
        wide[:, :ch] = table
        table = wide[:, :ch]
    t = torch.empty((nb, n, ch), dtype=torch.float32, device=table.device)
    slabs = None
    if xb2 is not None:
        assert xb2.shape == (nb, n * ch) and xb2.stride(1) == 1
        slabs = torch.empty((int(lib().tipk_rgcn_row_products_slabs(n, ch)), r, nb), dtype=torch.float32, device=table.device)
    with _timed('row_products[%dx%dx%d,edges=%d,%s]' % (n, nb, ch, rp.n_edges, 'T+datt' if slabs is not None else 'T')):
        check(lib().tipk_rgcn_row_products(ptr(table), table.stride(0), n, ch, ptr(att), att.stride(0), r, nb, ptr(rp.entries),
                                           ptr(rp.desc), ptr(xb2), xb2.stride(0) if xb2 is not None else 0, ptr(t), ptr(slabs),
                                           stream_ptr(table.device)), 'tipk_rgcn_row_products')
    if slabs is None:
        return t
    return slab_job(slabs), t


def sum_slabs_xb(slabs, row_scale, addend, relu, x_out, basis, root, xb_pad):
    """x_out = relu?(row_scale * sum_s slabs[s] + addend) AND, in the same launch, the next layer's row-local products:
    xb_pad[:N, :, :d_out] = x_out basis (node-major, rows padded to 32 columns) and the returned x_out root
    (`tipk_sum_slabs_xb`, include/tipk.h section 2g).  slabs [S, N, 32], basis [bases, 32, d_out], root [32, d_out]."""
    require_device(slabs, x_out, basis, root, xb_pad)
    s_, n, d_in = slabs.shape
    nb, _, d_out = basis.shape
    assert slabs.is_contiguous() and x_out.is_contiguous() and x_out.shape == (n, d_in) and basis.is_contiguous() and root.is_contiguous()
    assert xb_pad.stride()[-2:] == (32, 1) and xb_pad.shape[1] == nb and xb_pad.stride(0) == nb * 32 and xb_pad.shape[0] >= n
    assert addend is None or (addend.is_contiguous() and addend.shape == (n, d_in))
    xroot = torch.empty((n, d_out), dtype=torch.float32, device=slabs.device)
    with _timed('sum_slabs_xb[%dx%d -> %dx%d]' % (s_, n * d_in, nb, d_out)):
        check(lib().tipk_sum_slabs_xb(ptr(slabs), s_, n * d_in, n, d_in, ptr(row_scale), ptr(addend), int(bool(relu)), ptr(x_out),
                                      ptr(basis), ptr(root), nb, d_out, ptr(xb_pad), ptr(xroot), stream_ptr(slabs.device)),
              'tipk_sum_slabs_xb')
    return xroot


def sum_slabs_xb_supported(d_in, d_out):
    return d_in == 32 and 1 <= d_out <= 32 and not switches.on('TIPK_NO_LAYER_HANDOVER')


def pair_grads_supported(nb, d):
    return bool(lib().tipk_rgcn_pair_grads_supported(int(nb), int(d))) and not switches.on('TIPK_NO_PAIR_BWD')


def pair_grads(pb, cells, xb_pad, g, table=0):
    """The dense half of the pair-form backward pass of an R-GCN layer (include/tipk.h section 2e) on plan `pb`
    (plan.PairBwdPlan): cells = the cell buffer the forward pass filled ([N_pad, N, bases] + its trailing zeros, contiguous),
    xb_pad [N_pad, bases, 32] = the node-major XB buffer of the pair product, g [N, d] (1 / deg is in the plan's slots).
    -> (pg [2 n_alloc + 1, bases]: the gradient row of every linked pair at the place `pair_att_gather` stages it from,
    d XB [bases, N, d] complete)."""
    g = _f32c(g)
    require_device(cells, xb_pad, g, pb.slots)
    n, d = g.shape
    nb = cells.shape[-1]
    assert pb.n_nodes == n and g.stride(1) == 1 and cells.is_contiguous() and xb_pad.stride()[-2:] == (32, 1) and xb_pad.shape[1] == nb
    dev = g.device
    # `table`: which of the plan's gradient tables to fill -- layers that share the plan and whose d att gathers run in ONE
    # launch (tip_amd/encoder.py) need a table each
    key = str(dev) if table == 0 else (str(dev), int(table))
    pg = pb.pg.get(key)
    if pg is None:                                    # kept on the plan, zeroed ONCE: a call rewrites the rows of the linked pairs,
        pg = pb.pg[key] = torch.zeros((2 * pb.n_alloc + 1, nb), dtype=torch.float32, device=dev)   # the others stay zero
    dxb = torch.empty((nb, n, d), dtype=torch.float32, device=dev)
    with _timed('pair_grads[%dx%dx%d,slots=%d]' % (n, nb, d, pb.n_slots)):
        check(lib().tipk_rgcn_pair_grads(ptr(cells), cells.numel() // nb, ptr(xb_pad), ptr(g), g.stride(0), n, nb, d,
                                         ptr(pb.node_desc), ptr(pb.slots), ptr(pb.tile_node), pb.n_slots, ptr(dxb), dxb.stride(0), dxb.stride(1),
                                         ptr(pg), pg.shape[0], stream_ptr(dev)), 'tipk_rgcn_pair_grads')
    return pg, dxb


def pair_att_gather(pb, pg):
    """d att of the pair-form backward pass: per partition of the pairs one slab [R, bases] of sums of (symmetrised) rows of
    pg over the pairs each relation links (`tipk_stream_gather_parts`) -> the pending ordered slab sum (`slab_job`)."""
    require_device(pg, pb.part_first)
    nb = pg.shape[1]
    assert pg.shape[0] == 2 * pb.n_alloc + 1 and pg.is_contiguous()
    gp = pb.gather
    assert gp.lanes == 8, 'tipk_stream_gather_parts walks 128-byte rows with 8 lanes: the plan was built for another launch shape'
    slabs = torch.empty((pb.n_parts, pb.n_rel, nb), dtype=torch.float32, device=pg.device)
    with _timed('pair_att_gather[parts=%d,edges=%d]' % (pb.n_parts, gp.n_edges)):
        check(lib().tipk_stream_gather_parts(ptr(pg), nb, nb, pb.n_alloc, ptr(pb.part_first), pb.part_len, ptr(pb.wg_part), gp.n_wg,
                                             ptr(gp.wave_ptr), ptr(gp.cells), ptr(gp.ids), gp.idx_unit, ptr(gp.zero_ptr),
                                             ptr(gp.zero_rows), ptr(slabs), nb, stream_ptr(pg.device)), 'tipk_stream_gather_parts')
    return slab_job(slabs)


def pair_backward(pb, cells, xb_pad, g):
    """(pending slab sum of d att [R, bases], d XB [bases, N, d]): `pair_grads` + `pair_att_gather`."""
    pg, dxb = pair_grads(pb, cells, xb_pad, g)
    return pair_att_gather(pb, pg), dxb


class SlabJob(object):
    """An ordered slab sum with the fused epilogue of `sum_slabs`, prepared for a grouped launch."""
    __slots__ = ('desc', 'out', 'keep')


def slab_job(slabs, out=None, alpha=1.0, accumulate=False, row_scale=None, addend=None, relu=False, gate=None):
    assert slabs.is_contiguous()
    per = slabs[0].numel()
    if out is None:
        out = torch.empty(slabs.shape[1:], dtype=torch.float32, device=slabs.device)
    assert out.is_contiguous() and out.numel() == per
    if addend is not None:
        assert addend.is_contiguous() and addend.numel() == per
    d = SlabSumDesc()
    d.in_, d.n_slabs, d.slab_stride, d.count = slabs.data_ptr(), slabs.shape[0], per, per
    d.alpha, d.accumulate = alpha, int(accumulate)
    d.row_scale = row_scale.data_ptr() if row_scale is not None else None
    d.cols = slabs.shape[-1]
    d.addend = addend.data_ptr() if addend is not None else None
    d.relu, d.out = int(relu), out.data_ptr()
    if gate is not None:
        assert gate.is_contiguous() and gate.numel() == per
        d.gate = gate.data_ptr()
    job = SlabJob()
    job.desc, job.out, job.keep = d, out, (slabs, row_scale, addend, gate)
    return job


def _slab_desc_of(job):
    d = SlabSumDesc()
    d.in_, d.n_slabs, d.slab_stride, d.count = job.slabs.data_ptr(), job.n_slabs, job.per, job.per
    d.alpha, d.accumulate = job.alpha, int(job.accumulate)
    d.row_scale, d.cols, d.addend, d.relu, d.out = None, 0, None, 0, job.out.data_ptr()
    if job.gate is not None:
        assert job.gate.is_contiguous() and job.gate.numel() == job.per
        d.gate = job.gate.data_ptr()
    return d


def gemm_group(jobs, slab_jobs=(), defer_sums=False):
    """Run independent products in ONE grouped launch, then ONE grouped ordered slab sum for those
    that were split (plus any extra `slab_jobs` that are ready at the same point).  Results are
    bit-identical to running the jobs one by one.  Returns the jobs' outputs.
    defer_sums: do NOT launch the slab sums -- return them as a list of `slab_job`-like riders (the caller hands them
    to the next launch that takes riders: `gather_sum(..., riders=...)`); the jobs' outputs are complete only then."""
    jobs = list(jobs)
    slab_jobs = list(slab_jobs)
    if not jobs and not slab_jobs:
        return []
    dev = (jobs[0].out if jobs else slab_jobs[0].out).device
    st = stream_ptr(dev)
    # two members may share an output only as "written by the GEMM launch" + "slab sum accumulated on top"
    by_out = {}
    for j in jobs:
        by_out.setdefault(j.out.data_ptr(), []).append(j)
    for same in by_out.values():
        if len(same) > 1:
            direct = [j for j in same if j.slabs is None]
            assert len(direct) == 1 and all(j.accumulate for j in same if j.slabs is not None), \
                'group members sharing an output: one un-split product + accumulating slab sums only'
            assert len(same) == 2, 'at most one accumulating member per output (order of the sums)'
    for i in range(0, len(jobs), _lib.GROUP_MAX):
        part = jobs[i:i + _lib.GROUP_MAX]
        arr = (GemmDesc * len(part))(*[j.desc for j in part])
        with _timed('gemm_group[%s]' % ' | '.join(j.label for j in part)):
            check(lib().tipk_gemm_f32_group(arr, len(part), st), 'tipk_gemm_f32_group')
    sums = [_slab_desc_of(j) for j in jobs if j.slabs is not None] + [s.desc for s in slab_jobs]
    if defer_sums:
        riders = []
        for dsc, keep in zip(sums, [j for j in jobs if j.slabs is not None] + list(slab_jobs)):
            r = SlabJob()
            r.desc, r.out, r.keep = dsc, keep.out, keep
            riders.append(r)
        return riders
    for i in range(0, len(sums), _lib.GROUP_MAX):
        part = sums[i:i + _lib.GROUP_MAX]
        arr = (SlabSumDesc * len(part))(*part)
        with _timed('sum_slabs_group[%s]' % ' | '.join('%dx%d' % (d.n_slabs, d.count) for d in part)):
            check(lib().tipk_sum_slabs_group(arr, len(part), st), 'tipk_sum_slabs_group')
    return [j.out for j in jobs]


class WgGemmJob(object):
    """A product whose reduction runs inside one workgroup per output tile (`wg_gemm_group`)."""
    __slots__ = ('desc', 'out', 'keep', 'label')


def wg_gemm_job(a, b, out=None, reduce_batch=False, a2=None, b2=None, gate=None, alpha=1.0):
    """Prepare out = gate?(alpha * (a @ b [summed over the batch] + a2 @ b2)) for `wg_gemm_group` (include/tipk.h
    `tipk_gemm_wg_group`): a [M, K] or [Z, M, K], b [K, N] or [Z, K, N], arbitrary strides; a2 [M, K2], b2 [K2, N]
    optional (only without a surviving batch); gate: a tensor shaped like the output.  Returns None when the shape is
    not taken (reductions beyond 64 K tiles of 32, more than 4096 output tiles): the caller uses `gemm_job` then."""
    require_device(a, b)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    z = max(a.shape[0] if a.dim() == 3 else 1, b.shape[0] if b.dim() == 3 else 1)
    batched = a.dim() == 3 or b.dim() == 3
    m, k = a.shape[-2], a.shape[-1]
    k_b, n = b.shape[-2], b.shape[-1]
    assert k == k_b, (a.shape, b.shape)
    reduce_batch = bool(reduce_batch and batched)
    oshape = (z, m, n) if (batched and not reduce_batch) else (m, n)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=a.device)
    assert tuple(out.shape) == oshape and out.stride(-1) == 1, (out.shape, oshape, out.stride())
    a_sz, a_sm, a_sk = _strides3(a)
    b_sz, b_sk, b_sn = _strides3(b)
    d = WgGemmDesc()
    g = d.p
    g.m, g.n, g.k, g.ksplit = m, n, k, 1
    g.a, g.b = a.data_ptr(), b.data_ptr()
    g.a_sm, g.a_sk, g.b_sk, g.b_sn = a_sm, a_sk, b_sk, b_sn
    if reduce_batch:
        g.batch, g.kbatch = 1, z
        g.a_sq, g.b_sq, g.a_sz, g.b_sz = a_sz, b_sz, 0, 0
    else:
        g.batch, g.kbatch = (z if batched else 1), 1
        g.a_sq, g.b_sq, g.a_sz, g.b_sz = 0, 0, a_sz, b_sz
    g.c, g.c_sm = out.data_ptr(), out.stride(-2)
    g.c_sz = out.stride(0) if out.dim() == 3 else 0
    g.c_ss = 0
    g.c_in, g.cin_sm, g.cin_sz = None, 0, 0
    g.alpha, g.relu = alpha, 0
    if a2 is not None:
        require_device(a2, b2)
        assert a2.dim() == 2 and b2.dim() == 2 and a2.shape[0] == m and b2.shape[1] == n and a2.shape[1] == b2.shape[0]
        assert a2.dtype == torch.float32 and b2.dtype == torch.float32 and len(oshape) == 2
        d.a2, d.a2_sm, d.a2_sk = a2.data_ptr(), a2.stride(0), a2.stride(1)
        d.b2, d.b2_sk, d.b2_sn = b2.data_ptr(), b2.stride(0), b2.stride(1)
        d.k2 = a2.shape[1]
    if gate is not None:
        require_device(gate)
        assert tuple(gate.shape) == oshape and gate.stride(-1) == 1 and gate.dtype == torch.float32
        d.gate, d.gate_sm = gate.data_ptr(), gate.stride(-2)
        d.gate_sz = gate.stride(0) if gate.dim() == 3 else 0
    if not lib().tipk_gemm_wg_group_supported(d):
        return None
    job = WgGemmJob()
    job.desc, job.out, job.keep = d, out, (a, b, a2, b2, gate)
    job.label = '%dx%dx%d,z=%d%s' % (m, n, k, z, '+%d' % a2.shape[1] if a2 is not None else '')
    return job


def wg_gemm_group(jobs, slab_jobs=()):
    """Run up to 4 `wg_gemm_job`s and up to 3 ordered slab sums (`slab_job`) in ONE launch; returns the products' outputs."""
    jobs, slab_jobs = list(jobs), list(slab_jobs)
    assert len(jobs) <= _lib.WG_GEMM_MAX and len(slab_jobs) <= _lib.WG_SUMS_MAX and (jobs or slab_jobs)
    dev = (jobs[0].out if jobs else slab_jobs[0].out).device
    arr = (WgGemmDesc * max(1, len(jobs)))(*[j.desc for j in jobs])
    sums = (SlabSumDesc * max(1, len(slab_jobs)))(*[s.desc for s in slab_jobs])
    with _timed('wg_gemm_group[%s%s]' % (' | '.join(j.label for j in jobs),
                                          ''.join(' | sum %dx%d' % (s.desc.n_slabs, s.desc.count) for s in slab_jobs))):
        check(lib().tipk_gemm_wg_group(arr, len(jobs), sums, len(slab_jobs), stream_ptr(dev)), 'tipk_gemm_wg_group')
    return [j.out for j in jobs]


def transpose(x):
    """x^T as a row-major tensor; a view when x is stored column-major already (no launch)."""
    if x.dim() == 2 and x.t().is_contiguous() and x.dtype == torch.float32:
        return x.t()
    x = _f32c(x).contiguous()
    require_device(x)
    out = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float32, device=x.device)
    check(lib().tipk_transpose(ptr(x), x.shape[0], x.shape[1], ptr(out), stream_ptr(x.device)), 'tipk_transpose')
    return out


def rows_affine(x, row_mul=None, row_div=None, gate=None, out=None, accumulate=False):
    """out (+)= x * row_mul / row_div * (gate > 0); x/out/gate may be column-slice views."""
    x = _f32c(x)
    require_device(x)
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
        assert not accumulate
    assert out.shape == x.shape and out.stride(1) == 1
    if gate is not None:
        gate = _f32c(gate)
    check(lib().tipk_rows_affine(ptr(x), x.stride(0), ptr(row_mul), ptr(row_div), ptr(gate),
                                 gate.stride(0) if gate is not None else 0, ptr(out), out.stride(0), rows, cols,
                                 int(accumulate), stream_ptr(x.device)), 'tipk_rows_affine')
    return out


def gate_colsum(x, gate):
    """(x * (gate > 0), partial column sums [G, 1, cols] of it) in one pass; None if unsupported.
    (Round 4: letting the launch's LAST workgroup add the partial rows behind a ticket -- no sum_slabs launch -- made the
    step 16 us SLOWER: handing data between workgroups inside a launch takes a device-scope release in every workgroup,
    i.e. an L2 write-back per XCD on MI355X.)"""
    x, gate = _f32c(x), _f32c(gate)
    require_device(x, gate)
    rows, cols = x.shape
    groups = int(lib().tipk_gate_colsum_groups(rows, cols))
    if groups == 0:
        return None
    out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    scratch = torch.empty((groups, 1, cols), dtype=torch.float32, device=x.device)
    check(lib().tipk_gate_colsum(ptr(x), x.stride(0), ptr(gate), gate.stride(0), ptr(out), out.stride(0), rows, cols,
                                 ptr(scratch), stream_ptr(x.device)), 'tipk_gate_colsum')
    return out, scratch


def col_sum(x):
    x = _f32c(x)
    require_device(x)
    rows, cols = x.shape
    scratch = torch.empty((256, cols), dtype=torch.float32, device=x.device)
    out = torch.empty((cols,), dtype=torch.float32, device=x.device)
    check(lib().tipk_col_sum(ptr(x), x.stride(0), rows, cols, ptr(scratch), ptr(out), stream_ptr(x.device)),
          'tipk_col_sum')
    return out


def _idx_bytes(t):
    if t.dtype == torch.int64:
        return 8
    if t.dtype == torch.int32:
        return 4
    raise _lib.TipkError('index tensors must be int32 or int64, got %s' % t.dtype)


def _uv(edge_index):
    ei = edge_index if edge_index.is_contiguous() else edge_index.contiguous()
    return ei[0], ei[1]


# Derived facts about an index tensor (range verdict, packed copy) are kept in a SIDE TABLE keyed by the tensor object,
# not as attributes on it: `torch.save(model)` (tip.py:36) pickles a tensor's __dict__, so attributes would put a 4 E-byte
# packed copy into every checkpoint and restore a stale "range ok" verdict on load (a loaded tensor's version counter
# restarts at 0).  An entry dies with its tensor (weakref finalizer) and is only trusted while the tensor's version,
# storage address and shape are what they were when it was made.
_TENSOR_FACTS = {}


def _facts(t):
    """The side-table entry (a dict) of tensor `t`, emptied if `t` was modified, re-pointed or re-shaped since."""
    import weakref
    tag = (t._version, t.data_ptr(), tuple(t.shape), str(t.device))
    ent = _TENSOR_FACTS.get(id(t))
    if ent is None or ent[0]() is not t:
        ent = _TENSOR_FACTS[id(t)] = [weakref.ref(t), tag, {}]
        weakref.finalize(t, _TENSOR_FACTS.pop, id(t), None)
    elif ent[1] != tag:
        ent[1], ent[2] = tag, {}
    return ent[2]


def _range_checked(t, limit, what):
    """Raise IndexError unless every entry of the index tensor `t` lies in [0, limit).  The verdict is remembered per
    tensor OBJECT (`_facts`: keyed by version counter, storage address, shape): no global cache pins index tensors, a
    tensor that was modified in place -- or unpickled -- is checked again, and a fresh tensor costs ONE fused device
    reduction and one sync."""
    facts = _facts(t)
    if facts.get('range_ok') == int(limit):
        return
    if t.numel():
        lo, hi = torch.stack([t.min(), t.max()]).tolist()
        if lo < 0 or hi >= limit:
            raise IndexError('%s id out of range: [%d, %d] for %d' % (what, lo, hi, limit))
    facts['range_ok'] = int(limit)


def validate_triples(edge_index, edge_type, n_nodes, n_rel):
    """Range check of a triple list, done ONCE per tensor (the verdict is stored on the tensor, so the per-step cost
    is an attribute lookup): the decoder kernels index the LDS images of z / d z with 16-bit node ids and `weight`
    rows with the relation id, so an out-of-range id would corrupt memory silently where the reference raises
    IndexError.  (A first-time check synchronises: do not meet it inside a hipGraph capture -- the warm-up steps of
    tip_amd.train.GraphedTrainStep take care of that.)"""
    n = edge_index.shape[-1]
    if n >= 2 ** 31:
        raise ValueError('triple lists are indexed with 32-bit positions: %d >= 2^31' % n)
    _range_checked(edge_index, n_nodes, 'node')
    if edge_type is not None:
        if edge_type.numel() != n:
            raise ValueError('edge_type has %d entries for %d triples' % (edge_type.numel(), n))
        _range_checked(edge_type, n_rel, 'relation')


_TASK_CACHE = DerivedCache(16)
TASK_POSITIONS = 2048          # = TASK_MAX in tipk_distmult.hip (a task's ids are staged in LDS)


def relation_tasks(edge_type, pos_index=None):
    """int32 [T,4] (relation, begin, end, pos_weight) tasks for the LDS-resident decoder kernels, or
    None when the triples are not grouped by relation (include/tipk.h section 4).  Built once per tensor(s)
    (`_cache.DerivedCache`; None is cached like a task list).

    pos_index: the positive triples of the fused objective.  If every relation's block is
    [pairs | the same pairs mirrored] (the data contract of the path, src/utils.py:35-65 -- verified
    here, element by element), the first half gets weight 2 and the mirrored half weight 0."""
    return _TASK_CACHE.get((edge_type, pos_index), None, lambda: _relation_tasks(edge_type, pos_index))


def _relation_tasks(edge_type, pos_index):
    tasks = None
    if edge_type.numel():
        rels, counts = torch.unique_consecutive(edge_type, return_counts=True)
        if torch.unique(rels).numel() == rels.numel():                      # each relation is one run
            start = torch.cumsum(counts, 0) - counts
            dev = rels.device
            mirrored = False
            if pos_index is not None and not switches.on('TIPK_NO_SYMMETRIC_POS') and bool((counts % 2 == 0).all()):
                half = counts // 2
                pos = torch.arange(edge_type.numel(), device=dev)
                run_of = torch.repeat_interleave(torch.arange(rels.numel(), device=dev), counts)
                first = pos < (start + half)[run_of]
                partner = torch.where(first, pos + half[run_of], pos - half[run_of])
                u, v = pos_index[0], pos_index[1]
                mirrored = bool(((u == v[partner]) & (v == u[partner])).all())
            if mirrored:                                                    # two segments per relation
                seg_rel = torch.repeat_interleave(rels, 2)
                seg_cnt = torch.repeat_interleave(counts // 2, 2)
                seg_start = torch.stack([start, start + counts // 2], dim=1).view(-1)
                seg_w = torch.tensor([2, 0], device=dev).repeat(rels.numel())
            else:
                seg_rel, seg_cnt, seg_start = rels, counts, start
                seg_w = torch.ones_like(rels)
            n_chunks = (seg_cnt + TASK_POSITIONS - 1) // TASK_POSITIONS
            run = torch.repeat_interleave(torch.arange(seg_rel.numel(), device=dev), n_chunks)
            first_c = torch.cumsum(n_chunks, 0) - n_chunks
            local = torch.arange(run.numel(), device=dev) - first_c[run]
            begin = seg_start[run] + local * TASK_POSITIONS
            end = torch.minimum(begin + TASK_POSITIONS, seg_start[run] + seg_cnt[run])
            # heavier tasks first: a weight-2 / weight-1 position costs two evaluations, a weight-0 one
            cost = (end - begin) * (1 + (seg_w[run] > 0).long())
            order = torch.sort(cost, descending=True, stable=True).indices
            tasks = torch.stack([seg_rel[run], begin, end, seg_w[run]], dim=1)[order].to(torch.int32).contiguous()
    return tasks


def distmult_fwd(z, weight, edge_index, edge_type, sigmoid=True):
    z, weight = _f32c(z).contiguous(), _f32c(weight).contiguous()
    require_device(z, weight, edge_index, edge_type)
    validate_triples(edge_index, edge_type, z.shape[0], weight.shape[0])
    u, v = _uv(edge_index)
    et = edge_type.contiguous()
    n = u.numel()
    score = torch.empty((n,), dtype=torch.float32, device=z.device)
    check(lib().tipk_distmult_fwd(ptr(z), z.shape[0], z.shape[1], ptr(weight), weight.shape[0], ptr(u), ptr(v),
                                  _idx_bytes(u), ptr(et), _idx_bytes(et), n, int(sigmoid), ptr(score),
                                  stream_ptr(z.device)), 'tipk_distmult_fwd')
    return score


def distmult_bwd(g_score, score, z, weight, edge_index, edge_type, sigmoid=True):
    z, weight = _f32c(z).contiguous(), _f32c(weight).contiguous()
    g_score = _f32c(g_score).contiguous()
    validate_triples(edge_index, edge_type, z.shape[0], weight.shape[0])
    u, v = _uv(edge_index)
    et = edge_type.contiguous()
    g_z, g_w = torch.zeros_like(z), torch.zeros_like(weight)
    tasks = relation_tasks(et)
    check(lib().tipk_distmult_bwd(ptr(g_score), ptr(score), ptr(z), z.shape[0], z.shape[1], ptr(weight),
                                  weight.shape[0], ptr(u), ptr(v), _idx_bytes(u), ptr(et), _idx_bytes(et),
                                  u.numel(), int(sigmoid), ptr(tasks), 0 if tasks is None else tasks.shape[0],
                                  ptr(g_z), ptr(g_w), stream_ptr(z.device)),
          'tipk_distmult_bwd')
    return g_z, g_w


def distmult_screen(z, rel_w, queries, k, known=None):
    """The k best candidates of every query by DistMult logit, known pairs dropped (include/tipk.h section 4c).

    queries: int [Q, 2] = (relation r, drug u), u = -1 for a relation query (all pairs u < v), else a drug query (all
    partners v != u); read on the host.  known: None or (keys int64 u*n+v sorted inside each relation, ptr int64
    [n_rel + 1]) on z's device -- the sampler's layout (`neg_sampling._cached_keys`); a list without keys drops nothing.
    -> (logits float32 [Q, k], u int32 [Q, k], v int32 [Q, k]), descending logit then ascending key; (-inf, -1, -1)
    pads a query with fewer than k candidates.  A candidate whose logit is NaN is never returned; +inf and -inf logits rank
    as values, so a -inf candidate is an entry (valid u and v, score -inf) ahead of the padding, not padding.  Synchronises the current stream once (the query list goes to the device)."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_screen')
    keys, kptr = _relation_known(known)
    q = torch.as_tensor(queries).to('cpu', torch.int32).reshape(-1, 2).contiguous()
    n, dim, n_q, k = z.shape[0], z.shape[1], q.shape[0], int(k)
    dev = z.device
    out_s, out_u, out_v = _topk_outputs(n_q, k, 2, dev)
    ws_bytes = int(lib().tipk_distmult_screen_workspace_bytes(n, dim, n_q, k))
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    check(lib().tipk_distmult_screen(ptr(z), n, dim, ptr(rel_w), rel_w.shape[0], ptr(q), n_q, ptr(keys), ptr(kptr), k,
                                     ptr(out_s), ptr(out_u), ptr(out_v), ptr(ws), stream_ptr(dev)),
          'tipk_distmult_screen')
    return out_s, out_u, out_v


_PAIR_KNOWN = DerivedCache(8)


def known_relations_by_pair(edge_index, range_list, n_nodes, extra=None):
    """The pair-major known lists of include/tipk.h section 4d from edges grouped by relation -> (pair_keys int64
    strictly ascending min(u,v)*n+max(u,v), pair_ptr int64 [n_keys + 1], rel int32 ascending inside a pair's block), built
    with torch ops on edge_index's device (CPU tensors work too).  range_list [R, 2]: relation r owns the edge positions
    [begin, end) (the blocks tile the list in relation order).  Mirrored halves and duplicate edges collapse into one
    entry.  extra = (edge_index, range_list) of a second list to merge (train + test).  Cached (`_cache.DerivedCache`) per
    edge tensor(s) and range list(s) -- a range tensor by identity, a range given as a list by value; an edge_index given
    as a list is not cached."""
    def combined(ei, rl, n_rel):
        ends = torch.as_tensor(rl).to(device=ei.device, dtype=torch.int64).reshape(-1, 2)[:, 1].contiguous()
        rel = torch.bucketize(torch.arange(ei.shape[1], device=ei.device), ends, right=True)
        u, v = ei[0].to(torch.int64), ei[1].to(torch.int64)
        return (torch.minimum(u, v) * int(n_nodes) + torch.maximum(u, v)) * n_rel + rel

    def build():
        n_rel = int(torch.as_tensor(range_list).reshape(-1, 2).shape[0])
        c = combined(torch.as_tensor(edge_index), range_list, n_rel)
        if extra is not None:
            c = torch.cat([c, combined(torch.as_tensor(extra[0]).to(c.device), extra[1], n_rel)])
        c = torch.unique(c)                                              # sorted by (key, relation), duplicates gone
        keys, counts = torch.unique_consecutive(torch.div(c, n_rel, rounding_mode='floor'), return_counts=True)
        ptr = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=c.device)
        ptr[1:] = torch.cumsum(counts, 0)
        return keys.contiguous(), ptr, (c % n_rel).to(torch.int32).contiguous()

    more_ei, more_rl = (None, None) if extra is None else extra
    if not torch.is_tensor(edge_index) or not (extra is None or torch.is_tensor(more_ei)):
        return build()
    return _PAIR_KNOWN.get((edge_index, keyable(range_list), more_ei, None if extra is None else keyable(more_rl)),
                           int(n_nodes), build)


def _known_lists(known):
    """(keys, ptr, rel, n_keys) of a pair-major known list for the C entries: device tensors of the entries' types, or
    (None, None, None, 0) when there is nothing to drop."""
    keys = kptr = krel = None
    n_keys = 0
    if known is not None:
        keys, kptr, krel = known
        require_device(keys, kptr, krel)
        keys, kptr = keys.to(torch.int64).contiguous(), kptr.to(torch.int64).contiguous()
        krel = krel.to(torch.int32).contiguous()
        n_keys = keys.numel()
        if kptr.numel() != n_keys + 1:
            raise _lib.TipkError('known: pair_ptr has %d entries for %d keys' % (kptr.numel(), n_keys))
        if n_keys == 0 or krel.numel() == 0:                             # nothing to drop (empty tensors have no address)
            keys = kptr = krel = None
            n_keys = 0
    return keys, kptr, krel, n_keys


def _relation_known(known):
    """(keys, ptr) of a relation-major known list (`distmult_screen`) for the C entries: int64 contiguous device tensors, or
    (None, None) when there is nothing to drop -- None, or a list without keys (empty tensors have no address)."""
    if known is None:
        return None, None
    keys, kptr = known
    require_device(keys, kptr)
    if keys.numel() == 0:
        return None, None
    return keys.to(torch.int64).contiguous(), kptr.to(torch.int64).contiguous()


def _topk_outputs(n_rows, k, n_int, dev):
    """The [n_rows, max(k, 0)] outputs of a top-k entry on `dev`: the float32 scores, then n_int int32 tensors."""
    shape = (n_rows, max(int(k), 0))
    return (torch.empty(shape, dtype=torch.float32, device=dev),) \
        + tuple(torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(n_int))


def _distmult_operands(z, rel_w, who):
    """z [n, dim] and rel_w [n_rel, dim] as contiguous fp32 device tensors for the entry `who`."""
    z, rel_w = _f32c(z).contiguous(), _f32c(rel_w).contiguous()
    require_device(z, rel_w)
    if z.dim() != 2 or rel_w.dim() != 2 or rel_w.shape[1] != z.shape[1]:
        raise _lib.TipkError('%s: z [n, dim] and rel_w [n_rel, dim] expected, got %s and %s'
                             % (who, tuple(z.shape), tuple(rel_w.shape)))
    return z, rel_w


def _table_pair(t1, t2, who, shape='[n, n_rel]'):
    """Two decoder tables of one shape as fp32 device tensors the table entries of `who` can read.  The entries take ONE row
    stride and know no column stride: tables whose row strides differ or are shorter than a row, or whose column stride is
    not 1, are made contiguous."""
    t1, t2 = _f32c(t1), _f32c(t2)
    require_device(t1, t2)
    if t1.dim() != 2 or t1.shape != t2.shape:
        raise _lib.TipkError('%s: two tables %s expected, got %s and %s' % (who, shape, tuple(t1.shape), tuple(t2.shape)))
    if t1.stride(0) != t2.stride(0) or t1.stride(0) < t1.shape[1] or t1.stride(1) != 1 or t2.stride(1) != 1:
        t1, t2 = t1.contiguous(), t2.contiguous()
    return t1, t2


def _pair_topk_lists(pairs, known, dev):
    """(pair_u, pair_v int32 [P], keys, ptr, rel, n_keys) of the pair top-k entries, all on `dev`."""
    pairs = torch.as_tensor(pairs)
    require_device(pairs)
    if pairs.dim() != 2 or pairs.shape[0] != 2 or pairs.dtype.is_floating_point:
        raise _lib.TipkError('pairs: an int tensor [2, P] expected, got %s %s' % (pairs.dtype, tuple(pairs.shape)))
    pu, pv = pairs[0].to(torch.int32).contiguous(), pairs[1].to(torch.int32).contiguous()
    keys, kptr, krel, n_keys = _known_lists(known)
    return pu, pv, keys, kptr, krel, n_keys


def distmult_pair_topk(z, rel_w, pairs, k, known=None):
    """The k best relations of every pair by DistMult logit, known ones dropped (include/tipk.h section 4d).

    pairs: int tensor [2, P] on the device.  known: None or (pair_keys, pair_ptr, rel) on the device, the pair-major lists
    of `known_relations_by_pair`.  -> (logits float32 [P, k], relation int32 [P, k]), descending logit then ascending
    relation id; (-inf, -1) pads a row with fewer than k candidates.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_pair_topk')
    dev = z.device
    pu, pv, keys, kptr, krel, n_keys = _pair_topk_lists(pairs, known, dev)
    n, dim, n_rel, n_p, k = z.shape[0], z.shape[1], rel_w.shape[0], pu.numel(), int(k)
    out_s, out_r = _topk_outputs(n_p, k, 1, dev)
    ws_bytes = int(lib().tipk_distmult_pair_topk_workspace_bytes(n, dim, n_rel, n_p, k))
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    check(lib().tipk_distmult_pair_topk(ptr(z), n, dim, ptr(rel_w), n_rel, ptr(pu), ptr(pv), n_p, ptr(keys), ptr(kptr),
                                        ptr(krel), n_keys, k, ptr(out_s), ptr(out_r), ptr(ws), stream_ptr(dev)),
          'tipk_distmult_pair_topk')
    return out_s, out_r


def pair_table_pair_topk(s1, s2, pairs, k, known=None):
    """`distmult_pair_topk` for the NN decoder's node-major tables s1, s2 [n, n_rel] (row stride free, the same for both):
    the logit of (u, v, r) is s1[u, r] + s2[v, r] (not symmetric); `known` drops a relation in either pair direction."""
    s1, s2 = _table_pair(s1, s2, 'pair_table_pair_topk')
    dev = s1.device
    pu, pv, keys, kptr, krel, n_keys = _pair_topk_lists(pairs, known, dev)
    n, n_rel, n_p, k = s1.shape[0], s1.shape[1], pu.numel(), int(k)
    out_s, out_r = _topk_outputs(n_p, k, 1, dev)
    check(lib().tipk_pair_table_pair_topk(ptr(s1), ptr(s2), s1.stride(0), n, n_rel, ptr(pu), ptr(pv), n_p, ptr(keys),
                                          ptr(kptr), ptr(krel), n_keys, k, ptr(out_s), ptr(out_r), stream_ptr(dev)),
          'tipk_pair_table_pair_topk')
    return out_s, out_r


def restrict_known_relations(known, relations, n_rel):
    """The pair-major lists `known` (global relation ids in [0, n_rel)) cut down to the candidate ids `relations` (int64
    tensor on the lists' device, distinct) and renumbered to POSITIONS in `relations`: same keys, a pair's block keeps the
    candidates' entries only, ascending by position.  What the top-k entries need when they rank a subset of relations."""
    keys, kptr, krel = known
    dev = keys.device
    pos = torch.full((int(n_rel),), -1, dtype=torch.int64, device=dev)
    pos[relations] = torch.arange(relations.numel(), device=dev)
    owner = torch.repeat_interleave(torch.arange(keys.numel(), device=dev), kptr[1:] - kptr[:-1])
    new = pos[krel.long()]
    keep = new >= 0
    order = torch.sort(owner[keep] * max(1, relations.numel()) + new[keep]).indices
    kptr2 = torch.zeros_like(kptr)
    kptr2[1:] = torch.cumsum(torch.bincount(owner[keep], minlength=keys.numel()), 0)
    return keys, kptr2, new[keep][order].to(torch.int32)


def _triples(edge_index, edge_type):
    """(edge_index [2, T], edge_type [T]) as int tensors, checked."""
    edge_index, edge_type = torch.as_tensor(edge_index), torch.as_tensor(edge_type)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.dim() != 1 or edge_type.numel() != edge_index.shape[1] \
            or edge_index.dtype.is_floating_point or edge_type.dtype.is_floating_point:
        raise _lib.TipkError('triples: int tensors edge_index [2, T] and edge_type [T] expected, got %s %s and %s %s'
                             % (edge_index.dtype, tuple(edge_index.shape), edge_type.dtype, tuple(edge_type.shape)))
    return edge_index, edge_type


def _group_by_key(key):
    """int64 key [T] -> (keys [G] distinct ascending, ptr int64 [G + 1], order int64 [T]): group g is order[ptr[g]:ptr[g + 1]],
    the positions whose key is keys[g], in the caller's order (the sort is stable)."""
    order = torch.sort(key, stable=True).indices
    keys, counts = torch.unique_consecutive(key[order], return_counts=True)
    ptr = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=key.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return keys, ptr, order


def targets_by_pair(edge_index, edge_type, n_nodes):
    """Triples grouped by their ORDERED pair (u, v) -- the table decoder is not symmetric -- for the pair rank entries
    (include/tipk.h section 4f) -> (pairs int64 [2, P], tgt_ptr int64 [P + 1], tgt_rel int32 [T], order int64 [T]): pair p
    owns tgt_rel[tgt_ptr[p]:tgt_ptr[p + 1]], pairs ascend by u * n_nodes + v, a pair's targets keep the caller's order
    (repeats stay), and order[i] is the caller's position of grouped triple i: `out[order] = result` scatters a result
    back.  Torch ops on edge_index's device (CPU tensors work too)."""
    edge_index, edge_type = _triples(edge_index, edge_type)
    n = int(n_nodes)
    key = edge_index[0].to(torch.int64) * n + edge_index[1].to(torch.int64)
    keys, tgt_ptr, order = _group_by_key(key)
    pairs = torch.stack([torch.div(keys, n, rounding_mode='floor'), keys % n])
    return pairs, tgt_ptr, edge_type.to(key.device)[order].to(torch.int32).contiguous(), order


def _rank_targets(tgt_ptr, tgt, n_rows, dev):
    """(tgt_ptr int64 [n_rows + 1], tgt int32 [T], T, out_rank, out_logit) of the rank entries, all on `dev`: the target lists
    checked, the outputs filled with (0, NaN), which a target no row owns keeps."""
    tgt_ptr, tgt = torch.as_tensor(tgt_ptr), torch.as_tensor(tgt)
    require_device(tgt_ptr, tgt)
    if tgt_ptr.dim() != 1 or tgt.dim() != 1 or tgt_ptr.numel() != n_rows + 1 or tgt_ptr.dtype.is_floating_point \
            or tgt.dtype.is_floating_point:
        raise _lib.TipkError('targets: int tensors tgt_ptr [%d] and targets [T] expected, got %s %s and %s %s'
                             % (n_rows + 1, tgt_ptr.dtype, tuple(tgt_ptr.shape), tgt.dtype, tuple(tgt.shape)))
    tptr, tgt = tgt_ptr.to(torch.int64).contiguous(), tgt.to(torch.int32).contiguous()
    n_tgt = tgt.numel()
    out_rank = torch.zeros((n_tgt,), dtype=torch.int32, device=dev)
    out_logit = torch.full((n_tgt,), float('nan'), dtype=torch.float32, device=dev)
    return tptr, tgt, n_tgt, out_rank, out_logit


def _pair_rank_lists(pairs, tgt_ptr, tgt_rel, known, dev):
    """(pair_u, pair_v, tgt_ptr, tgt_rel, n_tgt, known lists, out_rank, out_logit) of the pair rank entries, all on `dev`."""
    pu, pv, keys, kptr, krel, n_keys = _pair_topk_lists(pairs, known, dev)
    tptr, trel, n_tgt, out_rank, out_logit = _rank_targets(tgt_ptr, tgt_rel, pu.numel(), dev)
    return pu, pv, tptr, trel, n_tgt, keys, kptr, krel, n_keys, out_rank, out_logit


def distmult_pair_rank(z, rel_w, pairs, tgt_ptr, tgt_rel, known=None):
    """The filtered rank of given relations among all relations of their pair by DistMult logit (include/tipk.h section 4f).

    pairs: int tensor [2, P]; tgt_ptr int [P + 1], tgt_rel int [T]: pair p owns the targets tgt_rel[tgt_ptr[p]:tgt_ptr[p+1]]
    (`targets_by_pair`); known: None or the pair-major lists of `known_relations_by_pair`; all on the device.
    -> (rank int32 [T], logit float32 [T]): rank = 1 + the number of relations, not listed for the pair, that beat the
    target (higher logit, or equal logit and lower id); rank - 1 is the target's position in `distmult_pair_topk` under the
    same filter.  (0, NaN): not ranked -- a NaN logit, a target outside [0, n_rel), a pair index outside [0, n).
    Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_pair_rank')
    dev = z.device
    pu, pv, tptr, trel, n_tgt, keys, kptr, krel, n_keys, out_rank, out_logit = _pair_rank_lists(pairs, tgt_ptr, tgt_rel,
                                                                                               known, dev)
    check(lib().tipk_distmult_pair_rank(ptr(z), z.shape[0], z.shape[1], ptr(rel_w), rel_w.shape[0], ptr(pu), ptr(pv),
                                        pu.numel(), ptr(tptr), ptr(trel), n_tgt, ptr(keys), ptr(kptr), ptr(krel), n_keys,
                                        ptr(out_rank), ptr(out_logit), stream_ptr(dev)), 'tipk_distmult_pair_rank')
    return out_rank, out_logit


def pair_table_pair_rank(s1, s2, pairs, tgt_ptr, tgt_rel, known=None):
    """`distmult_pair_rank` for the NN decoder's node-major tables s1, s2 [n, n_rel] (row stride free, the same for both):
    the logit of (u, v, r) is s1[u, r] + s2[v, r] (not symmetric); `known` drops a relation in either pair direction."""
    s1, s2 = _table_pair(s1, s2, 'pair_table_pair_rank')
    dev = s1.device
    pu, pv, tptr, trel, n_tgt, keys, kptr, krel, n_keys, out_rank, out_logit = _pair_rank_lists(pairs, tgt_ptr, tgt_rel,
                                                                                               known, dev)
    check(lib().tipk_pair_table_pair_rank(ptr(s1), ptr(s2), s1.stride(0), s1.shape[0], s1.shape[1], ptr(pu), ptr(pv),
                                          pu.numel(), ptr(tptr), ptr(trel), n_tgt, ptr(keys), ptr(kptr), ptr(krel), n_keys,
                                          ptr(out_rank), ptr(out_logit), stream_ptr(dev)), 'tipk_pair_table_pair_rank')
    return out_rank, out_logit


def targets_by_query(edge_index, edge_type, n_nodes):
    """Triples (u, v, r) grouped by the (relation, drug) query (r, u) that ranks v -- for the partner rank entries
    (include/tipk.h section 4g) -> (q_rel int32 [Q], q_drug int32 [Q], tgt_ptr int64 [Q + 1], tgt_node int32 [T], order
    int64 [T]): query q owns tgt_node[tgt_ptr[q]:tgt_ptr[q + 1]], the queries ascend by r * n_nodes + u, a query's targets
    keep the caller's order (repeats stay), and order[i] is the caller's position of grouped triple i:
    `out[order] = result` scatters a result back.  Torch ops on edge_index's device (CPU tensors work too)."""
    edge_index, edge_type = _triples(edge_index, edge_type)
    n = int(n_nodes)
    key = edge_type.to(device=edge_index.device, dtype=torch.int64) * n + edge_index[0].to(torch.int64)
    keys, tgt_ptr, order = _group_by_key(key)
    q_rel = torch.div(keys, n, rounding_mode='floor').to(torch.int32)
    return q_rel, (keys % n).to(torch.int32), tgt_ptr, edge_index[1][order].to(torch.int32).contiguous(), order


def _partner_rank_lists(q_rel, q_drug, tgt_ptr, tgt_node, known, dev):
    """(q_rel, q_drug, tgt_ptr, tgt_node, n_tgt, keys, ptr, out_rank, out_logit) of the partner rank entries, all on `dev`."""
    q_rel, q_drug = torch.as_tensor(q_rel), torch.as_tensor(q_drug)
    require_device(q_rel, q_drug)
    if any(t.dim() != 1 or t.dtype.is_floating_point for t in (q_rel, q_drug)) or q_drug.numel() != q_rel.numel():
        raise _lib.TipkError('queries: int tensors q_rel [Q] and q_drug [Q] expected, got %s %s and %s %s'
                             % (q_rel.dtype, tuple(q_rel.shape), q_drug.dtype, tuple(q_drug.shape)))
    tptr, tnode, n_tgt, out_rank, out_logit = _rank_targets(tgt_ptr, tgt_node, q_rel.numel(), dev)
    keys, kptr = _relation_known(known)
    qr, qd = q_rel.to(torch.int32).contiguous(), q_drug.to(torch.int32).contiguous()
    return qr, qd, tptr, tnode, n_tgt, keys, kptr, out_rank, out_logit


def distmult_partner_rank(z, rel_w, q_rel, q_drug, tgt_ptr, tgt_node, known=None):
    """The filtered rank of given partners among all drugs, per (relation, drug) query, by DistMult logit (include/tipk.h
    section 4g).

    q_rel, q_drug: int tensors [Q]; tgt_ptr int [Q + 1], tgt_node int [T]: query q = (r, u) owns the target partners
    tgt_node[tgt_ptr[q]:tgt_ptr[q+1]] (`targets_by_query`); known: None or (keys int64 u*n+v sorted inside each relation, ptr
    int64 [n_rel + 1]), the relation-major lists `distmult_screen` takes; all on the device.
    -> (rank int32 [T], logit float32 [T]): rank = 1 + the number of drugs c != u, with neither u*n+c nor c*n+u listed for
    r, that beat the target (higher logit, or equal logit and lower id); rank - 1 is the target's position in the drug query
    (r, u) of `distmult_screen` under the same filter.  The logit multiplies z[u] with rel_w[r] first: it is the screen's,
    not symmetric in (u, target) to the last bit.  (0, NaN): not ranked -- r outside [0, n_rel), u or the target outside
    [0, n), target == u, a NaN logit.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_partner_rank')
    dev = z.device
    qr, qd, tptr, tnode, n_tgt, keys, kptr, out_rank, out_logit = _partner_rank_lists(q_rel, q_drug, tgt_ptr, tgt_node, known,
                                                                                      dev)
    check(lib().tipk_distmult_partner_rank(ptr(z), z.shape[0], z.shape[1], ptr(rel_w), rel_w.shape[0], ptr(qr), ptr(qd),
                                           qr.numel(), ptr(tptr), ptr(tnode), n_tgt, ptr(keys), ptr(kptr), ptr(out_rank),
                                           ptr(out_logit), stream_ptr(dev)), 'tipk_distmult_partner_rank')
    return out_rank, out_logit


def pair_table_partner_rank(s1t, s2t, q_rel, q_drug, tgt_ptr, tgt_node, known=None):
    """`distmult_partner_rank` for the NN decoder's RELATION-major tables s1t, s2t [n_rel, n] (row stride free, the same for
    both), as `NNDecoder.objective` forms them: the logit of target c of query (r, u) is s1t[r, u] + s2t[r, c]."""
    s1t, s2t = _table_pair(s1t, s2t, 'pair_table_partner_rank', '[n_rel, n]')
    dev = s1t.device
    qr, qd, tptr, tnode, n_tgt, keys, kptr, out_rank, out_logit = _partner_rank_lists(q_rel, q_drug, tgt_ptr, tgt_node, known,
                                                                                      dev)
    check(lib().tipk_pair_table_partner_rank(ptr(s1t), ptr(s2t), s1t.stride(0), s1t.shape[1], s1t.shape[0], ptr(qr), ptr(qd),
                                             qr.numel(), ptr(tptr), ptr(tnode), n_tgt, ptr(keys), ptr(kptr), ptr(out_rank),
                                             ptr(out_logit), stream_ptr(dev)), 'tipk_pair_table_partner_rank')
    return out_rank, out_logit


_SYMMETRIC_KNOWN = DerivedCache(8)


def symmetric_known(known, n_nodes):
    """Relation-major known lists (keys int64 u*n+v sorted inside each relation, ptr int64 [n_rel + 1]) that hold BOTH
    directions of every pair: each key is mirrored to v*n+u, the keys are sorted inside each relation and duplicates dropped
    (a self key u*n+u is its own mirror).  Lists that are already symmetric come back UNCHANGED (the same tuple); None stays
    None.  Torch ops on the lists' device (CPU tensors work too); cached per list tensors (`_cache.DerivedCache`)."""
    if known is None:
        return None
    keys, kptr = known
    n = int(n_nodes)

    def build():                                                        # None: already symmetric
        k64, p64 = keys.to(torch.int64), kptr.to(torch.int64)
        n_rel = p64.numel() - 1
        rel = torch.repeat_interleave(torch.arange(n_rel, device=keys.device), p64[1:] - p64[:-1])
        comb = rel * (n * n) + k64
        mirror = rel * (n * n) + (k64 % n) * n + torch.div(k64, n, rounding_mode='floor')
        both = torch.unique(torch.cat([comb, mirror]))                  # sorted by (relation, key), duplicates gone
        if both.numel() == comb.numel() and torch.equal(both, comb):
            return None
        ptr = torch.zeros(n_rel + 1, dtype=torch.int64, device=keys.device)
        ptr[1:] = torch.cumsum(torch.bincount(torch.div(both, n * n, rounding_mode='floor'), minlength=n_rel), 0)
        return (both % (n * n)).contiguous(), ptr

    both = _SYMMETRIC_KNOWN.get((keys, kptr), n, build)
    return known if both is None else both


def _partner_sum_lists(q_drug, k, rel_ids, partner_w, known, n, n_rel, dev):
    """(q_drug int32 [Q], rel_ids int32 [S] or None, n_sel, partner_w or None, keys, ptr, k, outputs) of the partner sum
    entries, all on `dev`; the known lists are made symmetric (`symmetric_known`)."""
    q_drug = torch.as_tensor(q_drug)
    rel_ids = None if rel_ids is None else torch.as_tensor(rel_ids)
    require_device(q_drug, rel_ids, partner_w)
    ints = (q_drug,) + (() if rel_ids is None else (rel_ids,))
    if any(t.dim() != 1 or t.dtype.is_floating_point for t in ints):
        raise _lib.TipkError('partner sum: 1-d int tensors q_drug [Q] and rel_ids [S] (or None) expected, got %s'
                             % ', '.join('%s %s' % (t.dtype, tuple(t.shape)) for t in ints))
    if partner_w is not None:
        partner_w = _f32c(partner_w).contiguous()
        if partner_w.dim() != 1 or partner_w.numel() != n:
            raise _lib.TipkError('partner_w: a float tensor [%d] expected, got %s' % (n, tuple(partner_w.shape)))
    keys, kptr = _relation_known(symmetric_known(known, n))
    qd = q_drug.to(torch.int32).contiguous()
    rel = None if rel_ids is None else rel_ids.to(torch.int32).contiguous()
    n_q, n_sel, k = qd.numel(), (n_rel if rel is None else rel.numel()), int(k)
    out_sum = torch.empty((n_q, n_sel), dtype=torch.float32, device=dev)
    out_cnt = torch.empty((n_q, n_sel), dtype=torch.int32, device=dev)
    if n_sel == 0 and k > 0:                                             # (no launch without columns: the rows are padding)
        top_v = torch.full((n_q, k), float('-inf'), dtype=torch.float32, device=dev)
        top_p = torch.full((n_q, k), -1, dtype=torch.int32, device=dev)
    else:
        top_v, top_p = _topk_outputs(n_q, k, 1, dev)
    return qd, rel, n_sel, partner_w, keys, kptr, k, out_sum, out_cnt, top_v, top_p


def distmult_partner_sum(z, rel_w, q_drug, k, rel_ids=None, partner_w=None, known=None):
    """The expected number of unrecorded partners of every queried drug per relation by DistMult logit, and the k relations of
    each drug with the largest expectation (include/tipk.h section 4l).

    q_drug int [Q] (entries may repeat); rel_ids None (all relations) or int [S]: the relations that are the columns of the
    result (entries may repeat); partner_w None (all 1) or float [n], finite and >= 0; known: None or (keys int64 u*n+v sorted
    inside each relation, ptr int64 [n_rel + 1]), the relation-major lists `distmult_screen` takes -- made symmetric here
    (`symmetric_known`), so a recorded pair is dropped in both directions.  All on the device.
    -> (sum float32 [Q, S], count int32 [Q, S], top_val float32 [Q, k], top_pos int32 [Q, k]): sum = the sum over the
    candidates c (c != u, partner_w[c] != 0, (u, c) not recorded for the relation) of partner_w[c] * sigma(logit), count =
    their number; (NaN, 0) for a drug outside [0, n) or a relation outside [0, n_rel); NaN where a candidate's logit is NaN.
    top_*: the k largest non-NaN cells of each row, descending, ties by column position, padded with (-inf, -1); empty for
    k = 0.  Does not synchronise (the first call on new known lists does, once, to mirror them)."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_partner_sum')
    dev = z.device
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]
    qd, rel, n_sel, pw, keys, kptr, k, out_sum, out_cnt, top_v, top_p = _partner_sum_lists(q_drug, k, rel_ids, partner_w,
                                                                                           known, n, n_rel, dev)
    check(lib().tipk_distmult_partner_sum(ptr(z), n, dim, ptr(rel_w), n_rel, ptr(qd), qd.numel(), ptr(rel), n_sel, ptr(pw),
                                          ptr(keys), ptr(kptr), k, ptr(out_sum), ptr(out_cnt), ptr(top_v), ptr(top_p),
                                          stream_ptr(dev)), 'tipk_distmult_partner_sum')
    return out_sum, out_cnt, top_v, top_p


def pair_table_partner_sum(s1t, s2t, q_drug, k, rel_ids=None, partner_w=None, known=None):
    """`distmult_partner_sum` for the NN decoder's RELATION-major tables s1t, s2t [n_rel, n] (row stride free, the same for
    both), as `NNDecoder.objective` forms them: the logit of partner c of drug u under r is s1t[r, u] + s2t[r, c]."""
    s1t, s2t = _table_pair(s1t, s2t, 'pair_table_partner_sum', '[n_rel, n]')
    dev = s1t.device
    n, n_rel = s1t.shape[1], s1t.shape[0]
    qd, rel, n_sel, pw, keys, kptr, k, out_sum, out_cnt, top_v, top_p = _partner_sum_lists(q_drug, k, rel_ids, partner_w,
                                                                                           known, n, n_rel, dev)
    check(lib().tipk_pair_table_partner_sum(ptr(s1t), ptr(s2t), s1t.stride(0), n, n_rel, ptr(qd), qd.numel(), ptr(rel), n_sel,
                                            ptr(pw), ptr(keys), ptr(kptr), k, ptr(out_sum), ptr(out_cnt), ptr(top_v),
                                            ptr(top_p), stream_ptr(dev)), 'tipk_pair_table_partner_sum')
    return out_sum, out_cnt, top_v, top_p


# what `fit_pairs_csr` returns: the distinct recorded pairs of B new side effects and their weights (include/tipk.h 4m)
FitPairs = collections.namedtuple('FitPairs', ['ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w', 'n_pairs', 'known'])


def _ragged_lists(arg, what, item_names, tensor_form):
    """A ragged argument of the fits' list builders -- a list of lists of 2-tuples, or (index int [2, P], ptr int [rows + 1])
    -- as (index int64 [2, P], ptr int64 [rows + 1]) on the host.  ValueError names the argument `what`, the tuple's items
    and the tensor form."""
    if isinstance(arg, tuple) and len(arg) == 2 and torch.is_tensor(arg[0]):
        idx, lptr = torch.as_tensor(arg[0]).to('cpu'), torch.as_tensor(arg[1]).to('cpu')
        if idx.dtype.is_floating_point or lptr.dtype.is_floating_point or idx.dim() != 2 or idx.shape[0] != 2 or lptr.dim() != 1 \
                or lptr.numel() < 1:
            raise ValueError('%s: %s expected' % (what, tensor_form))
        idx, lptr = idx.to(torch.int64), lptr.to(torch.int64)
        if int(lptr[0]) != 0 or int(lptr[-1]) != idx.shape[1] or bool((lptr[1:] < lptr[:-1]).any()):
            raise ValueError('%s: ptr must rise from 0 to P = %d' % (what, idx.shape[1]))
        return idx, lptr
    try:
        rows = [[(int(a), int(b)) for a, b in lst] for lst in arg]
    except (TypeError, ValueError):
        raise ValueError('%s: a list of lists of %s expected' % (what, item_names)) from None
    lptr = torch.zeros(len(rows) + 1, dtype=torch.int64)
    if rows:
        lptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows], dtype=torch.int64), 0)
    flat = [p for r in rows for p in r]
    idx = torch.tensor(flat, dtype=torch.int64).reshape(-1, 2).t() if flat else torch.zeros((2, 0), dtype=torch.int64)
    return idx, lptr


def fit_pairs_csr(pairs, n_nodes, neg_weight=1.0):
    """The recorded pairs of B new side effects in the form the fit entries read (host function, CPU tensors).

    pairs: a list of B lists of (u, v), or (edge_index int [2, P], ptr int [B + 1]): relation b owns the columns
    ptr[b]:ptr[b + 1].  A pair is unordered -- (u, v), (v, u) and repeats are ONE distinct pair whose multiplicity is the number
    of times it is listed; self pairs are allowed.
    -> FitPairs(ptr int64 [B + 1], u, v int32 [D] with u <= v, sorted by (u, v) inside a relation, wpos fp32 [D] =
    multiplicity / P_b, wneg fp32 [D] = neg_weight * ordered multiplicity (2, or 1 for u == v) / N_b, dense_w fp32 [B] =
    neg_weight / N_b, n_pairs int64 [B] = P_b (duplicates count), known = (keys int64 u * n + v, ptr int64 [B + 1]): both
    directions of every distinct pair, sorted inside each relation -- the lists `distmult_screen` and `distmult_partner_sum`
    take).  N_b = n^2 minus the ordered recorded pairs; N_b == 0 gives dense_w = wneg = 0.
    ValueError for an id outside [0, n_nodes) or a malformed list."""
    n = int(n_nodes)
    if n < 1:
        raise ValueError('n_nodes must be >= 1, not %d' % n)
    if not float(neg_weight) > 0:
        raise ValueError('neg_weight must be > 0, not %r' % (neg_weight,))
    idx, lptr = _ragged_lists(pairs, 'pairs', '(u, v)', '(edge_index int [2, P], ptr int [B + 1])')
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError('drug id out of range: [%d, %d] for %d drugs' % (int(idx.min()), int(idx.max()), n))
    b = lptr.numel() - 1
    n_pairs = lptr[1:] - lptr[:-1]
    rel = torch.repeat_interleave(torch.arange(b, dtype=torch.int64), n_pairs)
    lo, hi = torch.minimum(idx[0], idx[1]), torch.maximum(idx[0], idx[1])
    key, count = torch.unique(rel * (n * n) + lo * n + hi, return_counts=True)         # sorted by (relation, u, v)
    drel, dkey = torch.div(key, n * n, rounding_mode='floor'), key % (n * n)
    du, dv = torch.div(dkey, n, rounding_mode='floor'), dkey % n
    ordered = torch.where(du == dv, 1, 2).to(torch.float64)
    recorded = torch.zeros(b, dtype=torch.float64).index_add_(0, drel, ordered)
    n_neg = float(n) * n - recorded
    dense = torch.where(n_neg > 0, float(neg_weight) / n_neg.clamp(min=1.0), torch.zeros_like(n_neg))
    dptr = torch.zeros(b + 1, dtype=torch.int64)
    dptr[1:] = torch.cumsum(torch.bincount(drel, minlength=b), 0)
    wpos = count.to(torch.float64) / n_pairs.to(torch.float64)[drel]
    both = torch.unique(torch.cat([key, drel * (n * n) + dv * n + du]))
    kptr = torch.zeros(b + 1, dtype=torch.int64)
    kptr[1:] = torch.cumsum(torch.bincount(torch.div(both, n * n, rounding_mode='floor'), minlength=b), 0)
    return FitPairs(dptr, du.to(torch.int32), dv.to(torch.int32), wpos.to(torch.float32),
                    (dense[drel] * ordered).to(torch.float32), dense.to(torch.float32), n_pairs,
                    ((both % (n * n)).contiguous(), kptr))


def _lists_on(dev, nt, term_ints, row_ints, who, what):
    """The lists of a fit's named tuple `nt` on dev as the entries read them -> ((ptr int64, the per-term lists: `term_ints`
    int32, wpos, wneg fp32, the per-row lists: dense_w fp32, `row_ints` int32), number of rows)."""
    terms = [getattr(nt, f).to(dev, torch.int32) for f in term_ints] + [nt.wpos.to(dev, torch.float32),
                                                                        nt.wneg.to(dev, torch.float32)]
    rows = [nt.dense_w.to(dev, torch.float32)] + [getattr(nt, f).to(dev, torch.int32) for f in row_ints]
    lptr = nt.ptr.to(dev, torch.int64)
    n_rows = lptr.numel() - 1
    if any(t.numel() != n_rows for t in rows) or any(t.numel() != terms[0].numel() for t in terms[1:]):
        raise _lib.TipkError('%s: the %s lists do not belong together' % (who, what))
    return tuple(t.contiguous() for t in [lptr] + terms + rows), n_rows


def _fit_workspace(nbytes, dev, who, shape_text, section):
    """The workspace of a fit entry from its *_workspace_bytes answer; a negative answer is an unsupported shape."""
    if nbytes < 0:
        raise _lib.TipkError('%s: unsupported shape %s (include/tipk.h section %s)' % (who, shape_text, section))
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _trial_active_out(x, active, out, n_rows, width, dev, who, name):
    """What a *_stats wrapper takes besides the lists: the trial rows `name` [n_rows, width], the active mask and the
    (loss, grad, hess) triple, made where `out` is None."""
    x = _f32c(x).contiguous()
    require_device(x, active)
    if tuple(x.shape) != (n_rows, width):
        raise _lib.TipkError('%s: %s [%d, %d] expected, got %s' % (who, name, n_rows, width, tuple(x.shape)))
    if active is not None:
        active = active.to(torch.int32).contiguous()
        if tuple(active.shape) != (n_rows,):
            raise _lib.TipkError('%s: active [%d] expected, got %s' % (who, n_rows, tuple(active.shape)))
    if out is None:
        out = (torch.empty(n_rows, dtype=torch.float32, device=dev),
               torch.empty((n_rows, width), dtype=torch.float32, device=dev),
               torch.empty((n_rows, width, width), dtype=torch.float32, device=dev))
    return x, active, out


def _newton_outputs(init, n_rows, width, max_iter, gtol, dev, who):
    """What a fit wrapper takes besides the lists: max_iter and gtol checked, init [n_rows, width] or None as the entry reads
    it, and the outputs -> (init, x [n_rows, width], loss [n_rows], grad [n_rows, width], info int32 [n_rows, 4])."""
    if int(max_iter) < 0 or not float(gtol) >= 0:
        raise _lib.TipkError('%s: max_iter >= 0 and gtol >= 0 expected, got %r and %r' % (who, max_iter, gtol))
    if init is not None:
        init = _f32c(init).contiguous()
        require_device(init)
        if tuple(init.shape) != (n_rows, width):
            raise _lib.TipkError('%s: init [%d, %d] expected, got %s' % (who, n_rows, width, tuple(init.shape)))
    return (init, torch.empty((n_rows, width), dtype=torch.float32, device=dev),
            torch.empty(n_rows, dtype=torch.float32, device=dev),
            torch.empty((n_rows, width), dtype=torch.float32, device=dev),
            torch.zeros((n_rows, 4), dtype=torch.int32, device=dev))


def _fit_operands(z, fp, l2, who):
    """z as the fit entries read it and the lists of `fp` (a `FitPairs`) on its device."""
    z = _f32c(z).contiguous()
    require_device(z)
    if z.dim() != 2:
        raise _lib.TipkError('%s: z [n, dim] expected, got %s' % (who, tuple(z.shape)))
    if not float(l2) >= 0:
        raise _lib.TipkError('%s: l2 must be >= 0, not %r' % (who, l2))
    lists, n_fit = _lists_on(z.device, fp, ('u', 'v'), (), who, 'pair')
    ws = _fit_workspace(lib().tipk_distmult_fit_workspace_bytes(z.shape[0], z.shape[1], n_fit), z.device, who,
                        'n = %d, dim = %d, n_fit = %d' % (z.shape[0], z.shape[1], n_fit), '4m')
    return z, lists, n_fit, ws


def distmult_fit_supported(n_nodes, dim, n_fit=1):
    return bool(lib().tipk_distmult_fit_supported(n_nodes, dim, n_fit))


def distmult_fit_stats(z, w, fp, l2=1e-4, active=None, out=None):
    """Loss, gradient and Hessian of the new side effects' objective at the trial rows w [B, dim] (include/tipk.h section 4m).
    fp: the `FitPairs` of `fit_pairs_csr` (moved to z's device); active: None or int [B], 0 = leave that relation's rows of
    `out` untouched; out: None or (loss [B], grad [B, dim], hess [B, dim, dim]) to write into.
    -> (loss, grad, hess), fp32, the l2 terms included.  Does not synchronise."""
    z, (pptr, pu, pv, wpos, wneg, dense), n_fit, ws = _fit_operands(z, fp, l2, 'distmult_fit_stats')
    dim = z.shape[1]
    w, active, (loss, grad, hess) = _trial_active_out(w, active, out, n_fit, dim, z.device, 'distmult_fit_stats', 'w')
    check(lib().tipk_distmult_fit_stats(ptr(z), z.shape[0], dim, ptr(w), n_fit, ptr(dense), ptr(pptr), ptr(pu), ptr(pv),
                                        ptr(wpos), ptr(wneg), pu.numel(), float(l2), ptr(active), ptr(loss), ptr(grad),
                                        ptr(hess), ptr(ws), stream_ptr(z.device)), 'tipk_distmult_fit_stats')
    return loss, grad, hess


def distmult_fit(z, fp, l2=1e-4, init=None, max_iter=16, gtol=1e-5):
    """Fit the DistMult rows of B new side effects on the frozen z by damped Newton steps: max_iter + 1 (statistics, step)
    launches enqueued by ONE `tipk_distmult_fit` call (include/tipk.h section 4m).  init: None (zeros) or [B, dim].
    -> (w [B, dim], loss [B], grad [B, dim], info int32 [B, 4] = (status, evaluations, accepted, rejected)); status 1
    converged (max |grad| <= gtol), 2 step below 2^-20, 3 non-finite statistic, 0 still running after max_iter + 1
    evaluations.  Does not synchronise."""
    z, (pptr, pu, pv, wpos, wneg, dense), n_fit, ws = _fit_operands(z, fp, l2, 'distmult_fit')
    dim, dev = z.shape[1], z.device
    init, w, loss, grad, info = _newton_outputs(init, n_fit, dim, max_iter, gtol, dev, 'distmult_fit')
    check(lib().tipk_distmult_fit(ptr(z), z.shape[0], dim, n_fit, ptr(dense), ptr(pptr), ptr(pu), ptr(pv), ptr(wpos), ptr(wneg),
                                  pu.numel(), float(l2), ptr(init), int(max_iter), float(gtol), ptr(w), ptr(loss), ptr(grad),
                                  ptr(info), ptr(ws), stream_ptr(dev)), 'tipk_distmult_fit')
    return w, loss, grad, info


# what `drug_fit_csr` returns: the distinct recorded cells of M new drugs and their weights (include/tipk.h 4q)
DrugFitLists = collections.namedtuple('DrugFitLists', ['ptr', 'v', 'r', 'wpos', 'wneg', 'dense_w', 'n_interactions', 'known'])


def drug_fit_csr(interactions, n_nodes, n_rel, neg_weight=1.0):
    """The recorded interactions of M new drugs in the form the drug-fit entries read (host function, CPU tensors).

    interactions: a list of M lists of (partner, side effect), or (index int [2, P], ptr int [M + 1]): row 0 the partners, row 1
    the side effects, drug a owns the columns ptr[a]:ptr[a + 1].  A repeat is ONE distinct cell whose multiplicity is the
    number of times it is listed.
    -> DrugFitLists(ptr int64 [M + 1], v, r int32 [D], sorted by (v, r) inside a drug, wpos fp32 [D] = multiplicity / P_a,
    wneg fp32 [D] = dense_w of the cell's drug, dense_w fp32 [M] = neg_weight / N_a, n_interactions int64 [M] = P_a (duplicates
    count), known = (keys int64 v * n_rel + r, ptr int64 [M + 1]): the distinct cells, sorted inside each drug).
    N_a = n_nodes * n_rel minus the distinct recorded cells; N_a == 0 gives dense_w = wneg = 0.
    ValueError for an id outside [0, n_nodes) x [0, n_rel) or a malformed list."""
    n, nr = int(n_nodes), int(n_rel)
    if n < 1 or nr < 1:
        raise ValueError('n_nodes and n_rel must be >= 1, not %d and %d' % (n, nr))
    if not float(neg_weight) > 0:
        raise ValueError('neg_weight must be > 0, not %r' % (neg_weight,))
    idx, lptr = _ragged_lists(interactions, 'interactions', '(partner, side effect)', '(index int [2, P], ptr int [M + 1])')
    if idx.numel() and (int(idx[0].min()) < 0 or int(idx[0].max()) >= n):
        raise ValueError('partner id out of range: [%d, %d] for %d drugs' % (int(idx[0].min()), int(idx[0].max()), n))
    if idx.numel() and (int(idx[1].min()) < 0 or int(idx[1].max()) >= nr):
        raise ValueError('side-effect id out of range: [%d, %d] for %d side effects' % (int(idx[1].min()), int(idx[1].max()), nr))
    m = lptr.numel() - 1
    cells = n * nr
    n_inter = lptr[1:] - lptr[:-1]
    drug = torch.repeat_interleave(torch.arange(m, dtype=torch.int64), n_inter)
    key, count = torch.unique(drug * cells + idx[0] * nr + idx[1], return_counts=True)     # sorted by (drug, v, r)
    ddrug, dkey = torch.div(key, cells, rounding_mode='floor'), key % cells
    dptr = torch.zeros(m + 1, dtype=torch.int64)
    dptr[1:] = torch.cumsum(torch.bincount(ddrug, minlength=m), 0)
    n_neg = (float(cells) - (dptr[1:] - dptr[:-1]).to(torch.float64))
    dense = torch.where(n_neg > 0, float(neg_weight) / n_neg.clamp(min=1.0), torch.zeros_like(n_neg))
    wpos = count.to(torch.float64) / n_inter.to(torch.float64)[ddrug]
    return DrugFitLists(dptr, torch.div(dkey, nr, rounding_mode='floor').to(torch.int32), (dkey % nr).to(torch.int32),
                        wpos.to(torch.float32), dense[ddrug].to(torch.float32), dense.to(torch.float32), n_inter,
                        (dkey.contiguous(), dptr.clone()))


def _drug_fit_operands(z, rel_w, fl, prior, l2, who):
    """z and rel_w as the drug-fit entries read them, the lists of `fl` (a `DrugFitLists`) and the prior on their device."""
    z, rel_w = _f32c(z).contiguous(), _f32c(rel_w).contiguous()
    require_device(z, rel_w, prior)
    if z.dim() != 2 or rel_w.dim() != 2 or z.shape[1] != rel_w.shape[1]:
        raise _lib.TipkError('%s: z [n, dim] and rel_w [n_rel, dim] expected, got %s and %s'
                             % (who, tuple(z.shape), tuple(rel_w.shape)))
    if not float(l2) >= 0:
        raise _lib.TipkError('%s: l2 must be >= 0, not %r' % (who, l2))
    lists, n_fit = _lists_on(z.device, fl, ('v', 'r'), (), who, 'interaction')
    if prior is not None:
        prior = _f32c(prior).contiguous()
        if tuple(prior.shape) != (n_fit, z.shape[1]):
            raise _lib.TipkError('%s: prior [%d, %d] expected, got %s' % (who, n_fit, z.shape[1], tuple(prior.shape)))
    ws = _fit_workspace(lib().tipk_distmult_drug_fit_workspace_bytes(z.shape[0], z.shape[1], rel_w.shape[0], n_fit), z.device,
                        who, 'n = %d, n_rel = %d, dim = %d, n_fit = %d' % (z.shape[0], rel_w.shape[0], z.shape[1], n_fit), '4q')
    return z, rel_w, lists, prior, n_fit, ws


def distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit=1):
    return bool(lib().tipk_distmult_drug_fit_supported(n_nodes, dim, n_rel, n_fit))


def distmult_drug_fit_stats(z, rel_w, x, fl, prior=None, l2=1e-4, active=None, out=None):
    """Loss, gradient and Hessian of the new drugs' objective at the trial rows x [M, dim] (include/tipk.h section 4q).
    fl: the `DrugFitLists` of `drug_fit_csr` (moved to z's device); prior: None (zeros) or the centres [M, dim] of the l2 term;
    active: None or int [M], 0 = leave that drug's rows of `out` untouched; out: None or (loss [M], grad [M, dim], hess
    [M, dim, dim]) to write into.
    -> (loss, grad, hess), fp32, the l2 terms included.  Does not synchronise."""
    z, rel_w, (rptr, rv, rr, wpos, wneg, dense), prior, n_fit, ws = _drug_fit_operands(z, rel_w, fl, prior, l2,
                                                                                         'distmult_drug_fit_stats')
    dim = z.shape[1]
    x, active, (loss, grad, hess) = _trial_active_out(x, active, out, n_fit, dim, z.device, 'distmult_drug_fit_stats', 'x')
    check(lib().tipk_distmult_drug_fit_stats(ptr(z), z.shape[0], dim, ptr(rel_w), rel_w.shape[0], ptr(x), n_fit, ptr(dense),
                                             ptr(rptr), ptr(rv), ptr(rr), ptr(wpos), ptr(wneg), rv.numel(), ptr(prior),
                                             float(l2), ptr(active), ptr(loss), ptr(grad), ptr(hess), ptr(ws),
                                             stream_ptr(z.device)), 'tipk_distmult_drug_fit_stats')
    return loss, grad, hess


def distmult_drug_fit(z, rel_w, fl, prior=None, l2=1e-4, init=None, max_iter=16, gtol=1e-5):
    """Fit the embedding rows of M new drugs on the frozen z and rel_w by damped Newton steps: max_iter + 1 (statistics, step)
    launches enqueued by ONE `tipk_distmult_drug_fit` call (include/tipk.h section 4q).  prior: None (zeros) or the centres
    [M, dim] of the l2 term; init: None (the prior) or the start [M, dim].
    -> (x [M, dim], loss [M], grad [M, dim], info int32 [M, 4] = (status, evaluations, accepted, rejected), hess [M, dim, dim]:
    the Hessian at x); status 1 converged (max |grad| <= gtol), 2 step below 2^-20, 3 non-finite statistic, 0 still running after
    max_iter + 1 evaluations.  Does not synchronise."""
    z, rel_w, (rptr, rv, rr, wpos, wneg, dense), prior, n_fit, ws = _drug_fit_operands(z, rel_w, fl, prior, l2,
                                                                                         'distmult_drug_fit')
    dim, dev = z.shape[1], z.device
    init, x, loss, grad, info = _newton_outputs(init, n_fit, dim, max_iter, gtol, dev, 'distmult_drug_fit')
    h = torch.empty((n_fit, dim, dim), dtype=torch.float32, device=dev)
    check(lib().tipk_distmult_drug_fit(ptr(z), z.shape[0], dim, ptr(rel_w), rel_w.shape[0], n_fit, ptr(dense), ptr(rptr), ptr(rv),
                                       ptr(rr), ptr(wpos), ptr(wneg), rv.numel(), ptr(prior), float(l2), ptr(init),
                                       int(max_iter), float(gtol), ptr(x), ptr(loss), ptr(grad), ptr(info), ptr(h), ptr(ws),
                                       stream_ptr(dev)), 'tipk_distmult_drug_fit')
    return x, loss, grad, info, h


# what `calibration_lists` returns: per query the merged, sorted list of its distinct TRAIN and POS cells and their weights
# (include/tipk.h 4r)
CalibrationLists = collections.namedtuple('CalibrationLists', ['ptr', 'u', 'v', 'wpos', 'wneg', 'dense_w', 'q_rel', 'n_pos',
                                                               'n_neg', 'n_dropped'])


def _distinct_cells(edge_index, edge_type, n, n_rel, what):
    """The distinct (relation, unordered pair u < v) of the triples, self pairs dropped, as sorted int64 keys
    relation * n^2 + u * n + v (host)."""
    idx, et = torch.as_tensor(edge_index).to('cpu'), torch.as_tensor(edge_type).to('cpu')
    if idx.dim() != 2 or idx.shape[0] != 2 or et.dim() != 1 or et.numel() != idx.shape[1] or idx.dtype.is_floating_point \
            or et.dtype.is_floating_point:
        raise ValueError('%s: int tensors (edge_index [2, T], edge_type [T]) expected' % what)
    idx, et = idx.to(torch.int64), et.to(torch.int64)
    if et.numel():
        if int(idx.min()) < 0 or int(idx.max()) >= n:
            raise ValueError('%s: drug id out of range: [%d, %d] for %d drugs' % (what, int(idx.min()), int(idx.max()), n))
        if int(et.min()) < 0 or int(et.max()) >= n_rel:
            raise ValueError('%s: side-effect id out of range: [%d, %d] for %d side effects'
                             % (what, int(et.min()), int(et.max()), n_rel))
    lo, hi = torch.minimum(idx[0], idx[1]), torch.maximum(idx[0], idx[1])
    return torch.unique((et * (n * n) + lo * n + hi)[lo != hi])


def calibration_lists(train, given, n_nodes, n_rel, relations=None):
    """The cells of a per-relation calibration in the form the entries of include/tipk.h section 4r read (host function, CPU
    tensors).  train, given: (edge_index int [2, T], edge_type int [T]) -- the training triples and the calibration
    (held-out) triples.  A pair is unordered: (u, v), (v, u) and repeats are ONE cell; self pairs are dropped; a given pair
    that is also a training pair of its relation is dropped and counted.  relations: the ids that become the queries, in
    that order (None: all n_rel).
    -> CalibrationLists(ptr int64 [Q + 1], u, v int32 [D] with u < v, sorted by (u, v) inside a query, wpos fp32 [D] (1/M for
    a POS cell, 0 for a TRAIN cell), wneg fp32 [D] = -1/M, dense_w fp32 [Q] = 1/M, q_rel int32 [Q], n_pos, n_neg, n_dropped
    int64 [Q]); M = n (n - 1) / 2 - |TRAIN| = n_pos + n_neg; M == 0 gives dense_w = wpos = wneg = 0.
    ValueError for an id outside its range or a malformed argument."""
    n, n_rel = int(n_nodes), int(n_rel)
    if n < 1 or n_rel < 1:
        raise ValueError('n_nodes and n_rel must be >= 1, not %d and %d' % (n, n_rel))
    tr = _distinct_cells(train[0], train[1], n, n_rel, 'train')
    gv = _distinct_cells(given[0], given[1], n, n_rel, 'given')
    if relations is None:
        rel = torch.arange(n_rel, dtype=torch.int64)
    else:
        rel = torch.as_tensor(relations).to('cpu')
        if rel.numel() and (rel.dtype.is_floating_point or rel.dtype == torch.bool):
            raise ValueError('relations: int ids expected, got %s' % rel.dtype)
        rel = rel.to(torch.int64).reshape(-1)
        if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= n_rel):
            raise ValueError('relations: side-effect id out of range: [%d, %d] for %d side effects'
                             % (int(rel.min()), int(rel.max()), n_rel))
    in_train = torch.isin(gv, tr)
    pos = gv[~in_train]
    cells = n * n
    per = lambda keys: torch.bincount(torch.div(keys, cells, rounding_mode='floor'), minlength=n_rel)   # noqa: E731
    n_train, n_pos, n_drop = per(tr), per(pos), per(gv[in_train])
    big_m = n * (n - 1) // 2 - n_train
    merged, order = torch.sort(torch.cat([tr, pos]))                     # (TRAIN and POS are disjoint: no key twice)
    is_pos = torch.cat([torch.zeros(tr.numel(), dtype=torch.bool), torch.ones(pos.numel(), dtype=torch.bool)])[order]
    first = torch.searchsorted(merged, rel * cells)
    last = torch.searchsorted(merged, (rel + 1) * cells)
    count = last - first
    ptr = torch.zeros(rel.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(count, 0)
    q_of = torch.repeat_interleave(torch.arange(rel.numel(), dtype=torch.int64), count)
    take = first[q_of] + torch.arange(int(ptr[-1]), dtype=torch.int64) - ptr[:-1][q_of]
    key, posf = merged[take] % cells, is_pos[take]
    m_q = big_m[rel].to(torch.float64)
    dense = torch.where(m_q > 0, 1.0 / m_q.clamp(min=1.0), torch.zeros_like(m_q))
    return CalibrationLists(ptr, torch.div(key, n, rounding_mode='floor').to(torch.int32), (key % n).to(torch.int32),
                            torch.where(posf, dense[q_of], torch.zeros_like(dense[q_of])).to(torch.float32),
                            (-dense[q_of]).to(torch.float32), dense.to(torch.float32), rel.to(torch.int32), n_pos[rel],
                            big_m[rel] - n_pos[rel], n_drop[rel])


def calibration_queries(cl, index):
    """The queries `index` (int64 positions, in that order) of a `CalibrationLists` as a `CalibrationLists` of their own: a row
    subset, no second pass over the triples (host)."""
    index = torch.as_tensor(index, dtype=torch.int64).reshape(-1)
    count = (cl.ptr[1:] - cl.ptr[:-1])[index]
    ptr = torch.zeros(index.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(count, 0)
    q_of = torch.repeat_interleave(torch.arange(index.numel(), dtype=torch.int64), count)
    take = cl.ptr[:-1][index][q_of] + torch.arange(int(ptr[-1]), dtype=torch.int64) - ptr[:-1][q_of]
    return CalibrationLists(ptr, cl.u[take], cl.v[take], cl.wpos[take], cl.wneg[take], cl.dense_w[index], cl.q_rel[index],
                            cl.n_pos[index], cl.n_neg[index], cl.n_dropped[index])


def _calibrate_operands(z, rel_w, cl, l2, who):
    """z and rel_w as the calibration entries read them and the lists of `cl` (a `CalibrationLists`) on their device."""
    z, rel_w = _distmult_operands(z, rel_w, who)
    if not float(l2) >= 0:
        raise _lib.TipkError('%s: l2 must be >= 0, not %r' % (who, l2))
    lists, n_q = _lists_on(z.device, cl, ('u', 'v'), ('q_rel',), who, 'cell')
    ws = _fit_workspace(lib().tipk_distmult_calibrate_workspace_bytes(z.shape[0], z.shape[1], n_q), z.device, who,
                        'n = %d, dim = %d, n_q = %d' % (z.shape[0], z.shape[1], n_q), '4r')
    return z, rel_w, lists, n_q, ws


def distmult_calibrate_supported(n_nodes, dim, n_q=1):
    return bool(lib().tipk_distmult_calibrate_supported(n_nodes, dim, n_q))


def distmult_calibrate_stats(z, rel_w, ab, cl, l2=1e-6, active=None, out=None):
    """Loss, gradient and Hessian of the calibration objective at the trial maps ab [Q, 2] = (scale, offset) (include/tipk.h
    section 4r).  cl: the `CalibrationLists` of `calibration_lists` (moved to z's device); active: None or int [Q], 0 = leave
    that query's rows of `out` untouched; out: None or (loss [Q], grad [Q, 2], hess [Q, 2, 2]) to write into.
    -> (loss, grad, hess), fp32, the l2 term included.  Does not synchronise."""
    z, rel_w, (pptr, pu, pv, wpos, wneg, dense, qrel), n_q, ws = _calibrate_operands(z, rel_w, cl, l2, 'distmult_calibrate_stats')
    ab, active, (loss, grad, hess) = _trial_active_out(ab, active, out, n_q, 2, z.device, 'distmult_calibrate_stats', 'ab')
    check(lib().tipk_distmult_calibrate_stats(ptr(z), z.shape[0], z.shape[1], ptr(rel_w), rel_w.shape[0], ptr(qrel), ptr(ab),
                                              n_q, ptr(dense), ptr(pptr), ptr(pu), ptr(pv), ptr(wpos), ptr(wneg), pu.numel(),
                                              float(l2), ptr(active), ptr(loss), ptr(grad), ptr(hess), ptr(ws),
                                              stream_ptr(z.device)), 'tipk_distmult_calibrate_stats')
    return loss, grad, hess


def distmult_calibrate(z, rel_w, cl, l2=1e-6, init=None, max_iter=32, gtol=1e-6):
    """Fit the Platt map (scale, offset) of every query of `cl` by damped Newton steps on two unknowns: max_iter + 1
    (statistics, step) launches enqueued by ONE `tipk_distmult_calibrate` call (include/tipk.h section 4r).  init: None (the
    identity (1, 0)) or [Q, 2].
    -> (ab [Q, 2], loss [Q], grad [Q, 2], info int32 [Q, 4] = (status, evaluations, accepted, rejected)); status as
    `distmult_fit`.  Does not synchronise."""
    z, rel_w, (pptr, pu, pv, wpos, wneg, dense, qrel), n_q, ws = _calibrate_operands(z, rel_w, cl, l2, 'distmult_calibrate')
    dev = z.device
    init, ab, loss, grad, info = _newton_outputs(init, n_q, 2, max_iter, gtol, dev, 'distmult_calibrate')
    check(lib().tipk_distmult_calibrate(ptr(z), z.shape[0], z.shape[1], ptr(rel_w), rel_w.shape[0], ptr(qrel), n_q, ptr(dense),
                                        ptr(pptr), ptr(pu), ptr(pv), ptr(wpos), ptr(wneg), pu.numel(), float(l2), ptr(init),
                                        int(max_iter), float(gtol), ptr(ab), ptr(loss), ptr(grad), ptr(info), ptr(ws),
                                        stream_ptr(dev)), 'tipk_distmult_calibrate')
    return ab, loss, grad, info


CONF_MODES ={'moderated': 0, 'bound': 1}                             # TIPK_CONF_MODERATED, TIPK_CONF_BOUND


def distmult_pair_conf_topk_supported(n_nodes, dim, n_rel, k=10):
    return bool(lib().tipk_distmult_pair_conf_topk_supported(n_nodes, dim, n_rel, k))


def spd_factor(hess, row_scale):
    """Cholesky factors of B symmetric positive definite matrices and their scaled inverses (include/tipk.h section 4p).
    hess [B, dim, dim] (only the lower triangle is read), row_scale [B].
    -> (L [B, dim, dim] = chol(hess), W [B, dim, dim] = row_scale * L^-1 in the PHYSICAL layout the query entry reads:
    W[b, j, i] holds the logical entry (i, j), i.e. the tensor is the transpose of the lower-triangular factor; status
    int32 [B], 1 = factored, 0 = not positive definite or not finite: that row's L and W are zeros).  Does not synchronise."""
    hess, row_scale = _f32c(hess).contiguous(), _f32c(row_scale).contiguous()
    require_device(hess, row_scale)
    if hess.dim() != 3 or hess.shape[1] != hess.shape[2] or tuple(row_scale.shape) != (hess.shape[0],):
        raise _lib.TipkError('spd_factor: hess [B, dim, dim] and row_scale [B] expected, got %s and %s'
                             % (tuple(hess.shape), tuple(row_scale.shape)))
    dev = hess.device
    out_l, out_w = torch.empty_like(hess), torch.empty_like(hess)
    status = torch.empty(hess.shape[0], dtype=torch.int32, device=dev)
    check(lib().tipk_spd_factor(ptr(hess), ptr(row_scale), hess.shape[0], hess.shape[1], ptr(out_l), ptr(out_w), ptr(status),
                                stream_ptr(dev)), 'tipk_spd_factor')
    return out_l, out_w, status


def distmult_pair_conf_topk(z, rel_w, w_fac, pairs, k, mode, c=0.0, known=None, dense=False):
    """The k best relations of every pair by a key that knows the variance of the logit under the decoder rows' Laplace
    posterior (include/tipk.h section 4p).  w_fac [n_rel, dim, dim]: the W of `spd_factor` / `distmult_posterior`; pairs and
    known as `distmult_pair_topk`; mode 0 | 'moderated': key = s / sqrt(1 + pi/8 var); 1 | 'bound': key = s + c sqrt(var).
    -> (key fp32 [P, k], relation int32 [P, k], logit [P, k], var [P, k], dense_logit, dense_var): key descending then
    ascending relation id, padding (-inf, -1, -inf, +inf); the dense pair [P, n_rel] (known relations included) with
    dense = True, else (None, None).  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_pair_conf_topk')
    w_fac = _f32c(w_fac).contiguous()
    require_device(w_fac)
    n, dim, n_rel, k = z.shape[0], z.shape[1], rel_w.shape[0], int(k)
    if tuple(w_fac.shape) != (n_rel, dim, dim):
        raise _lib.TipkError('distmult_pair_conf_topk: w_fac [%d, %d, %d] expected, got %s' % (n_rel, dim, dim, tuple(w_fac.shape)))
    mode = CONF_MODES.get(mode, mode)
    dev = z.device
    pu, pv, keys, kptr, krel, n_keys = _pair_topk_lists(pairs, known, dev)
    n_p = pu.numel()
    out_key, out_rel = _topk_outputs(n_p, k, 1, dev)
    out_logit, out_var = torch.empty_like(out_key), torch.empty_like(out_key)
    d_logit = torch.empty((n_p, n_rel), dtype=torch.float32, device=dev) if dense else None
    d_var = torch.empty((n_p, n_rel), dtype=torch.float32, device=dev) if dense else None
    check(lib().tipk_distmult_pair_conf_topk(ptr(z), n, dim, ptr(rel_w), ptr(w_fac), n_rel, ptr(pu), ptr(pv), n_p, ptr(keys),
                                             ptr(kptr), ptr(krel), n_keys, k, int(mode), float(c), ptr(out_key), ptr(out_rel),
                                             ptr(out_logit), ptr(out_var), ptr(d_logit), ptr(d_var), stream_ptr(dev)),
          'tipk_distmult_pair_conf_topk')
    return out_key, out_rel, out_logit, out_var, d_logit, d_var


def distmult_posterior(z, w, fp, l2):
    """The Laplace posterior N(w_b, (P_b H_b)^-1) of the decoder rows w [B, dim] given the recorded pairs `fp` (a `FitPairs`):
    `distmult_fit_stats` at w, then `spd_factor` with row_scale = P_b^(-1/2) (include/tipk.h sections 4m, 4p).
    -> (W [B, dim, dim] physical layout of `spd_factor`, L, status int32 [B], hess [B, dim, dim]).  Synchronises nowhere: the
    caller reads `status`."""
    if not float(l2) > 0:
        raise _lib.TipkError('distmult_posterior: l2 must be > 0 (the prior makes the Hessian positive definite), not %r' % (l2,))
    _, _, hess = distmult_fit_stats(z, w, fp, l2)
    scale = fp.n_pairs.to(device=hess.device, dtype=torch.float64).clamp(min=1.0).rsqrt().to(torch.float32)
    out_l, out_w, status = spd_factor(hess, scale)
    return out_w, out_l, status, hess


def targets_by_relation(edge_index, edge_type, n_rel):
    """Triples (u, v, r) grouped by the relation query r that ranks the pair {u, v} -- for the screen rank entry
    (include/tipk.h section 4h) -> (q_rel int32 [Q], tgt_ptr int64 [Q + 1], tgt_u int32 [T], tgt_v int32 [T], order int64
    [T]): one query per relation that has triples, relations ascending; query q owns tgt_u/tgt_v[tgt_ptr[q]:tgt_ptr[q + 1]]
    in the given orientation and the caller's order (repeats stay), and order[i] is the caller's position of grouped triple
    i: `out[order] = result` scatters a result back.  n_rel only documents the id range (ids are not checked here: the
    entry leaves a query outside [0, n_rel) unranked).  Torch ops on edge_index's device (CPU tensors work too)."""
    edge_index, edge_type = _triples(edge_index, edge_type)
    keys, tgt_ptr, order = _group_by_key(edge_type.to(device=edge_index.device, dtype=torch.int64))
    return (keys.to(torch.int32), tgt_ptr, edge_index[0][order].to(torch.int32).contiguous(),
            edge_index[1][order].to(torch.int32).contiguous(), order)


def distmult_screen_rank(z, rel_w, q_rel, tgt_ptr, tgt_u, tgt_v, known=None):
    """The filtered rank of given drug pairs among all unordered pairs, per relation query, by DistMult logit (include/tipk.h
    section 4h).

    q_rel: int tensor [Q]; tgt_ptr int [Q + 1], tgt_u / tgt_v int [T]: query q is relation q_rel[q] and owns the target pairs
    tgt_u/tgt_v[tgt_ptr[q]:tgt_ptr[q+1]] (`targets_by_relation`); known: None or (keys int64 u*n+v sorted inside each
    relation, ptr int64 [n_rel + 1]), the relation-major lists `distmult_screen` takes; all on the device.
    -> (rank int32 [T], logit float32 [T]): rank = 1 + the number of pairs a < b, with neither a*n+b nor b*n+a listed for r,
    that beat the target (higher logit, or equal logit and lower key); rank - 1 is the pair's position in the relation query
    (r, -1) of `distmult_screen` under the same filter, and the logit is that query's, equal for (u, v) and (v, u).
    (0, NaN): not ranked -- r outside [0, n_rel), u or v outside [0, n), u == v, a NaN logit.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_screen_rank')
    dev = z.device
    q_rel, tgt_v = torch.as_tensor(q_rel), torch.as_tensor(tgt_v)
    require_device(q_rel, tgt_v)
    if q_rel.dim() != 1 or q_rel.dtype.is_floating_point:
        raise _lib.TipkError('queries: an int tensor q_rel [Q] expected, got %s %s' % (q_rel.dtype, tuple(q_rel.shape)))
    tptr, tu, n_tgt, out_rank, out_logit = _rank_targets(tgt_ptr, tgt_u, q_rel.numel(), dev)
    if tgt_v.dim() != 1 or tgt_v.numel() != n_tgt or tgt_v.dtype.is_floating_point:
        raise _lib.TipkError('targets: int tensors tgt_u [%d] and tgt_v [%d] expected, got tgt_v %s %s'
                             % (n_tgt, n_tgt, tgt_v.dtype, tuple(tgt_v.shape)))
    keys, kptr = _relation_known(known)
    qr, tv = q_rel.to(torch.int32).contiguous(), tgt_v.to(torch.int32).contiguous()
    n, dim = z.shape
    ws_bytes = int(lib().tipk_distmult_screen_rank_workspace_bytes(n, dim, qr.numel(), n_tgt))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
    check(lib().tipk_distmult_screen_rank(ptr(z), n, dim, ptr(rel_w), rel_w.shape[0], ptr(qr), qr.numel(), ptr(tptr), ptr(tu),
                                          ptr(tv), n_tgt, ptr(keys), ptr(kptr), ptr(out_rank), ptr(out_logit), ptr(ws),
                                          stream_ptr(dev)), 'tipk_distmult_screen_rank')
    return out_rank, out_logit


REGIMEN_AGGREGATES = {'max': 0, 'noisy_or': 1}                        # TIPK_REGIMEN_MAX, TIPK_REGIMEN_NOISY_OR


def regimen_max_drugs():
    """The longest regimen the regimen top-k entries rank (include/tipk.h section 4e)."""
    return int(lib().tipk_regimen_max_drugs())


def _regimen_args(reg_drugs, reg_ptr, k, aggregate, known, dev):
    if aggregate not in REGIMEN_AGGREGATES:
        raise _lib.TipkError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
    reg_drugs, reg_ptr = torch.as_tensor(reg_drugs), torch.as_tensor(reg_ptr)
    require_device(reg_drugs, reg_ptr)
    if reg_drugs.dim() != 1 or reg_ptr.dim() != 1 or reg_ptr.numel() < 1 or reg_drugs.dtype.is_floating_point \
            or reg_ptr.dtype.is_floating_point:
        raise _lib.TipkError('regimens: int tensors reg_drugs [n_entries] and reg_ptr [n_regimens + 1] expected, got %s %s '
                             'and %s %s' % (reg_drugs.dtype, tuple(reg_drugs.shape), reg_ptr.dtype, tuple(reg_ptr.shape)))
    drugs, rptr = reg_drugs.to(torch.int32).contiguous(), reg_ptr.to(torch.int64).contiguous()
    if drugs.numel() == 0:                                               # an empty tensor has no address
        drugs = torch.zeros(1, dtype=torch.int32, device=dev)
    n_g, k = rptr.numel() - 1, int(k)
    return (drugs, rptr, n_g, k, REGIMEN_AGGREGATES[aggregate], _known_lists(known)) + _topk_outputs(n_g, k, 2, dev)


def _regimen_result(out_s, out_r, out_p):
    have = out_p >= 0
    return out_s, out_r, torch.where(have, out_p & 0xffff, out_p), torch.where(have, out_p >> 16, out_p)


def distmult_regimen_topk(z, rel_w, reg_drugs, reg_ptr, k, aggregate='max', known=None):
    """The k best relations of every drug list by the DistMult logits of its pairs, aggregated (include/tipk.h section 4e).

    reg_drugs int [n_entries], reg_ptr int [G + 1] on the device: regimen g is reg_drugs[reg_ptr[g]:reg_ptr[g + 1]], its
    pairs are the position pairs i < j.  aggregate: 'max' (the largest logit) or 'noisy_or' (sum of softplus(logit) =
    -log(1 - P)).  known: None or the pair-major lists of `known_relations_by_pair` on the device: a known triple
    contributes nothing.  -> (score float32 [G, k], relation int32 [G, k], pair_i int32 [G, k], pair_j int32 [G, k]):
    descending score then ascending relation id, (pair_i, pair_j) the list positions of the pair with the largest logit;
    (-inf, -1, -1, -1) pads a row with fewer than k candidates.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_regimen_topk')
    dev = z.device
    drugs, rptr, n_g, k, agg, (keys, kptr, krel, n_keys), out_s, out_r, out_p = _regimen_args(reg_drugs, reg_ptr, k,
                                                                                              aggregate, known, dev)
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]
    check(lib().tipk_distmult_regimen_topk(ptr(z), n, dim, ptr(rel_w), n_rel, ptr(drugs), ptr(rptr), n_g, ptr(keys),
                                           ptr(kptr), ptr(krel), n_keys, agg, k, ptr(out_s), ptr(out_r), ptr(out_p), None,
                                           stream_ptr(dev)), 'tipk_distmult_regimen_topk')
    return _regimen_result(out_s, out_r, out_p)


def pair_table_regimen_topk(s1, s2, reg_drugs, reg_ptr, k, aggregate='max', known=None):
    """`distmult_regimen_topk` for the NN decoder's node-major tables s1, s2 [n, n_rel] (row stride free, the same for
    both): the logit of the position pair i < j under r is s1[d_i, r] + s2[d_j, r]."""
    s1, s2 = _table_pair(s1, s2, 'pair_table_regimen_topk')
    dev = s1.device
    drugs, rptr, n_g, k, agg, (keys, kptr, krel, n_keys), out_s, out_r, out_p = _regimen_args(reg_drugs, reg_ptr, k,
                                                                                              aggregate, known, dev)
    n, n_rel = s1.shape[0], s1.shape[1]
    check(lib().tipk_pair_table_regimen_topk(ptr(s1), ptr(s2), s1.stride(0), n, n_rel, ptr(drugs), ptr(rptr), n_g,
                                             ptr(keys), ptr(kptr), ptr(krel), n_keys, agg, k, ptr(out_s), ptr(out_r),
                                             ptr(out_p), stream_ptr(dev)), 'tipk_pair_table_regimen_topk')
    return _regimen_result(out_s, out_r, out_p)


def addon_max_context():
    """The longest context (drugs a patient already takes) the add-on burden entries score (include/tipk.h section 4i)."""
    return int(lib().tipk_addon_max_context())


def _addon_args(ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights, known, n_rel, dev):
    if aggregate not in REGIMEN_AGGREGATES:
        raise _lib.TipkError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
    ctx_drugs, ctx_ptr, cand = torch.as_tensor(ctx_drugs), torch.as_tensor(ctx_ptr), torch.as_tensor(cand)
    cand_ptr = None if cand_ptr is None else torch.as_tensor(cand_ptr)
    require_device(ctx_drugs, ctx_ptr, cand, cand_ptr, weights)
    ints = (ctx_drugs, ctx_ptr, cand) + (() if cand_ptr is None else (cand_ptr,))
    if any(t.dim() != 1 or t.dtype.is_floating_point for t in ints) or ctx_ptr.numel() < 1:
        raise _lib.TipkError('add-on queries: 1-d int tensors ctx_drugs, ctx_ptr [Q + 1], cand and cand_ptr [Q + 1] (or None) '
                             'expected, got %s' % ', '.join('%s %s' % (t.dtype, tuple(t.shape)) for t in ints))
    n_q = ctx_ptr.numel() - 1
    if cand_ptr is not None and cand_ptr.numel() != n_q + 1:
        raise _lib.TipkError('add-on queries: cand_ptr has %d entries for %d queries' % (cand_ptr.numel(), n_q))
    if weights is not None:
        weights = _f32c(weights).contiguous()
        if weights.dim() != 1 or weights.numel() != n_rel:
            raise _lib.TipkError('weights: a float tensor [%d] expected, got %s' % (n_rel, tuple(weights.shape)))
    drugs, cptr = ctx_drugs.to(torch.int32).contiguous(), ctx_ptr.to(torch.int64).contiguous()
    cd = cand.to(torch.int32).contiguous()
    dptr = None if cand_ptr is None else cand_ptr.to(torch.int64).contiguous()
    n_cand, k = cd.numel(), int(k)
    if drugs.numel() == 0:                                               # an empty tensor has no address
        drugs = torch.zeros(1, dtype=torch.int32, device=dev)
    out_b = torch.empty((n_cand,) if dptr is not None else (n_q, n_cand), dtype=torch.float32, device=dev)
    best_b = best_p = None
    if k > 0:                                                            # (no launch without candidates: the rows are padding)
        best_b = torch.full((n_q, k), float('inf'), dtype=torch.float32, device=dev) if n_cand == 0 \
            else torch.empty((n_q, k), dtype=torch.float32, device=dev)
        best_p = torch.full((n_q, k), -1, dtype=torch.int32, device=dev) if n_cand == 0 \
            else torch.empty((n_q, k), dtype=torch.int32, device=dev)
    return drugs, cptr, n_q, cd, dptr, n_cand, weights, k, REGIMEN_AGGREGATES[aggregate], _known_lists(known), out_b, \
        best_b, best_p


def distmult_addon_burden(z, rel_w, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights=None, known=None):
    """The burden every candidate drug adds to every context (a patient's drug list) by the DistMult logits of its pairs with
    the context, and the k candidates of each query with the lowest burden (include/tipk.h section 4i).

    ctx_drugs int [n_entries], ctx_ptr int [Q + 1]: context q is ctx_drugs[ctx_ptr[q]:ctx_ptr[q + 1]].  cand int, cand_ptr
    int [Q + 1]: query q owns cand[cand_ptr[q]:cand_ptr[q + 1]]; cand_ptr None: the one list `cand` serves every query.
    aggregate: 'noisy_or' (P_r = 1 - prod (1 - sigma(logit)) over the context) or 'max' (P_r = sigma(largest logit));
    weights: None (all 1) or float [n_rel], finite and >= 0; known: None or the pair-major lists of
    `known_relations_by_pair`: a known triple contributes nothing.  All on the device.
    -> (burden float32 [n_cand] (cand_ptr given) or [Q, n_cand] (shared list), best_burden float32 [Q, k], best_pos int32
    [Q, k]): burden = sum_r weights[r] * P_r, NaN where the task is not applicable (candidate out of range or in its
    context, a context of 0 or more than `addon_max_context()` drugs or with an id out of range, a NaN logit); best_*: the
    k lowest burdens of each query, ascending, ties by position in the query's list, padded with (+inf, -1); both None for
    k = 0.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_addon_burden')
    dev = z.device
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]
    drugs, cptr, n_q, cd, dptr, n_cand, wts, k, agg, (keys, kptr, krel, n_keys), out_b, best_b, best_p = _addon_args(
        ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights, known, n_rel, dev)
    check(lib().tipk_distmult_addon_burden(ptr(z), n, dim, ptr(rel_w), n_rel, ptr(drugs), ptr(cptr), n_q, ptr(cd), ptr(dptr),
                                           n_cand, ptr(wts), ptr(keys), ptr(kptr), ptr(krel), n_keys, agg, k, ptr(out_b),
                                           ptr(best_b), ptr(best_p), None, stream_ptr(dev)), 'tipk_distmult_addon_burden')
    return out_b, best_b, best_p


def pair_table_addon_burden(s1, s2, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights=None, known=None):
    """`distmult_addon_burden` for the NN decoder's node-major tables s1, s2 [n, n_rel] (row stride free, the same for
    both): the logit of candidate c with context drug s under r is s1[min(c, s), r] + s2[max(c, s), r]."""
    s1, s2 = _table_pair(s1, s2, 'pair_table_addon_burden')
    dev = s1.device
    n, n_rel = s1.shape[0], s1.shape[1]
    drugs, cptr, n_q, cd, dptr, n_cand, wts, k, agg, (keys, kptr, krel, n_keys), out_b, best_b, best_p = _addon_args(
        ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights, known, n_rel, dev)
    check(lib().tipk_pair_table_addon_burden(ptr(s1), ptr(s2), s1.stride(0), n, n_rel, ptr(drugs), ptr(cptr), n_q, ptr(cd),
                                             ptr(dptr), n_cand, ptr(wts), ptr(keys), ptr(kptr), ptr(krel), n_keys, agg, k,
                                             ptr(out_b), ptr(best_b), ptr(best_p), stream_ptr(dev)),
          'tipk_pair_table_addon_burden')
    return out_b, best_b, best_p


ComboLimits = collections.namedtuple('ComboLimits', ['max_fixed', 'max_slots', 'max_alternatives', 'max_combinations'])
ComboPlan = collections.namedtuple('ComboPlan', ['fix_drugs', 'fix_ptr', 'alt', 'alt_ptr', 'slot_ptr', 'comb_ptr', 'row_ptr', 'n_q',
                                     'n_fix', 'n_alt', 'n_slots', 'n_comb', 'n_rows', 'host_comb_ptr', 'host_row_ptr'])
COMBO_WORKSPACE_BYTES = 1 << 30                                        # the tables of one entry call: more queries are chunked


def combo_limits():
    """The limits of the combination-burden entries (include/tipk.h section 4n), read from the library."""
    return ComboLimits(int(lib().tipk_addon_max_context()), int(lib().tipk_combo_max_slots()),
                       int(lib().tipk_combo_max_alternatives()), int(lib().tipk_combo_max_combinations()))


def combo_plan(fix_drugs, fix_ptr, alt, alt_ptr, slot_ptr, device):
    """The query lists of the combination-burden entries on `device`, with the two offset arrays the entries size their
    output and workspace by.  fix_drugs int [n_fix], fix_ptr int [Q + 1]: the fixed drugs of every query; slot_ptr int
    [Q + 1]: query q owns the slots slot_ptr[q]:slot_ptr[q + 1]; alt int [n_alt], alt_ptr int [n_slots + 1]: the alternatives
    of every slot (-1: leave the slot empty).  Tensors or lists, host or device -- the sizes are taken on the host (one
    synchronisation when the lists live on the device); the entry calls that use the plan do not synchronise.
    A query within the limits owns prod A_s entries of the result (1 without slots) and 1 + sum A_s + sum_{s < t} A_s A_t
    workspace rows; one that breaks a structural limit (more than `max_slots` slots, an empty slot, more than
    `max_alternatives` alternatives or `max_combinations` combinations, offsets that descend) owns ONE entry, which the
    kernel writes as NaN, and no row.  Ids and fixed lists are checked by the kernel."""
    lim = combo_limits()
    host = [torch.as_tensor(t).detach().to('cpu') for t in (fix_drugs, fix_ptr, alt, alt_ptr, slot_ptr)]
    host = [t.to(torch.int64) if t.numel() == 0 and t.dim() == 1 else t for t in host]       # (an empty list has no dtype)
    if any(t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool for t in host):
        raise _lib.TipkError('combination queries: 1-d int tensors fix_drugs, fix_ptr [Q + 1], alt, alt_ptr [n_slots + 1] and '
                             'slot_ptr [Q + 1] expected, got %s' % ', '.join('%s %s' % (t.dtype, tuple(t.shape)) for t in host))
    fd, fp, al, ap, sp = (t.to(torch.int64) for t in host)
    n_q = fp.numel() - 1
    if n_q < 0 or sp.numel() != n_q + 1 or ap.numel() < 1:
        raise _lib.TipkError('combination queries: fix_ptr and slot_ptr [Q + 1] and alt_ptr [n_slots + 1] expected, got %d, %d '
                             'and %d entries' % (fp.numel(), sp.numel(), ap.numel()))
    n_slots = ap.numel() - 1
    size = (ap[1:] - ap[:-1]).tolist()
    comb, rows = [0], [0]
    for s0, s1 in zip(sp[:-1].tolist(), sp[1:].tolist()):
        c, r, seen = 1, 1, 0
        ok = 0 <= s0 <= s1 <= n_slots and s1 - s0 <= lim.max_slots
        for a in (size[s0:s1] if ok else ()):
            ok = ok and a >= 1
            c, r, seen = c * max(a, 0), r + a + a * seen, seen + a
        if not ok or seen > lim.max_alternatives or c > lim.max_combinations:
            c, r = 1, 0
        comb.append(comb[-1] + c)
        rows.append(rows[-1] + r)
    comb_ptr, row_ptr = torch.tensor(comb, dtype=torch.int64), torch.tensor(rows, dtype=torch.int64)
    parts = [fp, sp, ap, comb_ptr, row_ptr]
    flat = torch.cat(parts).to(device)                                   # two uploads: the offsets, the ids
    cuts = [0]
    for t in parts:
        cuts.append(cuts[-1] + t.numel())
    fp_d, sp_d, ap_d, cp_d, rp_d = (flat[cuts[i]:cuts[i + 1]] for i in range(5))
    ids = torch.cat([fd, al, torch.zeros(1, dtype=torch.int64)]).to(torch.int32).to(device)   # (an empty tensor has no address)
    fd_d, al_d = ids[:max(fd.numel(), 1)], ids[fd.numel():]
    return ComboPlan(fd_d, fp_d, al_d, ap_d, sp_d, cp_d, rp_d, n_q, fd.numel(), al.numel(), n_slots, comb[-1], rows[-1],
                     comb_ptr, row_ptr)


def _combo_run(entry, ws_bytes, plan, k, aggregate, weights, known, n_rel, dev, who):
    """The shared body of the two combination-burden ops: outputs, workspace, chunks of queries, the entry calls.
    entry(lists..., out pointers, workspace) -> status; ws_bytes(n_rows) -> bytes."""
    if aggregate not in REGIMEN_AGGREGATES:
        raise _lib.TipkError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
    if not isinstance(plan, ComboPlan):
        raise _lib.TipkError('%s: a ComboPlan (ops.combo_plan) expected, got %s' % (who, type(plan).__name__))
    require_device(plan.fix_ptr, weights)
    if weights is not None:
        weights = _f32c(weights).contiguous()
        if weights.dim() != 1 or weights.numel() != n_rel:
            raise _lib.TipkError('weights: a float tensor [%d] expected, got %s' % (n_rel, tuple(weights.shape)))
    keys, kptr, krel, n_keys = _known_lists(known)
    k, agg, n_q = int(k), REGIMEN_AGGREGATES[aggregate], plan.n_q
    out_b = torch.empty((plan.n_comb,), dtype=torch.float32, device=dev)
    best_b = best_c = None
    if k > 0:
        best_b = torch.empty((n_q, k), dtype=torch.float32, device=dev)
        best_c = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    # chunks of consecutive queries whose tables fit COMBO_WORKSPACE_BYTES (a single query always gets its own call)
    rows = plan.host_row_ptr.tolist()
    cuts, q0 = [0], 0
    for q in range(1, n_q + 1):
        if q - q0 > 1 and ws_bytes(rows[q] - rows[q0]) > COMBO_WORKSPACE_BYTES:
            cuts.append(q - 1)
            q0 = q - 1
    if n_q > 0:
        cuts.append(n_q)
    ws_most = max([ws_bytes(rows[b] - rows[a]) for a, b in zip(cuts[:-1], cuts[1:])] + [0])
    if ws_most < 0:
        raise _lib.TipkError('%s: unsupported shape (see include/tipk.h section 4n)' % who)
    ws = torch.empty((max(ws_most, 16),), dtype=torch.uint8, device=dev)
    combs = plan.host_comb_ptr.tolist()
    for a, b in zip(cuts[:-1], cuts[1:]):
        check(entry(ptr(plan.fix_drugs), ptr(plan.fix_ptr[a:]), plan.n_fix, ptr(plan.alt), ptr(plan.alt_ptr), plan.n_alt,
                    ptr(plan.slot_ptr[a:]), plan.n_slots, ptr(plan.comb_ptr[a:]), ptr(plan.row_ptr[a:]), b - a,
                    combs[b] - combs[a], rows[b] - rows[a], ptr(weights), ptr(keys), ptr(kptr), ptr(krel), n_keys, agg, k,
                    ptr(out_b[combs[a]:]) if combs[b] > combs[a] else None, None if best_b is None else ptr(best_b[a:]),
                    None if best_c is None else ptr(best_c[a:]), ptr(ws), stream_ptr(dev)), who)
    return out_b, plan.comb_ptr, best_b, best_c


def distmult_combo_burden(z, rel_w, plan, k, aggregate='noisy_or', weights=None, known=None):
    """The total burden sum_r weights[r] * P_r of every combination of every query of `plan` (`combo_plan`) by the DistMult
    logits of ALL pairs of its regimen -- the fixed drugs plus one alternative per slot --, and the k combinations of each
    query with the lowest burden (include/tipk.h section 4n).

    aggregate, weights, known: as `distmult_addon_burden`.  -> (burden float32 [n_comb], comb_ptr int64 [Q + 1], best_burden
    float32 [Q, k], best_comb int32 [Q, k]): query q owns burden[comb_ptr[q]:comb_ptr[q + 1]], combination index = position
    in that range, the last slot running fastest (itertools.product); NaN where a combination is not applicable (two
    chosen drugs coincide, a chosen drug is fixed, a NaN logit) or the query is illegal; best_*: ascending burden, ties by
    combination index, padded with (+inf, -1); both None for k = 0.  Queries whose tables would take more than
    COMBO_WORKSPACE_BYTES are dealt to several entry calls.  Does not synchronise."""
    z, rel_w = _distmult_operands(z, rel_w, 'distmult_combo_burden')
    dev = z.device
    n, dim, n_rel = z.shape[0], z.shape[1], rel_w.shape[0]

    def entry(*lists):
        return lib().tipk_distmult_combo_burden(ptr(z), n, dim, ptr(rel_w), n_rel, *lists)

    return _combo_run(entry, lambda n_rows: int(lib().tipk_distmult_combo_burden_workspace_bytes(n, dim, n_rel, n_rows, int(k))),
                      plan, k, aggregate, weights, known, n_rel, dev, 'tipk_distmult_combo_burden')


def pair_table_combo_burden(s1, s2, plan, k, aggregate='noisy_or', weights=None, known=None):
    """`distmult_combo_burden` for the NN decoder's node-major tables s1, s2 [n, n_rel] (row stride free, the same for
    both): the logit of the drugs c, d under r is s1[min(c, d), r] + s2[max(c, d), r]."""
    s1, s2 = _table_pair(s1, s2, 'pair_table_combo_burden')
    dev = s1.device
    n, n_rel = s1.shape[0], s1.shape[1]

    def entry(*lists):
        return lib().tipk_pair_table_combo_burden(ptr(s1), ptr(s2), s1.stride(0), n, n_rel, *lists)

    return _combo_run(entry, lambda n_rows: int(lib().tipk_pair_table_combo_burden_workspace_bytes(n, n_rel, n_rows, int(k))),
                      plan, k, aggregate, weights, known, n_rel, dev, 'tipk_pair_table_combo_burden')


_IN_EDGES = DerivedCache(8)
_PAIR_EDGES = DerivedCache(8)


def in_edges_by_node(edge_index, range_list_or_type, n_nodes):
    """The in-edge CSR of include/tipk.h section 4j from a directed edge list (source_to_target: edge e runs from
    edge_index[0][e] to edge_index[1][e]) -> (in_ptr int64 [n_nodes + 1], in_src int32 [E], in_rel int32 [E]): node v owns the
    positions in_ptr[v] .. in_ptr[v+1], sorted by (relation, source); duplicate edges stay separate entries.
    range_list_or_type: range_list [R, 2] (relation r owns the edge positions [begin, end), the blocks tile the list in
    relation order) or edge_type int [E].  Built with torch ops on edge_index's device (CPU tensors work too): one stable
    sort of the key (dst * R + rel) * n + src.  IndexError for a node id outside [0, n_nodes) or a negative relation.
    Cached per (edge tensor, range or type tensor) by identity and version, the tensors pinned while cached
    (`_cache.DerivedCache`); arguments given as lists are not cached."""
    return _in_edges(edge_index, range_list_or_type, n_nodes, False, _IN_EDGES, 'in_edges_by_node')


def in_edges_by_pair(edge_index, range_list_or_type, n_nodes):
    """The in-edge CSR of include/tipk.h section 4o: as `in_edges_by_node`, but node v's positions are sorted by (SOURCE,
    relation), so the edges of one pair (source -> v) are adjacent -- in the order they have in `in_edges_by_node`'s
    (relation, source) segment.  -> (pe_ptr int64 [n_nodes + 1], pe_src int32 [E], pe_rel int32 [E]).  Same arguments, same
    errors, same caching rule (a cache of its own next to `in_edges_by_node`'s)."""
    return _in_edges(edge_index, range_list_or_type, n_nodes, True, _PAIR_EDGES, 'in_edges_by_pair')


def _in_edges(edge_index, range_list_or_type, n_nodes, by_pair, cache, who):
    """`in_edges_by_node` (by_pair False) / `in_edges_by_pair` (True): one stable sort of the edges' key.  Arguments given as
    lists are not cached (a temporary tensor's address names nothing)."""
    build = lambda: _in_edges_built(torch.as_tensor(edge_index), range_list_or_type, int(n_nodes), by_pair, who)
    if not (torch.is_tensor(edge_index) and torch.is_tensor(range_list_or_type)):
        return build()
    return cache.get((edge_index, range_list_or_type), int(n_nodes), build)


def _in_edges_built(edge_index, range_list_or_type, n, by_pair, who):
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype.is_floating_point:
        raise _lib.TipkError(who + ': an int tensor edge_index [2, E] expected, got %s %s'
                             % (edge_index.dtype, tuple(edge_index.shape)))
    n_edges, dev = edge_index.shape[1], edge_index.device
    rt = torch.as_tensor(range_list_or_type)
    if rt.dtype.is_floating_point:
        raise _lib.TipkError(who + ': an int range_list [R, 2] or edge_type [E] expected, got %s' % rt.dtype)
    if rt.dim() == 2 and rt.shape[1] == 2:
        ends = rt.to(device=dev, dtype=torch.int64)[:, 1].contiguous()
        if rt.shape[0] == 0 or int(ends[-1]) != n_edges:
            raise _lib.TipkError(who + ': range_list must tile all %d edges' % n_edges)
        rel = torch.bucketize(torch.arange(n_edges, device=dev), ends, right=True)
        n_rel = rt.shape[0]
    elif rt.dim() == 1 and rt.numel() == n_edges:
        rel = rt.to(device=dev, dtype=torch.int64)
        n_rel = int(rel.max()) + 1 if n_edges else 1
    else:
        raise _lib.TipkError(who + ': range_list [R, 2] or edge_type [%d] expected, got %s'
                             % (n_edges, tuple(rt.shape)))
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    if n_edges:
        lo, hi, rlo = torch.stack([edge_index.min(), edge_index.max(), rel.min()]).tolist()
        if lo < 0 or hi >= n:
            raise IndexError('node id out of range: [%d, %d] for %d nodes' % (lo, hi, n))
        if rlo < 0:
            raise IndexError('relation id out of range: %d' % rlo)
    order = torch.sort((dst * n + src) * n_rel + rel if by_pair else (dst * n_rel + rel) * n + src, stable=True)[1]
    in_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    in_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return in_ptr, src[order].to(torch.int32).contiguous(), rel[order].to(torch.int32).contiguous()


def rgcn_edge_attribution(h, basis, att, root, in_edges, q_node, probe, k):
    """The k in-edges of every queried node that contribute most to probe . z[node], z = the bias-free R-GCN layer
    (basis, att, root) applied to h (include/tipk.h section 4j; one launch, no E x d temporary).

    h [n, d_in] (row stride free), basis [B, d_in, d_out], att [R, B], root [d_in, d_out]: fp32 device tensors; in_edges:
    `in_edges_by_node` of the layer's graph, on the device; q_node int [Q]; probe fp32 [Q, d_out].
    -> (contrib float32 [Q, k], src int32 [Q, k], rel int32 [Q, k], own float32 [Q], total float32 [Q]): the k largest
    per-edge contributions c_e, descending, ties by position in the node's segment, with the edge's source and relation,
    padded with (-inf, -1, -1); own = probe . (h[node] root); total = the sum of ALL c_e of the node (fp64 accumulation,
    rounded once), so probe . z[node] = own + total up to rounding.  A node outside [0, n): padding and NaN own / total.
    Bitwise repeatable.  Does not synchronise (a first call checks the ids of `in_edges` once per tensor)."""
    h, basis, att, root, probe = _f32c(h), _f32c(basis).contiguous(), _f32c(att), _f32c(root).contiguous(), _f32c(probe)
    in_ptr, in_src, in_rel = in_edges
    q_node = torch.as_tensor(q_node)
    require_device(h, basis, att, root, probe, in_ptr, in_src, in_rel, q_node)
    if h.dim() != 2 or basis.dim() != 3 or att.dim() != 2 or root.dim() != 2 or basis.shape[1] != h.shape[1] or \
            att.shape[1] != basis.shape[0] or tuple(root.shape) != tuple(basis.shape[1:]):
        raise _lib.TipkError('rgcn_edge_attribution: h [n, d_in], basis [B, d_in, d_out], att [R, B], root [d_in, d_out] expected, '
                             'got %s, %s, %s, %s' % (tuple(h.shape), tuple(basis.shape), tuple(att.shape), tuple(root.shape)))
    n, d_in = h.shape
    n_bases, _, d_out = basis.shape
    n_rel, k = att.shape[0], int(k)
    if q_node.dim() != 1 or q_node.dtype.is_floating_point or probe.dim() != 2 or \
            tuple(probe.shape) != (q_node.numel(), d_out):
        raise _lib.TipkError('rgcn_edge_attribution: q_node int [Q] and probe [Q, %d] expected, got %s %s and %s'
                             % (d_out, q_node.dtype, tuple(q_node.shape), tuple(probe.shape)))
    if in_ptr.dtype != torch.int64 or in_src.dtype != torch.int32 or in_rel.dtype != torch.int32 or \
            in_ptr.numel() != n + 1 or in_src.dim() != 1 or in_src.shape != in_rel.shape:
        raise _lib.TipkError('rgcn_edge_attribution: in_edges = (int64 [%d], int32 [E], int32 [E]) of in_edges_by_node expected'
                             % (n + 1))
    if h.stride(0) < d_in or att.stride(0) < n_bases or probe.stride(0) < d_out:
        h, att, probe = h.contiguous(), att.contiguous(), probe.contiguous()
    _range_checked(in_src, n, 'in_edges source')
    _range_checked(in_rel, n_rel, 'in_edges relation')
    dev, n_q = h.device, q_node.numel()
    in_ptr, in_src, in_rel = in_ptr.contiguous(), in_src.contiguous(), in_rel.contiguous()
    qn = q_node.to(torch.int32).contiguous()
    contrib, src, rel = _topk_outputs(n_q, k, 2, dev)
    own = torch.empty(n_q, dtype=torch.float32, device=dev)
    total = torch.empty(n_q, dtype=torch.float32, device=dev)
    ws_bytes = int(lib().tipk_rgcn_attribution_workspace_bytes(n, n_bases, n_q))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if ws_bytes > 0 else None
    check(lib().tipk_rgcn_attribution(ptr(h), h.stride(0), n, d_in, ptr(basis), ptr(att), att.stride(0), n_rel, n_bases,
                                      ptr(root), d_out, ptr(in_ptr), ptr(in_src), ptr(in_rel), in_src.numel(), ptr(qn),
                                      ptr(probe), probe.stride(0), n_q, k, ptr(contrib), ptr(src), ptr(rel), ptr(own),
                                      ptr(total), ptr(ws), stream_ptr(dev)), 'tipk_rgcn_attribution')
    return contrib, src, rel, own, total


_PROT_EDGES = DerivedCache(8)


def targets_by_protein(dp_edge_index, n_prot, n_nodes):
    """The protein-side CSR of include/tipk.h section 4o from the P -> D edge list (dp_edge_index [2, E]: row 0 the protein id,
    row 1 n_prot + the drug id, as the data set stores it) -> (prot_ptr int64 [n_prot + 1], prot_drug int32 [E], inv_cnt
    float32 [n_nodes], cnt int64 [n_nodes]): protein t owns the positions prot_ptr[t] .. prot_ptr[t+1], drugs ascending,
    duplicates kept; cnt = the number of P -> D edges into every drug and inv_cnt = 1 / max(cnt, 1), correctly rounded.
    Built with torch ops on the tensor's device; IndexError for an id out of range.  Cached per edge tensor
    (`_cache.DerivedCache`); an edge list given as a Python list is not cached."""
    build = lambda: _targets_by_protein(torch.as_tensor(dp_edge_index), int(n_prot), int(n_nodes))
    if not torch.is_tensor(dp_edge_index):
        return build()
    return _PROT_EDGES.get((dp_edge_index,), (int(n_prot), int(n_nodes)), build)


def _targets_by_protein(ei, n_prot, n):
    if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype.is_floating_point:
        raise _lib.TipkError('targets_by_protein: an int tensor dp_edge_index [2, E] expected, got %s %s'
                             % (ei.dtype, tuple(ei.shape)))
    prot, drug = ei[0].to(torch.int64), ei[1].to(torch.int64) - n_prot
    if ei.shape[1]:
        plo, phi, dlo, dhi = torch.stack([prot.min(), prot.max(), drug.min(), drug.max()]).tolist()
        if plo < 0 or phi >= n_prot:
            raise IndexError('protein id out of range: [%d, %d] for %d proteins' % (plo, phi, n_prot))
        if dlo < 0 or dhi >= n:
            raise IndexError('drug id out of range: [%d, %d] for %d drugs' % (dlo, dhi, n))
    order = torch.sort(prot * n + drug, stable=True)[1]
    prot_ptr = torch.zeros(n_prot + 1, dtype=torch.int64, device=ei.device)
    prot_ptr[1:] = torch.cumsum(torch.bincount(prot, minlength=n_prot), 0)
    cnt = torch.bincount(drug, minlength=n)
    inv_cnt = 1.0 / cnt.clamp(min=1).to(torch.float32)
    return prot_ptr, drug[order].to(torch.int32).contiguous(), inv_cnt.contiguous(), cnt


def protein_attribution_supported(n_nodes, n_prot, n_rel, n_bases, ne, pd, p, d1, d2, cat, k):
    """Whether `protein_attribution` takes these sizes (include/tipk.h section 4o)."""
    return bool(lib().tipk_protein_attribution_supported(int(n_nodes), int(n_prot), int(n_rel), int(n_bases), int(ne), int(pd),
                                                         int(p), int(d1), int(d2), int(bool(cat)), int(k)))


def protein_attribution_workspace_bytes(n_nodes, n_bases, d1, p, n_q):
    """Bytes of workspace `protein_attribution` allocates for such a call (-1: sizes the entry does not take)."""
    return int(lib().tipk_protein_attribution_workspace_bytes(int(n_nodes), int(n_bases), int(d1), int(p), int(n_q)))


def protein_attribution(h_prot, hgcn_w, xe, h, layer1, layer2, pair_edges, targets, cat, q_node, probe, k):
    """The k protein targets every query's probe . z[node] rests on most, by one fused reverse pass through both bias-free
    R-GCN layers and the P -> D stage (include/tipk.h section 4o; no autograd, no per-edge temporary).

    h_prot [P, p]: the P-P encoder's output for every protein; hgcn_w [p, pd]; xe [n, ne]: the drug embedding rows already
    divided by d_norm; h [n, d1]: the stored relu(rgcn1(x0)) (read for its mask h > 0 only); layer1 / layer2 = (basis, att,
    root) of rgcn1 / rgcn2; pair_edges: `in_edges_by_pair` of the D-D graph; targets: `targets_by_protein` of the P -> D
    edges; cat: the encoder's mode; q_node int [Q]; probe fp32 [Q, d2].  All fp32 device tensors, row strides free.
    -> (contrib float32 [Q, k], protein int32 [Q, k], direct float32 [Q, k], features float32 [Q], proteins float32 [Q]):
    the k targeted proteins with the largest contribution c_t, descending, ties by ascending protein id, with the part of
    c_t that arrives through the queried drug's own P -> D edges, padded with (-inf, -1, +0); features = the sum of every
    drug's own-feature part, proteins = the sum of c_t over ALL targeted proteins (fp64 accumulation, rounded once), so
    probe . z[node] = features + proteins up to rounding.  A node outside [0, n): padding and NaN features / proteins.
    Bitwise repeatable, and the same for a query whatever else is in the call.  Does not synchronise (a first call checks
    the ids of `pair_edges` and `targets` once per tensor)."""
    h_prot, hgcn_w, xe, h, probe = _f32c(h_prot), _f32c(hgcn_w).contiguous(), _f32c(xe), _f32c(h), _f32c(probe)
    basis1, att1, root1 = _f32c(layer1[0]).contiguous(), _f32c(layer1[1]), _f32c(layer1[2]).contiguous()
    basis2, att2, root2 = _f32c(layer2[0]).contiguous(), _f32c(layer2[1]), _f32c(layer2[2]).contiguous()
    pe_ptr, pe_src, pe_rel = pair_edges
    prot_ptr, prot_drug, inv_cnt = targets[:3]
    q_node = torch.as_tensor(q_node)
    require_device(h_prot, hgcn_w, xe, h, probe, basis1, att1, root1, basis2, att2, root2, pe_ptr, pe_src, pe_rel, prot_ptr,
                   prot_drug, inv_cnt, q_node)
    if h_prot.dim() != 2 or hgcn_w.dim() != 2 or xe.dim() != 2 or h.dim() != 2 or basis1.dim() != 3 or basis2.dim() != 3 or \
            att1.dim() != 2 or att2.dim() != 2 or hgcn_w.shape[0] != h_prot.shape[1] or xe.shape[0] != h.shape[0]:
        raise _lib.TipkError('protein_attribution: h_prot [P, p], hgcn_w [p, pd], xe [n, ne], h [n, d1] and two layers '
                             '(basis [B, d_in, d_out], att [R, B], root [d_in, d_out]) expected')
    n_prot, p = h_prot.shape
    pd, (n, ne), d1 = hgcn_w.shape[1], xe.shape, h.shape[1]
    n_bases, d0, d2 = basis1.shape[0], basis1.shape[1], basis2.shape[2]
    n_rel, k, cat = att1.shape[0], int(k), bool(cat)
    if d0 != (ne + pd if cat else ne) or (not cat and ne != pd) or tuple(basis1.shape) != (n_bases, d0, d1) or \
            tuple(basis2.shape) != (n_bases, d1, d2) or tuple(root1.shape) != (d0, d1) or tuple(root2.shape) != (d1, d2) or \
            tuple(att1.shape) != (n_rel, n_bases) or tuple(att2.shape) != (n_rel, n_bases):
        raise _lib.TipkError('protein_attribution: widths do not chain: ne %d, pd %d, cat %s, basis1 %s, root1 %s, att1 %s, '
                             'basis2 %s, root2 %s, att2 %s' % (ne, pd, cat, tuple(basis1.shape), tuple(root1.shape),
                                                                 tuple(att1.shape), tuple(basis2.shape), tuple(root2.shape),
                                                                 tuple(att2.shape)))
    if q_node.dim() != 1 or q_node.dtype.is_floating_point or probe.dim() != 2 or tuple(probe.shape) != (q_node.numel(), d2):
        raise _lib.TipkError('protein_attribution: q_node int [Q] and probe [Q, %d] expected, got %s %s and %s'
                             % (d2, q_node.dtype, tuple(q_node.shape), tuple(probe.shape)))
    if pe_ptr.dtype != torch.int64 or pe_src.dtype != torch.int32 or pe_rel.dtype != torch.int32 or pe_ptr.numel() != n + 1 or \
            pe_src.dim() != 1 or pe_src.shape != pe_rel.shape:
        raise _lib.TipkError('protein_attribution: pair_edges = (int64 [%d], int32 [E], int32 [E]) of in_edges_by_pair expected'
                             % (n + 1))
    if prot_ptr.dtype != torch.int64 or prot_drug.dtype != torch.int32 or inv_cnt.dtype != torch.float32 or \
            prot_ptr.numel() != n_prot + 1 or prot_drug.dim() != 1 or inv_cnt.numel() != n:
        raise _lib.TipkError('protein_attribution: targets = (int64 [%d], int32 [E], float32 [%d]) of targets_by_protein expected'
                             % (n_prot + 1, n))
    if not protein_attribution_supported(n, n_prot, n_rel, n_bases, ne, pd, p, d1, d2, cat, k):
        raise _lib.TipkError('protein_attribution: tipk_protein_attribution does not take n = %d, B = %d, widths (%d, %d, %d, '
                             '%d, %d), k = %d (include/tipk.h 4o)' % (n, n_bases, ne, pd, p, d1, d2, k))
    h_prot, xe, h, att1, att2, probe = (t if t.stride(0) >= t.shape[1] else t.contiguous()
                                        for t in (h_prot, xe, h, att1, att2, probe))
    _range_checked(pe_src, n, 'pair_edges source')
    _range_checked(pe_rel, n_rel, 'pair_edges relation')
    _range_checked(prot_drug, n, 'targets drug')
    dev, n_q = h.device, q_node.numel()
    pe_ptr, pe_src, pe_rel = pe_ptr.contiguous(), pe_src.contiguous(), pe_rel.contiguous()
    prot_ptr, prot_drug, inv_cnt = prot_ptr.contiguous(), prot_drug.contiguous(), inv_cnt.contiguous()
    qn = q_node.to(torch.int32).contiguous()
    contrib, protein = _topk_outputs(n_q, k, 1, dev)
    direct = torch.empty_like(contrib)
    features = torch.empty(n_q, dtype=torch.float32, device=dev)
    proteins = torch.empty(n_q, dtype=torch.float32, device=dev)
    ws_bytes = protein_attribution_workspace_bytes(n, n_bases, d1, p, n_q)
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=dev)
    check(lib().tipk_protein_attribution(ptr(h_prot), h_prot.stride(0), n_prot, p, ptr(hgcn_w), pd, ptr(xe), xe.stride(0), ne,
                                         ptr(h), h.stride(0), n, d1, ptr(basis1), ptr(att1), att1.stride(0), ptr(root1),
                                         ptr(basis2), ptr(att2), att2.stride(0), ptr(root2), d2, n_rel, n_bases, ptr(pe_ptr),
                                         ptr(pe_src), ptr(pe_rel), pe_src.numel(), ptr(prot_ptr), ptr(prot_drug),
                                         prot_drug.numel(), ptr(inv_cnt), int(cat), ptr(qn), ptr(probe), probe.stride(0), n_q,
                                         k, ptr(contrib), ptr(protein), ptr(direct), ptr(features), ptr(proteins), ptr(ws),
                                         stream_ptr(dev)), 'tipk_protein_attribution')
    return contrib, protein, direct, features, proteins


def drug_fold_in_supported(n_nodes, n_prot, n_rel, n_bases, ne, p, pd, d1, d2, cat):
    """Whether `drug_fold_in` takes these sizes (include/tipk.h section 4k)."""
    return bool(lib().tipk_drug_fold_in_supported(int(n_nodes), int(n_prot), int(n_rel), int(n_bases), int(ne), int(p), int(pd),
                                                  int(d1), int(d2), int(bool(cat))))


def drug_fold_in(h_prot, hgcn_w, x0, h1, layer1, layer2, xd, targets, interactions, cat):
    """x0, h1 and z rows of M drugs that are no node of the graph, from the frozen model's tables (include/tipk.h section 4k;
    one launch, no per-edge or [M, B d] temporary).

    h_prot [n_prot, p], x0 [N, d0], h1 [N, d1] (row strides free), hgcn_w [p, pd]; layer1 = (basis1 [B, d0, d1], att1 [R, B],
    root1 [d0, d1]), layer2 = (basis2 [B, d1, d2], att2 [R, B], root2 [d1, d2]); xd [M, ne]: fp32 device tensors; d0 = ne + pd
    with cat, else ne = pd = d0.  targets = (tgt_ptr int64 [M + 1], tgt_prot int32 [T]), interactions = (in_ptr int64
    [M + 1], in_src int32 [E], in_rel int32 [E]): CSR lists per new drug, on the device; each interaction is an in-edge from
    the existing drug in_src under relation in_rel, duplicates count.
    -> (x0_new [M, d0], h1_new [M, d1], z_new [M, d2]) float32.  Bitwise repeatable, row by row whatever else is in the call.
    Does not synchronise (a first call checks the ids of `targets` and `interactions` once per tensor: IndexError)."""
    basis1, att1, root1 = layer1
    basis2, att2, root2 = layer2
    h_prot, x0, h1, att1, att2, xd = _f32c(h_prot), _f32c(x0), _f32c(h1), _f32c(att1), _f32c(att2), _f32c(xd)
    hgcn_w, basis1, root1, basis2, root2 = (_f32c(t).contiguous() for t in (hgcn_w, basis1, root1, basis2, root2))
    tgt_ptr, tgt_prot = targets
    in_ptr, in_src, in_rel = interactions
    require_device(h_prot, hgcn_w, x0, h1, basis1, att1, root1, basis2, att2, root2, xd, tgt_ptr, tgt_prot, in_ptr, in_src, in_rel)
    if h_prot.dim() != 2 or hgcn_w.dim() != 2 or x0.dim() != 2 or h1.dim() != 2 or xd.dim() != 2 or \
            hgcn_w.shape[0] != h_prot.shape[1] or x0.shape[0] != h1.shape[0]:
        raise _lib.TipkError('drug_fold_in: h_prot [n_prot, p], hgcn_w [p, pd], x0 [N, d0], h1 [N, d1], xd [M, ne] expected, got '
                             '%s, %s, %s, %s, %s' % tuple(tuple(t.shape) for t in (h_prot, hgcn_w, x0, h1, xd)))
    (n_prot, p), pd, (n, d0), d1, (n_new, ne) = h_prot.shape, hgcn_w.shape[1], x0.shape, h1.shape[1], xd.shape
    cat = bool(cat)
    if d0 != (ne + pd if cat else ne) or (not cat and ne != pd):
        raise _lib.TipkError('drug_fold_in: d0 = ne + pd (cat) or d0 = ne = pd (add) expected, got d0 %d, ne %d, pd %d, cat %s'
                             % (d0, ne, pd, cat))
    if basis1.dim() != 3 or basis2.dim() != 3 or att1.dim() != 2 or tuple(basis1.shape[1:]) != (d0, d1) or \
            basis2.shape[:2] != (basis1.shape[0], d1) or tuple(root1.shape) != (d0, d1) or \
            tuple(root2.shape) != tuple(basis2.shape[1:]) or att1.shape[1] != basis1.shape[0] or att2.shape != att1.shape:
        raise _lib.TipkError('drug_fold_in: basis1 [B, %d, %d], att1 [R, B], root1 [%d, %d], basis2 [B, %d, d2], att2 [R, B], '
                             'root2 [%d, d2] expected, got %s, %s, %s, %s, %s, %s'
                             % ((d0, d1, d0, d1, d1, d1) + tuple(tuple(t.shape) for t in (basis1, att1, root1, basis2, att2, root2))))
    n_bases, d2, n_rel = basis1.shape[0], basis2.shape[2], att1.shape[0]
    if tgt_ptr.dtype != torch.int64 or tgt_prot.dtype != torch.int32 or tgt_ptr.numel() != n_new + 1 or tgt_prot.dim() != 1:
        raise _lib.TipkError('drug_fold_in: targets = (int64 [%d], int32 [T]) expected' % (n_new + 1))
    if in_ptr.dtype != torch.int64 or in_src.dtype != torch.int32 or in_rel.dtype != torch.int32 or \
            in_ptr.numel() != n_new + 1 or in_src.dim() != 1 or in_src.shape != in_rel.shape:
        raise _lib.TipkError('drug_fold_in: interactions = (int64 [%d], int32 [E], int32 [E]) expected' % (n_new + 1))
    if h_prot.stride(0) < p or x0.stride(0) < d0 or h1.stride(0) < d1 or att1.stride(0) < n_bases or att2.stride(0) < n_bases \
            or xd.stride(0) < ne:
        h_prot, x0, h1, att1, att2, xd = (t.contiguous() for t in (h_prot, x0, h1, att1, att2, xd))
    _range_checked(tgt_prot, n_prot, 'targets protein')
    _range_checked(in_src, n, 'interactions partner')
    _range_checked(in_rel, n_rel, 'interactions relation')
    dev = x0.device
    tgt_ptr, tgt_prot, in_ptr, in_src, in_rel = (t.contiguous() for t in (tgt_ptr, tgt_prot, in_ptr, in_src, in_rel))
    x0_new = torch.empty((n_new, d0), dtype=torch.float32, device=dev)
    h1_new = torch.empty((n_new, d1), dtype=torch.float32, device=dev)
    z_new = torch.empty((n_new, d2), dtype=torch.float32, device=dev)
    ws_bytes = int(lib().tipk_drug_fold_in_workspace_bytes(n, n_prot, n_rel, n_bases, ne, p, pd, d1, d2, int(cat), n_new,
                                                           in_src.numel()))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if ws_bytes > 0 else None
    check(lib().tipk_drug_fold_in(ptr(h_prot), h_prot.stride(0), n_prot, p, ptr(hgcn_w), pd, ptr(x0), x0.stride(0), ptr(h1),
                                  h1.stride(0), n, ptr(basis1), ptr(att1), att1.stride(0), ptr(root1), ptr(basis2), ptr(att2),
                                  att2.stride(0), ptr(root2), n_rel, n_bases, d1, d2, ptr(xd), max(xd.stride(0), ne), ne, int(cat),
                                  ptr(tgt_ptr), ptr(tgt_prot), tgt_prot.numel(), ptr(in_ptr), ptr(in_src), ptr(in_rel),
                                  in_src.numel(), n_new, ptr(x0_new), d0, ptr(h1_new), d1, ptr(z_new), d2, ptr(ws),
                                  stream_ptr(dev)), 'tipk_drug_fold_in')
    return x0_new, h1_new, z_new


_DET_WS = {}


def _det_workspace(device, n_nodes, k, n_rel):
    """Zeroed fixed-point workspace of the deterministic objective (one per device and shape; every
    call leaves it zeroed again, so it is allocated and cleared exactly once)."""
    key = (str(device), int(n_nodes), int(k), int(n_rel))
    ws = _DET_WS.get(key)
    if ws is None:
        n = int(lib().tipk_distmult_workspace_bytes(n_nodes, k, n_rel)) // 8
        ws = _DET_WS[key] = torch.zeros(n, dtype=torch.int64, device=device)
    return ws


def packed_pairs(edge_index, n_nodes):
    """int32 [E]: the pair (u, v) of every triple as ONE 32-bit word u | v << 16 (include/tipk.h section 4, idx_bytes = 2).
    Built once per tensor version (the positives of the path are static) and kept in the side table (`_facts`: it is
    derived data and must not travel with `torch.save(model)`)."""
    assert n_nodes <= 65535
    facts = _facts(edge_index)
    w = facts.get('packed')
    if w is None:
        w = (edge_index[0].to(torch.int64) | (edge_index[1].to(torch.int64) << 16))
        w = facts['packed'] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()
    return w


def unpack_pairs(packed):
    """int64 [2, E] from packed pairs (for callers that need the reference's form)."""
    w = packed.to(torch.int64) & 0xffffffff
    out = torch.stack([w & 0xffff, w >> 16])
    out._tipk_sampled = getattr(packed, '_tipk_sampled', False)
    return out


def distmult_loss(z, weight, pos_index, neg_index, edge_type, need_grad=True):
    """(loss [1], g_z, g_w) of the fused TIP objective (include/tipk.h section 4); bitwise reproducible
    (fixed-point cross-workgroup sums) unless TIPK_FLOAT_ATOMICS=1.
    neg_index: int64 / int32 [2, E] like pos_index, or the sampler's PACKED form (int32 [E], u | v << 16:
    `typed_negative_sampling(..., packed=True)`) -- the positives are then narrowed once to the same form and the kernel
    reads 8 bytes of ids per position instead of 32."""
    z, weight = _f32c(z).contiguous(), _f32c(weight).contiguous()
    require_device(z, weight, pos_index, neg_index, edge_type)
    validate_triples(pos_index, edge_type, z.shape[0], weight.shape[0])
    packed = bool(getattr(neg_index, '_tipk_packed_pairs', False))
    et = edge_type.contiguous()
    if packed:
        tasks = relation_tasks(et, pos_index)
        if (tasks is None or z.shape[1] not in (4, 8, 16) or switches.on('TIPK_FLOAT_ATOMICS') or z.shape[0] > 65535
                or neg_index.numel() != pos_index.shape[1]):
            neg_index, packed = unpack_pairs(neg_index).type_as(pos_index), False      # the general kernels take plain ids
    if packed and not getattr(neg_index, '_tipk_sampled', False):      # a packed tensor that is not the sampler's own output
        validate_triples(unpack_pairs(neg_index), None, z.shape[0], weight.shape[0])
    if packed:                                             # (`_store`: the finalize launch overwrites -- no zero fills)
        loss = torch.empty((1,), dtype=torch.float32, device=z.device)
        g_z = torch.empty_like(z) if need_grad else None
        g_w = torch.empty_like(weight) if need_grad else None
        pp = packed_pairs(pos_index, z.shape[0])
        ws = _det_workspace(z.device, z.shape[0], z.shape[1], weight.shape[0])
        st = lib().tipk_distmult_loss_store(ptr(z), z.shape[0], z.shape[1], ptr(weight), weight.shape[0], ptr(pp), None,
                                            ptr(neg_index), None, 2, ptr(et), _idx_bytes(et), pp.numel(),
                                            ptr(tasks), tasks.shape[0], ptr(loss), ptr(g_z), ptr(g_w), ptr(ws),
                                            stream_ptr(z.device))
        if st != -2:                                       # TIPK_EUNSUPPORTED: z does not fit the kernel's LDS image
            check(st, 'tipk_distmult_loss_store')
            return loss, g_z, g_w
        neg_index = unpack_pairs(neg_index).type_as(pos_index)
    if not getattr(neg_index, '_tipk_sampled', False):
        validate_triples(neg_index, None, z.shape[0], weight.shape[0])       # sampler output is in range by construction
    pu, pv = _uv(pos_index)
    nu, nv = _uv(neg_index)
    assert pu.dtype == nu.dtype and pu.numel() == nu.numel()
    tasks = relation_tasks(et, pos_index)
    ws = None if (tasks is None or switches.on('TIPK_FLOAT_ATOMICS')) else \
        _det_workspace(z.device, z.shape[0], z.shape[1], weight.shape[0])
    if ws is not None:                                     # deterministic path: its finalize launch overwrites the outputs
        loss = torch.empty((1,), dtype=torch.float32, device=z.device)
        g_z = torch.empty_like(z) if need_grad else None
        g_w = torch.empty_like(weight) if need_grad else None
        st = lib().tipk_distmult_loss_store(ptr(z), z.shape[0], z.shape[1], ptr(weight), weight.shape[0], ptr(pu), ptr(pv),
                                            ptr(nu), ptr(nv), _idx_bytes(pu), ptr(et), _idx_bytes(et), pu.numel(),
                                            ptr(tasks), tasks.shape[0], ptr(loss), ptr(g_z), ptr(g_w), ptr(ws),
                                            stream_ptr(z.device))
        if st != -2:
            check(st, 'tipk_distmult_loss_store')
            return loss, g_z, g_w
    loss = torch.zeros((1,), dtype=torch.float32, device=z.device)
    g_z = torch.zeros_like(z) if need_grad else None
    g_w = torch.zeros_like(weight) if need_grad else None
    check(lib().tipk_distmult_loss(ptr(z), z.shape[0], z.shape[1], ptr(weight), weight.shape[0], ptr(pu), ptr(pv),
                                   ptr(nu), ptr(nv), _idx_bytes(pu), ptr(et), _idx_bytes(et), pu.numel(),
                                   ptr(tasks), 0 if tasks is None else tasks.shape[0],
                                   ptr(loss), ptr(g_z), ptr(g_w), ptr(ws), stream_ptr(z.device)), 'tipk_distmult_loss')
    return loss, g_z, g_w


def typed_negative_sampling_device(pos_key_sorted, rel_ptr, n_rel, n_nodes, seed, n_positions, dtype=torch.int64,
                                   call_counter=None, wg=None, pos_offset=None, packed=False, keys32=None, out=None):
    """pos_offset: optional int64 device tensor [n_rel]: Philox counter of position e of relation r = e + pos_offset[r]
    (relation-sharded runs: the position's number in the whole triple list).
    call_counter: optional int64 device tensor [2] = {position, seed} (the stream's state): the
    Philox key is derived on the device from it, `seed` is ignored, and the position is advanced by
    one afterwards.
    out: optional preallocated result on the device -- int32 [n_positions] (packed), or `dtype` [2, n_positions] whose two
    rows are contiguous; every position is written."""
    require_device(pos_key_sorted, rel_ptr, call_counter, out)
    dev = pos_key_sorted.device
    if out is not None:
        shape = (n_positions,) if packed else (2, n_positions)
        if (tuple(out.shape) != shape or out.dtype != (torch.int32 if packed else dtype) or out.device != dev
                or out.stride()[-1] != 1):
            raise ValueError('out must be a %s %s tensor on %s with unit stride along positions'
                             % (torch.int32 if packed else dtype, shape, dev))
    st = stream_ptr(dev)
    wg_ptr, wg_units = wg if (wg is not None and not switches.on('TIPK_NO_BITMAP')) else (None, None)
    # a stream state with a ticket word {position, seed, ticket}: the sampling launch moves the position on itself
    adv = 1 if (call_counter is not None and call_counter.numel() >= 3 and n_positions > 0 and n_rel > 0) else 0
    if packed:                                     # one 32-bit word u | v << 16 per position (same draws, same pairs)
        assert n_nodes <= 65535
        if out is None:
            out = torch.empty((n_positions,), dtype=torch.int32, device=dev)
        check(lib().tipk_typed_negative_sampling(ptr(pos_key_sorted), ptr(rel_ptr), n_rel, n_nodes, seed, ptr(call_counter), adv,
                                                 ptr(wg_ptr), ptr(wg_units), 0 if wg_ptr is None else wg_ptr.numel() - 1,
                                                 ptr(pos_offset), ptr(keys32), ptr(out), None, 2, n_positions, st),
              'tipk_typed_negative_sampling')
        out._tipk_packed_pairs = True
    else:
        if out is None:
            out = torch.empty((2, n_positions), dtype=dtype, device=dev)
        check(lib().tipk_typed_negative_sampling(ptr(pos_key_sorted), ptr(rel_ptr), n_rel, n_nodes, seed,
                                                 ptr(call_counter), adv, ptr(wg_ptr), ptr(wg_units),
                                                 0 if wg_ptr is None else wg_ptr.numel() - 1, ptr(pos_offset), ptr(keys32), ptr(out[0]), ptr(out[1]),
                                                 8 if dtype == torch.int64 else 4, n_positions, st),
              'tipk_typed_negative_sampling')
    if call_counter is not None and not adv:
        check(lib().tipk_counter_advance(ptr(call_counter), st), 'tipk_counter_advance')
    out._tipk_sampled = True                       # ids < n_nodes by construction: no range check downstream
    return out


# ---------------------------------------------------------------------------------------------
# static graph containers (plans in both directions + normalisers)
# ---------------------------------------------------------------------------------------------
PAIR_FWD_MAX_WORLD = 4   # fallback rule when the forward routes cannot be timed (first call under capture): >= 4 ranks -> Y route
PAIR_KGROUP = 8          # source nodes whose products are summed inside one wavefront of the pair-form product


def pair_product(cells, xb_nb, symmetric=False, links=None, zeros=None, xbt=None):
    """slabs[g] = sum_{u in group g} cells[u] (N x bases) @ xb_nb[u] (bases x out)  (include/tipk.h section 2c):
    cells [N_pad, N, bases], xb_nb [N_pad, bases, out] -- or a column slice [..., :out] of a buffer whose rows are
    padded to 32 columns with zeros (what the dedicated kernel reads) -> [N_pad / PAIR_KGROUP, N, out].
    links (optional, uint32 [N_pad, ceil(N / 32)] as int32): bit r of word (u, t) = pair (u, 32 t + r) is linked; the cells of the
    other pairs are not read (they are zero).
    xbt (optional, [N, out, bases] contiguous): filled with XB of the N nodes, bases innermost (`node_products` reads it)."""
    n_pad, n, nb = cells.shape
    d = xb_nb.shape[2]
    assert xbt is None or (tuple(xbt.shape) == (n, d, nb) and xbt.is_contiguous() and xbt.dtype == torch.float32)
    assert cells.is_contiguous() and xb_nb.shape[:2] == (n_pad, nb) and n_pad % PAIR_KGROUP == 0
    padded = xb_nb.stride() == (nb * 32, 32, 1) and d <= 32
    if pair_product_on_gemm(nb, d, symmetric, padded):
        job = gemm_job(cells, xb_nb, reduce_batch=True, kgroup=PAIR_KGROUP)      # same sums on the tiled GEMM
        with _timed('gemm[%s]' % job.label):
            check(lib().tipk_gemm_f32(job.desc, stream_ptr(cells.device)), 'tipk_gemm_f32')
        if xbt is not None:
            xbt.copy_(xb_nb[:n].permute(0, 2, 1))
        return job.slabs
    assert padded, 'tipk_pair_product reads XB rows padded to 32 columns (AggGraph.pair_buffers)'
    slabs = torch.empty((n_pad // PAIR_KGROUP, n, d), dtype=torch.float32, device=cells.device)
    with _timed('pair_product[%dx%dx%dx%d]' % (n_pad, n, nb, d)):
        check(lib().tipk_pair_product(ptr(cells), ptr(xb_nb), n_pad, n, nb, d, PAIR_KGROUP, int(symmetric), ptr(links), ptr(zeros),
                                      ptr(xbt), ptr(slabs), stream_ptr(cells.device)), 'tipk_pair_product')
    return slabs


def _lazy_plan(name):
    """Property of a plan that may be given as a zero-argument callable: it is called once, on first read."""
    slot = '_' + name

    def get(self):
        plan = getattr(self, slot)
        if callable(plan):
            plan = plan()
            setattr(self, slot, plan)
        return plan
    return property(get)


class AggGraph(object):
    """fwd: out rows <- table rows;  bwd: the transpose.  scale = per-out-row factor (1/deg)."""
    fwd, bwd, csr_bwd, rl_fwd, rl_bwd, rs_bwd, pair_bwd, dest_fwd, row_fwd, row_bwd = (
        _lazy_plan(name) for name in ('fwd', 'bwd', 'csr_bwd', 'rl_fwd', 'rl_bwd', 'rs_bwd', 'pair_bwd', 'dest_fwd', 'row_fwd', 'row_bwd'))

    def __init__(self, fwd, bwd, scale=None, rl_fwd=None, rl_bwd=None, bwd_scaled=False, csr_bwd=None, rs_bwd=None,
                 pair_fwd=None, pair_bwd=None, dest_fwd=None, row_fwd=None, row_bwd=None, row_wave_uniform=False):
        """fwd / bwd: GatherPlans, or zero-argument callables that build them on first use (the
        generic D-D plans are only needed where the relation-local kernel does not apply).
        csr_bwd: optional callable -> CsrPlan of the transposed pass (every row written, rows short)."""
        self._fwd, self._bwd, self.scale = fwd, bwd, scale
        self._csr_bwd = csr_bwd
        self._rl_fwd, self._rl_bwd = rl_fwd, rl_bwd        # relation-local (LDS) plans of a D-D graph: plans, or callables
                                                           # that build them on first use (fallback routes only)
        self._rs_bwd = rs_bwd                              # wave-stream plan of the transposed pass (LDS-resident g'), or a
                                                           # callable that builds it on first use (the pair-form backward
                                                           # pass never needs it)
        self.pair_fwd = pair_fwd                           # wave-stream plan of the forward pass in pair form (LDS-resident att)
        self._pair_bwd = pair_bwd                          # plan.PairBwdPlan of the pair-form backward pass (or a callable)
        self._dest_fwd = dest_fwd                          # plan.DestPlan of the forward pass of large graphs (or a callable)
        self._row_fwd, self._row_bwd = row_fwd, row_bwd    # plan.RowStreamPlans of large graphs (rows by destination / by
                                                           # source), or callables: tipk_rgcn_row_products
        self.has_row_plans = row_fwd is not None and row_bwd is not None
        self.row_plans_wave_uniform = bool(row_wave_uniform)   # plan.RowStreamPlanS (widths % 64 == 0) | plan.RowStreamPlan
        self.pair_stamp = 0                                # bumped by every pass that rewrites the pair buffers
        self._pair_cells = {}                              # persistent cell / XB buffers of the pair form, zeroed once
        self.bwd_scaled = bwd_scaled                       # bwd plan's edge weights already carry `scale`
        self.fwd_route = {}                                # sharded layers: timed choice pair form | Y route (ops._fwd_route)

    def pair_buffers(self, n, nb, d_out, device):
        """(cells C[u, v, b] as [N_pad, N, bases], XB as [N_pad, bases, out] -- a column slice of rows padded to 32)
        of the pair-form forward, N_pad = N
        rounded up to PAIR_KGROUP.  Allocated and zeroed ONCE: every call rewrites the cells of the linked drug
        pairs and the first N blocks of XB; nothing ever touches the rest."""
        key = (int(n), int(nb), int(d_out), str(device))
        buf = self._pair_cells.get(key)
        if buf is None:
            n_pad = -(-n // PAIR_KGROUP) * PAIR_KGROUP
            xb_pad = torch.zeros((n_pad, nb, 32 if d_out <= 32 else d_out), dtype=torch.float32, device=device)
            flat = torch.zeros(n_pad * n * nb + 64, dtype=torch.float32, device=device)     # (+ a block of zeros behind the cells)
            buf = self._pair_cells[key] = (flat[:n_pad * n * nb].view(n_pad, n, nb),
                                           xb_pad[:, :, :d_out],           # rows padded to 32 columns: the product kernel's layout
                                           flat[n_pad * n * nb:])
        return buf

    def xbt_buffer(self, n, nb, d_out, device):
        """XB a second time as [N, out, bases] -- what the d att product of the backward pass reads (`node_products`): a
        column of all bases is one 128-byte line there (it is 32 lines in the node-major buffer of the pair product)."""
        key = ('xbt', int(n), int(nb), int(d_out), str(device))
        buf = self._pair_cells.get(key)
        if buf is None:
            buf = self._pair_cells[key] = torch.empty((n, d_out, nb), dtype=torch.float32, device=device)
        return buf


# ---------------------------------------------------------------------------------------------
# autograd Functions
# ---------------------------------------------------------------------------------------------
class _Aggregate(torch.autograd.Function):
    """out = scale * (A table) + bias, optional fused ReLU; grad: A^T (scale * g)."""

    @staticmethod
    def forward(ctx, table, bias, graph, relu):
        out = gather_sum(graph.fwd, table, row_scale=graph.scale, bias=bias, relu=relu)
        ctx.graph, ctx.relu, ctx.has_bias = graph, relu, bias is not None
        ctx.save_for_backward(out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        graph = ctx.graph
        g = _f32c(g)
        # pre = scale * agg + bias, out = relu(pre):  g_pre = g (.) [out > 0];  g_agg = scale * g_pre
        g_pre = rows_affine(g, gate=out) if ctx.relu else g
        g_bias = None
        if ctx.has_bias:
            g_bias = col_sum(g_pre)
        g_agg = g_pre
        if graph.scale is not None and not graph.bwd_scaled:
            g_agg = rows_affine(g_pre, row_mul=graph.scale)
        g_table = gather_sum(graph.bwd, g_agg) if ctx.needs_input_grad[0] else None
        return g_table, g_bias, None, None


def aggregate(table, graph, bias=None, relu=False):
    return _Aggregate.apply(table, bias, graph, relu)


class _Linear(torch.autograd.Function):
    """y = x @ W^T with W [out, in] (the `lin` of GCNConv); x=None means identity features."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.identity = x is None
        if x is None:
            ctx.save_for_backward(weight)
            return transpose(weight)
        x = _f32c(x)
        ctx.save_for_backward(x, weight)
        return gemm(x, weight.t())

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g)
        if ctx.identity:
            (weight,) = ctx.saved_tensors
            return None, (g.contiguous().t() if weight.t().is_contiguous() else transpose(g))
        x, weight = ctx.saved_tensors
        jobs = [gemm_job(g.t(), x)]
        if ctx.needs_input_grad[0]:
            jobs.append(gemm_job(g, weight))
        outs = gemm_group(jobs)                                          # d W and d x: one grouped launch
        return (outs[1] if len(outs) > 1 else None), outs[0]


def linear_t(x, weight):
    return _Linear.apply(x, weight)


class _MatMul(torch.autograd.Function):
    """y = x @ w  (plain dense product on the matrix cores)."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = _f32c(x), _f32c(w)
        ctx.save_for_backward(x, w)
        return gemm(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = _f32c(g)
        j_w = gemm_job(x.t(), g) if ctx.needs_input_grad[1] else None
        j_x = gemm_job(g, w.t()) if ctx.needs_input_grad[0] else None
        gemm_group([j for j in (j_w, j_x) if j is not None])
        return (j_x.out if j_x else None), (j_w.out if j_w else None)


def matmul(x, w):
    return _MatMul.apply(x, w)


FWD_ROUTE_MODE = os.environ.get('TIPK_FWD_ROUTE', 'rule')     # 'rule' | 'pair' | 'y' | 'timed' (bench.py sets 'timed' for sharded runs)


def _fwd_route(graph, x, basis, att, pair, shard):
    """'pair' | 'y': the forward route of a relation-SHARDED layer.  The two routes give the same partial aggregate up to
    ROUNDING, so the choice must not depend on anything that varies from run to run or from rank to rank:

      'rule'   (default) the rule of thumb from the 1-GPU timings: PAIR_FWD_MAX_WORLD ranks or more -> Y route;
      'pair' / 'y'       pinned (parity runs);
      'timed'  both routes are timed once per (graph, layer width) on this rank's relations -- HIP events on the launch
               stream, 3 runs each after a warm-up -- the times are SUMMED OVER THE RANKS (one all-reduce of two floats) and
               every rank takes the route with the smaller sum: one decision for the whole job, recorded on the graph
               (bench.py prints it as `config.forward_routes`).  A first call under graph capture cannot time anything and
               uses the rule.

    EVERY rank of a sharded layer calls this, with pair = None when it cannot take the pair form itself (no relations, an
    att table beyond the LDS, a plan of another shape): in 'timed' mode the all-reduce below is part of the layer's
    collective sequence, so whether it happens must not depend on a rank's own shard -- such a rank adds +inf to the pair
    form's sum (the job takes the Y route) and the time of its own Y route (0 without relations)."""
    n = x.shape[0]
    nb, _, d_out = basis.shape
    r = att.shape[0]
    key = (int(n), int(nb), int(d_out))
    hit = graph.fwd_route.get(key)
    if hit is not None:
        return hit[0] if pair is not None else 'y'
    mode = FWD_ROUTE_MODE
    if mode in ('pair', 'y'):
        return mode if pair is not None else 'y'
    rule = 'y' if shard.world >= PAIR_FWD_MAX_WORLD else 'pair'
    if mode != 'timed' or torch.cuda.is_current_stream_capturing() or _TIMING is not None:
        return rule if pair is not None else 'y'
    with torch.no_grad():
        routes = []
        if r > 0:
            xb = gemm(x, basis)
            use_rl = rel_gather_usable(graph.rl_fwd, n, d_out, False)

            def y_route():
                y = gemm(att, xb.view(nb, n * d_out)).view(r * n, d_out)
                return sum_slabs(rel_gather(graph.rl_fwd, y, backward=False, reduce=False)) if use_rl else gather_sum(graph.fwd, y)
            routes.append(('y', y_route))
        if pair is not None:
            cells, xb_nb, _ = graph.pair_buffers(n, nb, d_out, x.device)
            gemm(x, basis, out=xb_nb[:n].permute(1, 0, 2))
            graph.pair_stamp += 1                                 # (the pair buffers are rewritten here)

            def pair_route():
                stream_gather(pair, att, write_zeros=False, out=cells.view(-1, nb)[:n * n], label='pair_cells[dd.fwd]', kind=1)
                return sum_slabs(pair_product(cells, xb_nb, symmetric=pair.symmetric).view(-1, n, d_out))
            routes.append(('pair', pair_route))
        times = {'pair': float('inf'), 'y': 0.0}
        for name, fn in routes:
            fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(3):
                fn()
            b.record()
            torch.cuda.synchronize(x.device)
            times[name] = a.elapsed_time(b) / 3 * 1e3
        total = torch.tensor([min(times['pair'], 1e30), times['y']], dtype=torch.float32, device=x.device)
        shard.all_reduce(total)                                   # the same two sums on every rank -> the same decision
        total = total.tolist()
    choice = 'pair' if total[0] <= total[1] else 'y'
    graph.fwd_route[key] = (choice, times, {'pair': total[0], 'y': total[1]})
    return choice if pair is not None else 'y'


# What `rgcn_route` decides for one pass through an R-GCN layer:
#   fwd        'pair_sym' | 'pair_dir' | 'pair_gemm' (pair form: cells of att rows, then `tipk_pair_product` on half / all the cells,
#              or the tiled GEMM), 'rows' | 'dest' (large graphs: `row_products` / `dest_products`), 'rel_gather' | 'Y' (Y = att . XB,
#              then the LDS-resident gather or `gather_sum`)
#   pair       the pair plan (`graph.pair_fwd`) of a pair-form pass, else None
#   pair_bwd   the backward pass is the pair form as well (`pair_grads` on the cells and XB the forward pass leaves with the graph)
#   xb         where XB of the forward pass lives: 'graph' (the graph's node-major buffer, stamped), 'graph+xbt' (the same, and a
#              second copy [N, out, bases] for `node_products`), 'own' (a tensor saved for the backward pass)
#   handover   this layer can finish a pending slab sum of its input in the launch of its own XB (`sum_slabs_xb`)
#   cells_two  this layer's cell launch can gather the cells of `partner` (the next layer) too (`stream_gather_two`)
RgcnRoute = collections.namedtuple('RgcnRoute', 'fwd pair pair_bwd xb handover cells_two')


def pair_product_on_gemm(nb, d, symmetric, padded):
    """True where `pair_product` runs on the tiled GEMM instead of `tipk_pair_product` (only the kernel reads mirrored cells)."""
    return (not lib().tipk_pair_product_supported(nb, d) or switches.on('TIPK_NO_PAIR_PRODUCT') or not padded) and not symmetric


def rgcn_route(graph, n, d_in, d_out, nb, r, shard=None, need_grad=True, operands=None, partner=None):
    """-> RgcnRoute: THE route decision of an R-GCN layer [n, d_in] -> [n, d_out] with `nb` bases and `r` relations on `graph`,
    from plan attributes, switches and the library's `tipk_*_supported` queries alone (no device needed, nothing launched).
    `_RGCN.forward` asks once per pass and keeps the answer on its ctx; `encoder.usable` asks the same function.

    operands = (x, basis, att): needed by a relation-sharded layer (`_fwd_route`: in 'timed' mode it times both routes and
    holds a collective every rank must reach) and with `partner` = (att, graph, d_out[, token]) of the next layer.
    Plans are built on first use: a lazy plan is only read where the route that is being chosen needs it."""
    pair = graph.pair_fwd if r > 0 else None
    if pair is not None and pair.symmetric and not lib().tipk_pair_product_supported(nb, d_out):
        pair = None                                          # only the dedicated product kernel reads mirrored cells
    split = stream_gather_split(r, nb) if pair is not None else 0
    if pair is not None and not (pair.n_table == r and pair.n_rows == n * n and split and (nb // split) // 4 == pair.lanes):
        pair = None
    if shard is not None and shard.world > 1:
        # the pair form's dense product reads the whole N x N cell matrix on EVERY rank (16 us at BioSNAP, whatever
        # the rank's share of the relations); the Y route (Y = att . XB + unit gather) scales with the share.  One
        # decision for the whole job, the same from run to run unless timing is asked for; every rank asks, whether or
        # not it could take the pair form itself (`_fwd_route`: the timed mode's all-reduce is a collective)
        if _fwd_route(graph, operands[0], operands[1], operands[2], pair, shard) == 'y':
            pair = None
    if pair is not None:
        pair_bwd = bool(need_grad and pair_grads_supported(nb, d_out) and graph.pair_bwd is not None)
        # (the stream plan of the transposed pass is only read where the backward pass is not the pair form)
        rs = None if (pair_bwd or not need_grad) else graph.rs_bwd
        xb = 'graph' if pair_bwd else ('graph+xbt' if (rs is not None and rs.compact is not None) else 'own')
        on_gemm = pair_product_on_gemm(nb, d_out, pair.symmetric, d_out <= 32)      # (`pair_buffers` pads rows of <= 32 columns)
        two = partner is not None and shard is None and pair_cells_partner_ok(graph, operands[2], partner[1], partner[0], n)
        return RgcnRoute('pair_gemm' if on_gemm else ('pair_sym' if pair.symmetric else 'pair_dir'), pair, pair_bwd, xb,
                         pair_bwd and shard is None and sum_slabs_xb_supported(d_in, d_out), two)
    fwd, plan = 'Y', None
    if r > 0:
        if rel_gather_split(n, d_out, False) > 0 and graph.rl_fwd is not None:      # (the unit plan is built here, on first use)
            fwd, plan = 'rel_gather', graph.rl_fwd
        # LARGE node sets (round 5; include/tipk.h sections 2h / 2f): Y = att . XB [R N, out] is never formed -- the (relation,
        # node) row sums are multiplied where they are assembled, or per destination T[:, v, :] = sum_e att[r_e, :]^T (x) X[src_e]
        elif _row_plan(graph, False, n, r, nb, d_in) is not None:
            fwd, plan = 'rows', graph.row_fwd
        elif graph.dest_fwd is not None:
            fwd, plan = 'dest', graph.dest_fwd
        if plan is not None:
            assert plan.n_nodes == n and plan.n_rel == r, 'graph/plan mismatch'
        else:                                                                       # (the generic plan is built here, on first use)
            assert graph.fwd.n_out == n and graph.fwd.n_table == r * n, 'graph/plan mismatch'
    return RgcnRoute(fwd, None, False, 'own', False, False)


def _take_pending(x, handover):
    """x may be the output of the previous layer with its final slab sum still PENDING (`defer_output`): the consumer then
    finishes it in the launch that computes its own XB / X root (`sum_slabs_xb`; the pending sum is returned), or -- on any
    other route -- right here (None is returned)."""
    pend = x.__dict__.pop('_tipk_pending', None) if hasattr(x, '__dict__') else None
    if pend is not None and not handover:
        slabs, scale, addend, relu = pend
        sum_slabs(slabs, out=x, row_scale=scale, addend=addend, relu=relu)
        pend = None
    return pend


def _cells_from_partner(graph, cells_token):
    """True if the previous layer gathered this layer's cells in THIS pass.  The token is an OBJECT the caller made for this
    forward pass and handed to both layers (FMEncoder.forward) -- not a (pointer, version) pair, which a raw-pointer parameter
    update (tipk_adam_step does not bump `_version`) would leave looking current."""
    tok = getattr(graph, 'cells_token', None)
    graph.cells_token = None
    return cells_token is not None and tok is not None and tok[0] is cells_token and tok[1] == graph.pair_stamp - 1


def _finish_agg(agg, graph, shard, xroot, relu):
    """out = relu?(agg / deg + X root), after the all-reduce of a shard's partial aggregate."""
    if shard is not None:
        shard.all_reduce(agg)
    return sum_slabs(agg.view(1, *agg.shape), row_scale=graph.scale, addend=xroot, relu=bool(relu))


def _rgcn_fwd_pair(route, x, basis, att, root, graph, shard, relu, pend, defer, partner, cells_token):
    """The pair form: cells of att rows per linked (source, destination) pair, one dense product, the ordered slab sum."""
    # sum_r A_r X W_r = sum_{(u -> v)} sum_b C[v, u, b] XB_b[u],  C[v, u, :] = sum of att[r, :] over the relations r that link
    # u -> v.  A BioSNAP drug pair is linked by 66 relations on average, so the per-EDGE work shrinks to adding one att row
    # (LDS-resident for the whole launch: a wave-stream gather like the transposed pass) and the per-PAIR work is one dense
    # product -- Y = att . XB [R N, out] (91 MB written and gathered back at layer 1) is never formed.
    # cells are kept SOURCE-major, C[u, v, :]: the product  sum_u C[u] (N x bases) . XB[u] (bases x out)  then reads
    # 16 KB contiguous per operand tile (destination-major cells made every tile 128 separate 128-byte rows:
    # 2.5 TB/s); the u range is padded to a multiple of PAIR_KGROUP with cells / XB rows that stay zero
    pair = route.pair
    n = x.shape[0]
    nb, _, d_out = basis.shape
    cells, xb_nb, zeros = graph.pair_buffers(n, nb, d_out, x.device)
    xb = xbt = None
    if pend is not None:                                 # x itself + XB + X root in ONE launch (layer hand-over)
        xroot = sum_slabs_xb(pend[0], pend[1], pend[2], pend[3], x, basis, root, xb_nb)
    elif route.xb == 'own':
        xb, _, xroot = gemm_group([gemm_job(x, basis), gemm_job(x, basis, out=xb_nb[:n].permute(1, 0, 2)), gemm_job(x, root)])
    else:
        # XB is computed ONCE, into the node-major buffer the pair product reads; the backward pass (`pair_grads`, or
        # `node_products` on the compact dY: a node's 32 rows are one 4-KB block there) takes the same buffer.  It belongs to
        # the graph and the next forward pass rewrites it: the stamp tells a backward pass that runs after ANOTHER forward
        # to recompute XB instead of reading someone else's
        _, xroot = gemm_group([gemm_job(x, basis, out=xb_nb[:n].permute(1, 0, 2)), gemm_job(x, root)])
        if route.xb == 'graph+xbt':
            # ... and the pair product, which stages every node's XB block in LDS anyway, writes it back a second time as
            # [N, out, bases]: what the d att product of the backward pass reads (`node_products` xbt)
            xbt = graph.xbt_buffer(n, nb, d_out, x.device)
    if _cells_from_partner(graph, cells_token):
        pass                                             # this layer's cells were gathered with the previous layer's (below)
    elif route.cells_two:
        # the cells depend on the parameters only: the NEXT layer's (same graph, its own att) are gathered in this
        # launch too -- one launch ramp and one tail instead of two.  The partner's buffers are rewritten: its stamp
        # moves on, and it is told for which token and stamp its cells are current
        att2, g2, d_out2 = partner[0].contiguous(), partner[1], partner[2]
        cells2 = g2.pair_buffers(n, nb, d_out2, x.device)[0]
        stream_gather_two(pair, att, att2, cells.view(-1, nb)[:n * n], cells2.view(-1, nb)[:n * n])
        g2.pair_stamp += 1
        g2.cells_token = (partner[3] if len(partner) > 3 else None, g2.pair_stamp)
    else:
        stream_gather(pair, att, write_zeros=False, out=cells.view(-1, nb)[:n * n], label='pair_cells[dd.fwd]', kind=1)
    slabs = pair_product(cells, xb_nb, symmetric=pair.symmetric, links=getattr(pair, 'links', None), zeros=zeros, xbt=xbt)
    slabs = slabs.view(-1, n, d_out)
    if defer:
        # the ordered slab sum is left to the ONE consumer of this output (the next R-GCN layer, which runs it in the
        # launch of its own XB product): until then `out` is storage only
        out = torch.empty((n, d_out), dtype=torch.float32, device=x.device)
        out._tipk_pending = (slabs, graph.scale, xroot, True)
    elif shard is None:
        out = sum_slabs(slabs, row_scale=graph.scale, addend=xroot, relu=bool(relu))
    else:
        out = _finish_agg(sum_slabs(slabs), graph, shard, xroot, relu)
    return out, xb


def _rgcn_fwd_large(route, x, basis, att, root, graph, shard, relu):
    """LARGE node sets: T_b = the att-weighted row sums of X, by (relation, destination) row or per destination, then
    sum_b T_b basis_b (row sums first: 0.16 TFLOP per layer at config 5 instead of the 0.41 of the per-edge product)."""
    n = x.shape[0]
    nb = basis.shape[0]
    xb, xroot = gemm_group([gemm_job(x, basis), gemm_job(x, root)])      # XB and X root: one grouped launch
    t_b = row_products(graph.row_fwd, x, att) if route.fwd == 'rows' else dest_products(graph.dest_fwd, x, att)
    agg = gemm(t_b, basis, reduce_batch=True, kgroup=large_kgroup(n, nb))
    return _finish_agg(agg, graph, shard, xroot, relu), xb


def _rgcn_fwd_y(route, x, basis, att, root, graph, shard, relu):
    """Y = att . XB [R N, out], then one gather-sum over its rows: the LDS-resident `rel_gather` or the generic `gather_sum`."""
    n = x.shape[0]
    nb, _, d_out = basis.shape
    r = att.shape[0]
    xb, xroot = gemm_group([gemm_job(x, basis), gemm_job(x, root)])      # XB and X root: one grouped launch
    y = gemm(att, xb.view(nb, n * d_out)).view(r * n, d_out) if r > 0 else None
    if route.fwd == 'rel_gather':
        # LDS-resident gather -> per-workgroup partial slabs; unsharded, the ordered slab sum also applies
        # 1/deg, adds X root and the ReLU: the layer is finished in one pass
        part = rel_gather(graph.rl_fwd, y, backward=False, reduce=False)
        if shard is None:
            return sum_slabs(part, row_scale=graph.scale, addend=xroot, relu=bool(relu)), xb
        agg = sum_slabs(part)
    elif shard is None:
        agg = gather_sum(graph.fwd, y, row_scale=graph.scale)
        return sum_slabs(agg.view(1, n, d_out), addend=xroot, relu=bool(relu)), xb
    elif r == 0:
        agg = torch.zeros((n, d_out), dtype=torch.float32, device=x.device)
    else:
        agg = gather_sum(graph.fwd, y)
    # partial aggregate of this rank's relations -> one all-reduce -> 1/deg(global), + X root, ReLU
    return _finish_agg(agg, graph, shard, xroot, relu), xb


def _rgcn_grad_att_xb(ctx, x, basis, att, xb, g):
    """(d att, dXB [bases, N, out]) of the pass `ctx` describes; d att is the finished tensor, or a slab job whose ordered sum
    rides in the dense tail's grouped slab sum.  What depends on the state the backward pass finds -- the graph's stamp, the
    layout of the operands -- is decided here."""
    graph = ctx.graph
    n = x.shape[0]
    nb, _, d_out = basis.shape
    r = att.shape[0]
    if r == 0:
        return (torch.zeros((0, nb), dtype=torch.float32, device=x.device),
                torch.zeros((nb, n, d_out), dtype=torch.float32, device=x.device))
    xbt = None
    if ctx.route.pair_bwd:
        cells, xb_nb, _ = graph.pair_buffers(n, nb, d_out, x.device)
        if graph.pair_stamp != ctx.xb_stamp:
            # another forward pass has rewritten the graph's buffers: the same values again -- and a new stamp, so that
            # THAT pass's backward pass recomputes its own as well
            gemm(x, basis, out=xb_nb[:n].permute(1, 0, 2))
            stream_gather(graph.pair_fwd, att, write_zeros=False, out=cells.view(-1, nb)[:n * n], label='pair_cells[dd.fwd]', kind=1)
            graph.pair_stamp += 1
            ctx.xb_stamp = graph.pair_stamp
        return pair_backward(graph.pair_bwd, cells, xb_nb, g)
    if ctx.xb_stamp is not None:                                     # XB lives in the graph's node-major buffer (forward)
        if graph.pair_stamp == ctx.xb_stamp:
            xb = graph.pair_buffers(n, nb, d_out, x.device)[1][:n].permute(1, 0, 2)
            xbt = graph.xbt_buffer(n, nb, d_out, x.device)
        else:                                                        # another forward pass has rewritten it: same values again
            xb = gemm(x, basis)
    xb2 = xb.view(nb, n * d_out) if xb.is_contiguous() else None
    rs = graph.rs_bwd
    used = None
    if rs is not None and rs.compact is not None:
        assert rel_stream_split(n, d_out) and (d_out // rel_stream_split(n, d_out)) // 4 == rs.lanes and rs.n_rel == r
        # dY_r = A_r^T (D^-1 g) in COMPACT node-major form: only the (relation, source) rows that have an edge
        # exist; both products of dY run on that form (d XB complete, d att as a few small slabs)
        dyc = rel_stream_bwd(rs, g, row_scale=graph.scale)
        return node_products(dyc, rs.compact, att, xb, xbt)
    if rs is not None and rel_stream_split(n, d_out) and (d_out // rel_stream_split(n, d_out)) // 4 == rs.lanes:
        # dY_r = A_r^T (D^-1 g), 1/deg fused.  Rows (relation, node) without edges -- half of them -- are
        # neither written here nor read as data by the fused products (row mask)
        masked = dy_products_fused(r, n * d_out, nb) and xb.stride(-1) == 1
        g_y = rel_stream_bwd(rs, g, row_scale=graph.scale, write_zeros=not masked)
        used = rs.row_used if masked else None
    elif rel_gather_usable(graph.rl_bwd, n, d_out, True):
        g_y = rel_gather(graph.rl_bwd, g, backward=True, row_scale=graph.scale)
    elif xb2 is not None and n * d_out * 4 < 2 ** 31 and _row_plan(graph, True, n, r, nb, d_out) is not None:
        # LARGE node sets: dY = A_r^T (D^-1 g') is never written -- its rows are summed in LDS and multiplied there
        gs = rows_affine(g, row_mul=graph.scale)
        j_rows, g_xb = row_products(graph.row_bwd, gs, att, xb2)
        gemm_group([], [j_rows])                                     # (thousands of slabs: a slab sum of its own, as dy_products')
        return j_rows.out, g_xb
    else:
        gs = rows_affine(g, row_mul=graph.scale)
        csr = graph.csr_bwd if (d_out % 4 == 0 and 8 <= d_out <= 256 and gs.numel() * 4 < 2 ** 32) else None   # (32-bit row offsets)
        # R N short rows: contiguous streams, no descriptors -- else the generic transposed gather
        g_y = gather_rows_csr(csr, gs) if csr is not None else gather_sum(graph.bwd, gs)
    # both consumers of dY in one pass over it (+ one grouped slab sum)
    g_att, g_xb = dy_products(g_y.view(r, n * d_out), att, xb2, used, n)
    return g_att, g_xb.view(nb, n, d_out)


def rgcn_dense_tail(x, basis, root, g, g_xb, gate_x, slab_jobs, shard=None):
    """(dX, d basis, d root) of an R-GCN layer given dXB [bases, N, d_out] and g [N, d_out] (1/deg not applied to the root
    term); gate_x: dX is masked with (gate_x > 0); slab_jobs: pending ordered slab sums (d att) that ride along."""
    # d basis, d root and both halves of dX are independent given dXB and g: one grouped launch.  When the reductions
    # fit the waves of one workgroup per output tile (BioSNAP: 645 and 1 056 terms) the products are FINISHED by that
    # launch, together with the d att slab sum (round 4: 10.4 + 7.6 us of split-K slabs + their sum per layer before);
    # otherwise grouped split-K products.  With a `shard`, [partial dX | partial d basis] live in ONE flat buffer the
    # products write into: a single all-reduce, no pack / unpack copies; d att (this rank's rows) and d root (replicated
    # operands: identical on every rank) need no collective
    n, d_in = x.shape
    nb, _, d_out = basis.shape
    slab_jobs = list(slab_jobs)
    flat = x_out = b_out = None
    if shard is not None:
        flat = torch.empty(n * d_in + nb * d_in * d_out, dtype=torch.float32, device=x.device)
        x_out, b_out = flat[:n * d_in].view(n, d_in), flat[n * d_in:].view(nb, d_in, d_out)
    jobs = None
    if len(slab_jobs) <= _lib.WG_SUMS_MAX:
        jobs = [wg_gemm_job(x.t(), g_xb, out=b_out), wg_gemm_job(x.t(), g)]
        if shard is None:
            jobs.append(wg_gemm_job(g_xb, basis.transpose(1, 2), reduce_batch=True, a2=g, b2=root.t(), gate=gate_x))
        else:
            jobs.append(wg_gemm_job(g_xb, basis.transpose(1, 2), reduce_batch=True, out=x_out))
    if jobs is not None and None not in jobs:
        wg_gemm_group(jobs, slab_jobs)
        j_basis, j_root, g_x = jobs[0], jobs[1], jobs[2].out
    else:
        j_root = gemm_job(x.t(), g)
        j_basis = gemm_job(x.t(), g_xb, out=b_out)                       # [B, in, out]
        if shard is None:
            j_xr = gemm_job(g, root.t(), ksplit=1)                       # written by the GEMM launch itself: the
            g_x = j_xr.out                                               # basis half is summed on top of it afterwards
            j_xq = gemm_job(g_xb, basis.transpose(1, 2), out=g_x, c_in=g_x, reduce_batch=True, kgroup=large_kgroup(n, nb))
            if j_xq.slabs is not None:                                   # summed on top of g root^T afterwards
                j_xq.gate = gate_x                                       # ... and masked with (x > 0) in the same pass
                gemm_group([j_basis, j_root, j_xr, j_xq], slab_jobs)
            else:                                                        # reads g_x while accumulating
                gemm_group([j_basis, j_root, j_xr], slab_jobs)
                gemm_group([j_xq])
                if gate_x is not None:
                    g_x = rows_affine(g_x, gate=gate_x)
        else:
            g_x = x_out
            j_xq = gemm_job(g_xb, basis.transpose(1, 2), out=g_x, reduce_batch=True, kgroup=large_kgroup(n, nb))   # partial over this shard
            gemm_group([j_basis, j_root, j_xq], slab_jobs)
    if shard is not None:
        shard.all_reduce(flat)
        g_x = gemm(g, root.t(), out=g_x, c_in=g_x)                       # replicated term, added once
        if gate_x is not None:
            g_x = rows_affine(g_x, gate=gate_x)
    return g_x, j_basis.out, j_root.out


class _RGCN(torch.autograd.Function):
    """One basis-decomposed R-GCN layer with global-mean aggregation
    (reference MyRGCNConv2 / MyRGCNConv, src/layers.py:102-193 / :21-99):

        out = D^-1 sum_r A_r X W_r + X root,   W_r = sum_b att[r,b] basis[b]

    evaluated basis-first / transform-then-gather: XB_b = X basis_b, then the aggregate on the route `rgcn_route` names --
    the pair form, the row sums of large graphs, or Y = att . XB and one gather-sum over the rows of Y (no E x d
    intermediates) -- each route a function of its own (`_rgcn_fwd_pair`, `_rgcn_fwd_large`, `_rgcn_fwd_y`).  The route is
    decided ONCE per pass and kept on the ctx; the backward pass is `_rgcn_grad_att_xb` (d att, dXB on the matching route;
    what depends on the graph's stamp or the operands' layout is decided there) and `rgcn_dense_tail` (dX, d basis, d root).

    With a `shard` (tip_amd/dist.py) the graph, `att` and its gradient hold only this rank's relations
    (`graph.scale` = 1 / GLOBAL in-degree): the partial aggregate is all-reduced before the 1/deg
    scaling, and [partial dX | partial d basis] are all-reduced as ONE flat buffer that the GEMMs write
    into directly; d att rows are shard-local and never travel."""

    @staticmethod
    def forward(ctx, x, basis, att, root, graph, shard, relu, gate_input=False, defer_output=False, partner=None, cells_token=None):
        """relu: False | True | 'gated_downstream' (ReLU applied here, its backward mask applied by the
        consumer, which must be the ONLY consumer and run with gate_input=True).
        gate_input: x is the ReLU output of the producing layer; dX is masked with (x > 0) while it is
        finished, i.e. the producer's ReLU backward is fused into this layer's last kernel."""
        x, basis, att, root = _f32c(x), basis.contiguous(), att.contiguous(), root.contiguous()
        n, d_in = x.shape
        nb, _, d_out = basis.shape
        route = rgcn_route(graph, n, d_in, d_out, nb, att.shape[0], shard, any(ctx.needs_input_grad[:3]), (x, basis, att), partner)
        pend = _take_pending(x, route.handover)
        ctx.xb_stamp = None
        if route.pair is not None:
            # every pass through here rewrites the graph's cell / XB buffers: a backward pass that finds another stamp than
            # its own forward pass left knows they are no longer its operands
            graph.pair_stamp += 1
            if route.xb != 'own':
                ctx.xb_stamp = graph.pair_stamp
            defer = shard is None and defer_output and relu == 'gated_downstream' and d_out == 32
            out, xb = _rgcn_fwd_pair(route, x, basis, att, root, graph, shard, relu, pend, defer, partner, cells_token)
        else:
            fwd = _rgcn_fwd_large if route.fwd in ('rows', 'dest') else _rgcn_fwd_y
            out, xb = fwd(route, x, basis, att, root, graph, shard, relu)
        ctx.route, ctx.graph, ctx.shard, ctx.relu, ctx.gate_input = route, graph, shard, relu, gate_input
        ctx.save_for_backward(x, basis, att, root, xb, out if relu is True else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, basis, att, root, xb, out = ctx.saved_tensors
        g = _f32c(g).contiguous()
        if ctx.relu is True:
            g = rows_affine(g, gate=out)                                 # ReLU gate of the fused epilogue
        g_att, g_xb = _rgcn_grad_att_xb(ctx, x, basis, att, xb, g)
        pending = [] if torch.is_tensor(g_att) else [g_att]              # the d att slabs ride in the tail's grouped slab sum
        g_x, g_basis, g_root = rgcn_dense_tail(x, basis, root, g, g_xb, x if ctx.gate_input else None, pending, ctx.shard)
        if pending:
            g_att = g_att.out
        return g_x, g_basis, g_att, g_root, None, None, None, None, None, None, None


def rgcn(x, basis, att, root, graph, shard=None, relu=False, gate_input=False, defer_output=False, partner=None, cells_token=None):
    """partner (optional): (att, graph, d_out, token) of the NEXT R-GCN layer on the same D-D graph -- its pair cells are gathered
    in this layer's cell launch (`stream_gather_two`); the next layer is then called with cells_token = the same token object."""
    return _RGCN.apply(x, basis, att, root, graph, shard, relu, gate_input, defer_output, partner, cells_token)


class _DrugMix(torch.autograd.Function):
    """x0 = cat(embed / d_norm, pd) or embed / d_norm + pd  (src/layers.py:532-539)."""

    @staticmethod
    def forward(ctx, xd, pd, d_norm, cat):
        xd, pd = _f32c(xd), _f32c(pd)
        n, ne = xd.shape
        with _timed('drug_mix[%dx%d,%s]' % (n, pd.shape[1], 'cat' if cat else 'add')):      # (spans two launches, whose own labels are recorded as well)
            if cat:
                out = torch.empty((n, ne + pd.shape[1]), dtype=torch.float32, device=xd.device)
                rows_affine(xd, row_div=d_norm, out=out[:, :ne])
                rows_affine(pd, out=out[:, ne:])
            else:
                out = rows_affine(xd, row_div=d_norm)
                rows_affine(pd, out=out, accumulate=True)
        ctx.cat, ctx.ne = cat, ne
        ctx.save_for_backward(d_norm)
        return out

    @staticmethod
    def backward(ctx, g):
        (d_norm,) = ctx.saved_tensors
        g = _f32c(g)
        ne = ctx.ne
        if ctx.cat:
            return rows_affine(g[:, :ne], row_div=d_norm), rows_affine(g[:, ne:]), None, None
        return rows_affine(g, row_div=d_norm), g, None, None


def drug_mix(xd, pd, d_norm, cat):
    return _DrugMix.apply(xd, pd, d_norm, cat)


class _DrugMixMM(torch.autograd.Function):
    """x0 = cat(embed / d_norm, mean @ W) or embed / d_norm + mean @ W: the dense map of
    MyHierarchyConv (src/layers.py:239) writes straight into the mixed feature matrix
    (:532-539), and its gradient is read from a column-slice view on the way back."""

    @staticmethod
    def forward(ctx, xd, mean, weight, d_norm, cat):
        xd, mean, weight = _f32c(xd), _f32c(mean), _f32c(weight)
        n, ne = xd.shape
        pd_dim = weight.shape[1]
        p = weight.shape[0]
        ctx.fused = p <= 64 and pd_dim <= 64 and weight.is_contiguous() and d_norm.is_contiguous()
        if ctx.fused:                                                     # scaling, cat | add and the dense map: one launch
            out = torch.empty((n, ne + pd_dim if cat else ne), dtype=torch.float32, device=xd.device)
            with _timed('drug_mix_mm[%dx%dx%d,fused]' % (n, p, pd_dim)):
                check(lib().tipk_drug_mix_fwd(ptr(xd), xd.stride(0), ptr(d_norm), ptr(mean), mean.stride(0), ptr(weight), p, pd_dim,
                                              n, ne, int(cat), ptr(out), out.stride(0), stream_ptr(xd.device)), 'tipk_drug_mix_fwd')
            ctx.cat, ctx.ne = cat, ne
            ctx.save_for_backward(mean, weight, d_norm)
            return out
        with _timed('drug_mix_mm[%dx%dx%d,unfused]' % (n, p, pd_dim)):                       # (spans two launches, whose own labels are recorded as well)
            if cat:
                out = torch.empty((n, ne + pd_dim), dtype=torch.float32, device=xd.device)
                rows_affine(xd, row_div=d_norm, out=out[:, :ne])
                gemm(mean, weight, out=out[:, ne:])
            else:
                out = rows_affine(xd, row_div=d_norm)
                gemm(mean, weight, out=out, c_in=out)
        ctx.cat, ctx.ne = cat, ne
        ctx.save_for_backward(mean, weight, d_norm)
        return out

    @staticmethod
    def backward(ctx, g):
        mean, weight, d_norm = ctx.saved_tensors
        g = _f32c(g)
        g_pd = g[:, ctx.ne:] if ctx.cat else g
        g_xd = rows_affine(g[:, :ctx.ne] if ctx.cat else g, row_div=d_norm)
        j_w = gemm_job(mean.t(), g_pd)
        j_m = gemm_job(g_pd, weight.t()) if ctx.needs_input_grad[1] else None
        gemm_group([j for j in (j_w, j_m) if j is not None])
        return g_xd, (j_m.out if j_m else None), j_w.out, None, None


def drug_mix_mm(xd, mean, weight, d_norm, cat):
    return _DrugMixMM.apply(xd, mean, weight, d_norm, cat)


def drug_mix_gather_supported(h, weight, d_norm):
    p, q = weight.shape
    return bool(h.is_cuda and h.dtype == torch.float32 and h.stride(1) == 1 and weight.is_contiguous() and
                (d_norm is None or d_norm.is_contiguous()) and lib().tipk_drug_mix_gather_supported(int(p), int(q)))


def drug_mix_gather_launch(xd, h, weight, d_norm, cat, graph):
    """(x0, mean, weight as passed to the kernel): the forward launch of the fused P -> D + drug-mix stage (`tipk_drug_mix_gather_fwd`)."""
    xd, h, weight = _f32c(xd), _f32c(h), _f32c(weight).contiguous()
    csr = graph.pd_csr
    require_device(xd, h, weight, d_norm, csr['fwd_ptr'])
    n, ne = xd.shape
    p, q = weight.shape
    assert h.shape == (csr['n_src'], p) and csr['fwd_ptr'].numel() == n + 1
    out = torch.empty((n, ne + q if cat else ne), dtype=torch.float32, device=xd.device)
    mean = torch.empty((n, p), dtype=torch.float32, device=xd.device)
    with _timed('drug_mix_gather_fwd[%dx%dx%d]' % (n, p, q)):
        check(lib().tipk_drug_mix_gather_fwd(ptr(xd), xd.stride(0), ptr(d_norm), ptr(h), h.stride(0), ptr(csr['fwd_ptr']),
                                             ptr(csr['fwd_src']), ptr(csr['scale']), ptr(csr['fwd_wg']), ptr(csr['fwd_order']), csr['fwd_wg'].shape[0],
                                             ptr(weight), p, q, n, ne, int(cat),
                                             ptr(out), out.stride(0), ptr(mean), stream_ptr(xd.device)),
              'tipk_drug_mix_gather_fwd')
    return out, mean, weight


class _DrugMixGather(torch.autograd.Function):
    """x0 = cat(xd / d_norm, mean(H) W) or xd / d_norm + mean(H) W with mean(H)[d] = the mean of the source rows that point
    at d (MyHierarchyConv, src/layers.py:229-242, + the mix of :532-539): one launch forward; backward one launch for
    d xd, d mean and d W + the transposed gather of d mean on its plan (include/tipk.h section 3, csrc/tipk_drugmix.hip)."""

    @staticmethod
    def forward(ctx, xd, h, weight, d_norm, cat, graph):
        out, mean, weight = drug_mix_gather_launch(xd, h, weight, d_norm, cat, graph)
        ctx.cat, ctx.ne, ctx.graph = cat, xd.shape[1], graph
        ctx.save_for_backward(mean, weight, d_norm)
        return out

    @staticmethod
    def backward(ctx, g):
        mean, weight, d_norm = ctx.saved_tensors
        g = _f32c(g)
        n, p = mean.shape
        q = weight.shape[1]
        dev = g.device
        g_xd = torch.empty((n, ctx.ne), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_mean = torch.empty((n, p), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        g_w = torch.empty((p, q), dtype=torch.float32, device=dev)
        with _timed('drug_mix_bwd[%dx%dx%d]' % (n, p, q)):
            check(lib().tipk_drug_mix_bwd(ptr(g), g.stride(0), ptr(d_norm), ptr(mean), ptr(weight), p, q, n, ctx.ne, int(ctx.cat),
                                          ptr(g_xd), g_xd.stride(0) if g_xd is not None else 0, ptr(g_mean), ptr(g_w),
                                          stream_ptr(dev)), 'tipk_drug_mix_bwd')
        # back to the source rows: the transposed plan carries 1 / count of the edge's target as edge weights
        g_h = gather_sum(ctx.graph.bwd, g_mean) if g_mean is not None else None
        return g_xd, g_h, g_w, None, None, None


def drug_mix_gather(xd, h, weight, d_norm, cat, graph):
    return _DrugMixGather.apply(xd, h, weight, d_norm, cat, graph)


_ONES = {}


def _ones(n, device):
    key = (int(n), str(device))
    if key not in _ONES:
        _ONES[key] = torch.ones((1, int(n)), dtype=torch.float32, device=device)
    return _ONES[key]


class _GCNConv(torch.autograd.Function):
    """out = relu?(A_hat (x W^T) + bias): GCNConv as one node of the autograd graph, so that the
    three gradients that only need the transposed aggregate -- d W, d x and d bias (= 1^T g as a
    1-row product) -- leave in ONE grouped launch (PyG GCNConv.forward; src/layers.py:392-394)."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, relu, link=None):
        """relu: False | True | 'gated_downstream' -- the ReLU is applied here, its backward mask AND the column sums of the
        masked gradient (d bias, as partial rows in `link.parts`) are produced by the ONE consumer of the output, which runs
        with gate_input=True and the same `link` (`_GCNConvAggFirst`: in the epilogue of its transposed aggregation)."""
        ctx.identity = x is None
        if x is None:
            xl = transpose(weight)                                       # lin(I) = W^T
        else:
            x = _f32c(x)
            xl = gemm(x, weight.t())
        out = gather_sum(graph.fwd, xl, row_scale=graph.scale, bias=bias, relu=bool(relu))
        ctx.graph, ctx.relu, ctx.has_bias, ctx.link = graph, relu, bias is not None, link
        ctx.save_for_backward(x, weight, out if relu is True else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, out = ctx.saved_tensors
        graph = ctx.graph
        g = _f32c(g).contiguous()
        bias_parts = None
        handed = ctx.relu == 'gated_downstream'                         # g arrives masked; its column sums may come with it
        if handed:
            g_pre = g
            bias_parts = ctx.link.parts if (ctx.link is not None and ctx.has_bias) else None
            if ctx.link is not None:
                ctx.link.parts = None
        elif ctx.relu and ctx.has_bias:                                 # ReLU gate + stage 1 of d bias in one pass
            fused = gate_colsum(g, out)
            if fused is not None:
                g_pre, bias_parts = fused
        if bias_parts is None and not handed:
            g_pre = rows_affine(g, gate=out) if ctx.relu else g
        g_agg = rows_affine(g_pre, row_mul=graph.scale) if graph.scale is not None else g_pre
        s_bias = None
        if ctx.identity and bias_parts is not None:
            # identity features: nothing else is summed after the transposed aggregation -- the bias partials ride in ITS launch
            s_bias = slab_job(bias_parts)
            g_table = gather_sum(graph.bwd, g_agg, riders=[s_bias])
        else:
            g_table = gather_sum(graph.bwd, g_agg)
        j_b = None
        if ctx.has_bias and bias_parts is None:
            j_b = gemm_job(_ones(g_pre.shape[0], g.device), g_pre)
        if ctx.identity:
            # d W = (d lin)^T: a VIEW when the parameter is stored transposed (tip_amd.layers._Lin), its strides
            # then equal the parameter's, so the optimizer's fused / foreach paths apply
            g_w = g_table.t() if weight.t().is_contiguous() else transpose(g_table)
            if s_bias is not None:
                return None, g_w, s_bias.out.view(-1), None, None, None
            if j_b is not None:
                gemm_group([j_b])
            return None, g_w, (j_b.out.view(-1) if j_b else None), None, None, None
        # d W in the parameter's own memory layout (tip_amd.layers._Lin keeps [in, out] storage behind the [out, in]
        # shape): autograd's AccumulateGrad otherwise re-lays the gradient out with a copy kernel of its own
        w_t = weight.t().is_contiguous() and not weight.is_contiguous()
        j_w = gemm_job(x.t(), g_table) if w_t else gemm_job(g_table.t(), x)
        g_w = j_w.out.t() if w_t else j_w.out
        j_x = gemm_job(g_table, weight) if ctx.needs_input_grad[0] else None
        if bias_parts is not None:                                      # rides in the grouped slab sum below
            s_b = slab_job(bias_parts)
            gemm_group([j for j in (j_w, j_x) if j is not None], [s_b])
            return (j_x.out if j_x else None), g_w, s_b.out.view(-1), None, None, None
        gemm_group([j for j in (j_w, j_x, j_b) if j is not None])
        return (j_x.out if j_x else None), g_w, (j_b.out.view(-1) if j_b else None), None, None, None


class GateLink(object):
    """Hand-over between a ReLU layer (`relu='gated_downstream'`) and the one consumer of its output (`gate_input=True`): the
    consumer's backward pass leaves the column sums of the masked gradient here (partial rows [W, 1, d]) for the layer's."""
    __slots__ = ('parts',)

    def __init__(self):
        self.parts = None


def gcn_conv(x, weight, bias, graph, relu=False, link=None):
    """x = None means identity features."""
    return _GCNConv.apply(x, weight, bias, graph, relu, link)


class _GCNConvAggFirst(torch.autograd.Function):
    """out = relu?((A_hat x) W^T + bias) -- the same map as `_GCNConv` (A_hat (x W^T) = (A_hat x) W^T), aggregate FIRST: for a
    layer whose output is needed for a few rows only (`gcn_norm_graph(rows=...)`: conv2 of the P-P encoder, 3 640 of 19 081
    proteins) the dense map then runs on the kept rows inside the gather's launch (`gather_sum_lin`), and the backward pass
    is one launch for g W, d W = g^T (A_hat x) and d bias (reductions over the kept rows: `wg_gemm_group`) + the transposed
    gather -- 1 + 2 launches where transform-first took 2 + 3 (src/layers.py:392-394)."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, relu, gate_input=False, link=None):
        """gate_input: x is the ReLU output of a layer called with relu='gated_downstream' -- dx is masked with (x > 0), and
        the column sums of the masked dx go to `link.parts`, in the epilogue of the transposed aggregation."""
        x = _f32c(x)
        agg, out = gather_sum_lin(graph.fwd, x, weight, bias, relu, row_scale=graph.scale)
        ctx.graph, ctx.relu, ctx.has_bias, ctx.gate_input, ctx.link = graph, relu, bias is not None, gate_input, link
        ctx.save_for_backward(agg, weight, out if relu else None, x if gate_input else None)
        return out

    @staticmethod
    def backward(ctx, g):
        agg, weight, out, x_in = ctx.saved_tensors
        graph = ctx.graph
        g = _f32c(g).contiguous()
        if ctx.relu:
            g = rows_affine(g, gate=out)
        # d W in the parameter's own memory layout (tip_amd.layers._Lin keeps [in, out] storage behind the [out, in] shape)
        w_t = weight.t().is_contiguous() and not weight.is_contiguous()
        j_w = wg_gemm_job(agg.t(), g) if w_t else wg_gemm_job(g.t(), agg)
        j_x = wg_gemm_job(g, weight) if ctx.needs_input_grad[0] else None
        j_b = wg_gemm_job(_ones(g.shape[0], g.device), g) if ctx.has_bias else None
        if j_w is None or (ctx.needs_input_grad[0] and j_x is None) or (ctx.has_bias and j_b is None):
            # reductions beyond one workgroup's reach: the grouped split-K products and their slab sum
            j_w = gemm_job(agg.t(), g) if w_t else gemm_job(g.t(), agg)
            j_x = gemm_job(g, weight) if ctx.needs_input_grad[0] else None
            j_b = gemm_job(_ones(g.shape[0], g.device), g) if ctx.has_bias else None
            # ... whose slab sums ride in the transposed aggregation's launch (it only needs g W, which is written directly)
            riders = gemm_group([j for j in (j_w, j_x, j_b) if j is not None], defer_sums=j_x is not None and j_x.slabs is None)
            if j_x is None or j_x.slabs is not None:
                riders = []
        else:
            wg_gemm_group([j for j in (j_w, j_x, j_b) if j is not None])
            riders = []
        g_w = j_w.out.t() if w_t else j_w.out
        g_x = None
        if j_x is not None:
            gw = j_x.out if graph.scale is None else rows_affine(j_x.out, row_mul=graph.scale)
            if ctx.gate_input and gather_sum_epilogue_supported(graph.bwd, gw.shape[1]):
                # the producer's ReLU backward and the partial rows of ITS bias gradient in this launch's epilogue
                want = ctx.link is not None
                res = gather_sum(graph.bwd, gw, riders=riders, gate=x_in, colsum=want)
                g_x = res[0] if want else res
                if want:
                    ctx.link.parts = res[1]
            else:
                g_x = gather_sum(graph.bwd, gw, riders=riders)
                if ctx.gate_input:
                    g_x = rows_affine(g_x, gate=x_in)
        return g_x, g_w, (j_b.out.view(-1) if j_b is not None else None), None, None, None, None


def gcn_conv_agg_first(x, weight, bias, graph, relu=False, gate_input=False, link=None):
    return _GCNConvAggFirst.apply(x, weight, bias, graph, relu, gate_input, link)


class _DistMult(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, edge_index, edge_type, sigmoid):
        score = distmult_fwd(z, weight, edge_index, edge_type, sigmoid)
        ctx.sigmoid = sigmoid
        ctx.save_for_backward(z, weight, edge_index, edge_type, score)
        return score

    @staticmethod
    def backward(ctx, g):
        z, weight, edge_index, edge_type, score = ctx.saved_tensors
        g_z, g_w = distmult_bwd(g, score, z, weight, edge_index, edge_type, ctx.sigmoid)
        return g_z, g_w, None, None, None


def distmult(z, weight, edge_index, edge_type, sigmoid=True):
    return _DistMult.apply(z, weight, edge_index, edge_type, sigmoid)


_UNIT_GRADS = {}          # data_ptr -> tensor: upstream gradients known to be exactly 1 (`unit_grad`)


def unit_grad(device):
    """A 0-dim ones tensor for `loss.backward(gradient=...)` that the fused objective recognises by its address: the
    backward pass then hands out the gradients of the forward launch as they are (no seed-filling launch, no scaling
    launch).  tip_amd.train.GraphedTrainStep uses it; the tensor must never be written."""
    device = torch.device(device)
    for t in _UNIT_GRADS.values():
        if t.device == device:
            return t
    t = torch.ones((), dtype=torch.float32, device=device)
    _UNIT_GRADS[t.data_ptr()] = t
    return t


class _DistMultLoss(torch.autograd.Function):
    """loss of TIP.forward (src/layers.py:335-340) with gradients produced in the same pass."""

    @staticmethod
    def forward(ctx, z, weight, pos_index, neg_index, edge_type):
        need = z.requires_grad or weight.requires_grad
        loss, g_z, g_w = distmult_loss(z, weight, pos_index, neg_index, edge_type, need_grad=need)
        ctx.save_for_backward(g_z, g_w)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        g_z, g_w = ctx.saved_tensors
        if g_z is None:
            return None, None, None, None, None
        if g.data_ptr() in _UNIT_GRADS:                    # the caller vouches for an upstream gradient of exactly 1
            return g_z, g_w, None, None, None
        g_z, g_w = torch._foreach_mul([g_z, g_w], g)       # one launch for both
        return g_z, g_w, None, None, None


def distmult_objective(z, weight, pos_index, neg_index, edge_type):
    return _DistMultLoss.apply(z, weight, pos_index, neg_index, edge_type)


def rank_metrics(pos_score, neg_score, range_ptr, max_pairs):
    """fp64 [3, R] (AUPRC, AUROC, AP) per relation on device (include/tipk.h section 6), or None if a
    relation is too large for the single-workgroup sort."""
    pos_score, neg_score = _f32c(pos_score).contiguous(), _f32c(neg_score).contiguous()
    require_device(pos_score, neg_score, range_ptr)
    n_rel = range_ptr.numel() - 1
    out = torch.empty((3, n_rel), dtype=torch.float64, device=pos_score.device)
    st = lib().tipk_rank_metrics(ptr(pos_score), ptr(neg_score), ptr(range_ptr), n_rel, int(max_pairs), ptr(out),
                                 stream_ptr(pos_score.device))
    if st == -2:                                   # TIPK_EUNSUPPORTED
        return None
    check(st, 'tipk_rank_metrics')
    return out


class _PairTable(torch.autograd.Function):
    """score[e] = sigma(s1[u_e, r_e] + s2[v_e, r_e])  (include/tipk.h section 4b)."""

    @staticmethod
    def forward(ctx, s1, s2, edge_index, edge_type, sigmoid):
        s1, s2 = _f32c(s1).contiguous(), _f32c(s2).contiguous()
        require_device(s1, s2, edge_index, edge_type)
        assert s1.shape == s2.shape
        validate_triples(edge_index, edge_type, s1.shape[0], s1.shape[1])
        u, v = _uv(edge_index)
        et = edge_type.contiguous()
        n = u.numel()
        score = torch.empty((n,), dtype=torch.float32, device=s1.device)
        check(lib().tipk_pair_table_fwd(ptr(s1), ptr(s2), s1.shape[1], ptr(u), ptr(v), _idx_bytes(u), ptr(et),
                                        _idx_bytes(et), n, int(sigmoid), ptr(score), stream_ptr(s1.device)),
              'tipk_pair_table_fwd')
        ctx.sigmoid, ctx.shape = sigmoid, s1.shape
        ctx.save_for_backward(edge_index, et, score)
        return score

    @staticmethod
    def backward(ctx, g):
        edge_index, et, score = ctx.saved_tensors
        g = _f32c(g).contiguous()
        u, v = _uv(edge_index)
        g1 = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        g2 = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        check(lib().tipk_pair_table_bwd(ptr(g), ptr(score), ctx.shape[1], ptr(u), ptr(v), _idx_bytes(u), ptr(et),
                                        _idx_bytes(et), u.numel(), int(ctx.sigmoid), ptr(g1), ptr(g2),
                                        stream_ptr(g.device)), 'tipk_pair_table_bwd')
        return g1, g2, None, None, None


class _PairTableLoss(torch.autograd.Function):
    """The fused TIP objective on the TRANSPOSED score tables of the NNDecoder (`tipk_pair_table_loss`): loss and both table
    gradients in one launch, reproducible bit for bit."""

    @staticmethod
    def forward(ctx, s1t, s2t, pos_index, neg_index, edge_type):
        s1t, s2t = _f32c(s1t).contiguous(), _f32c(s2t).contiguous()
        require_device(s1t, s2t, pos_index, neg_index, edge_type)
        r, n = s1t.shape
        assert s2t.shape == (r, n) and n <= 65535
        validate_triples(pos_index, edge_type, n, r)
        facts = _facts(edge_type)
        blocks = facts.get('rel_blocks')
        if blocks is None:
            rels, counts = torch.unique_consecutive(edge_type, return_counts=True)
            if torch.unique(rels).numel() != rels.numel():
                raise _lib.TipkError('the fused objective needs the triples grouped by relation (src/utils.py:35-65)')
            cnt = torch.zeros(r, dtype=torch.int64, device=edge_type.device)
            cnt[rels.to(torch.int64)] = counts
            rel_ptr = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)]).contiguous()
            order = torch.sort(cnt, descending=True, stable=True).indices.to(torch.int32).contiguous()
            blocks = facts['rel_blocks'] = (rel_ptr, order)
        rel_ptr, order = blocks
        pp = packed_pairs(pos_index, n)
        if getattr(neg_index, '_tipk_packed_pairs', False):
            npk = neg_index
            if not getattr(neg_index, '_tipk_sampled', False):
                validate_triples(unpack_pairs(neg_index), None, n, r)
        else:
            if not getattr(neg_index, '_tipk_sampled', False):
                validate_triples(neg_index, None, n, r)
            w = neg_index[0].to(torch.int64) | (neg_index[1].to(torch.int64) << 16)
            npk = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()
        assert npk.numel() == pp.numel()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        parts = torch.empty((r, 2), dtype=torch.float64, device=s1t.device)
        g1 = torch.empty_like(s1t) if need else None
        g2 = torch.empty_like(s2t) if need else None
        with _timed('pair_table_loss[%dx%d,positions=%d]' % (r, n, pp.numel())):
            check(lib().tipk_pair_table_loss(ptr(s1t), ptr(s2t), s1t.stride(0), n, r, ptr(pp), ptr(npk), ptr(rel_ptr), ptr(order),
                                             pp.numel(), 1e-13, ptr(parts), ptr(g1), ptr(g2), stream_ptr(s1t.device)),
                  'tipk_pair_table_loss')
        ctx.save_for_backward(g1, g2)
        return (parts.sum() * (-1.0 / pp.numel())).to(torch.float32).view(1)

    @staticmethod
    def backward(ctx, g):
        g1, g2 = ctx.saved_tensors
        return g1 * g, g2 * g, None, None, None


def pair_table_loss_supported(n_nodes):
    """True if `tipk_pair_table_loss` takes a node set of this size (two table rows of a relation in LDS: 24 B per node)."""
    return 0 < int(n_nodes) * 24 <= 150 * 1024 and int(n_nodes) <= 65535


def pair_table_objective(s1t, s2t, pos_index, neg_index, edge_type):
    """loss [1] of the fused objective on the transposed score tables s1t / s2t [R, N] (include/tipk.h section 4b)."""
    return _PairTableLoss.apply(s1t, s2t, pos_index, neg_index, edge_type)


def pair_table_score(s1, s2, edge_index, edge_type, sigmoid=True):
    return _PairTable.apply(s1, s2, edge_index, edge_type, sigmoid)
