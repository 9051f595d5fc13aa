"""MI355X-native TIP modules behind the reference's `nn.Module` surface (`src/layers.py`).

Class names, constructor/forward signatures, parameter names, shapes and init rules follow the
reference so that its `state_dict`s load and `tip.py`'s loop runs unchanged (SURVEY.md section
8(b)); the bodies are new: every layer is a `torch.autograd.Function` from `tip_amd.ops` that
launches the HIP kernels of libtipk through the C ABI.  There is no PyG and no CPU path.

Static-graph caching: the reference's `GCNConv(cached=True)` (`src/layers.py:386-387`) keeps the
normalised P-P graph after the first call.  Here EVERY layer caches its gather plans, keyed by the
identity and version of the edge tensors it was given and pinning them while cached
(`_cache.DerivedCache`), because all three TIP graphs are constant during training.  Pass a new
tensor (or modify in place) to rebuild.
"""
import math
import os
import pickle
from collections import namedtuple

import numpy as np
import torch
from torch import nn
from torch.nn import Parameter as Param

from . import encoder, ops, switches
from ._cache import DerivedCache, keyable
from .data import Data, build_data_dict
from .neg_sampling import typed_negative_sampling
from .plan import (build_pair_bwd_plan, build_dest_plan, build_row_stream_plan, build_row_stream_plan_s, build_gather_plan, build_gather_plan_segmented, build_rel_plan, build_stream_plan, build_stream_plan_rows, build_csr_plan, group_slots_for,
                   relations_per_segment, DEFAULT_CHUNK)
from .utils import process_edges, auprc_auroc_ap_by_range, rank_report

EPS = 1e-13                    # src/layers.py:15

# TIP.screen's result: per query row the k best pairs (u, v) of side effect `relation`, best first
ScreenResult = namedtuple('ScreenResult', ['score', 'u', 'v', 'relation'])
# TIP.side_effects' result: per pair row the k best side effects, best first (padding: score 0 / -inf, relation -1)
SideEffects = namedtuple('SideEffects', ['score', 'relation'])
Explanation = namedtuple('Explanation', ['logit', 'offset', 'own', 'neighbours', 'contribution', 'partner', 'relation', 'degree'])
ProteinExplanation = namedtuple('ProteinExplanation', ['logit', 'offset', 'features', 'proteins', 'contribution', 'protein', 'direct',
                                                       'targets'])
NewDrugs = namedtuple('NewDrugs',['x0', 'h', 'z', 'degree', 'n_targets'])
# TIP.fit_side_effects' result: per new side effect its fitted DistMult row and how the fit ended
NewSideEffects = namedtuple('NewSideEffects', ['weight', 'loss', 'grad_norm', 'evaluations', 'status', 'n_pairs', 'decoder', 'known'])
# what `TIP.fit_new_drugs` returns; `.z` makes it go wherever the `NewDrugs` of `embed_new_drugs` goes
FittedDrugs = namedtuple('FittedDrugs', ['z', 'loss', 'grad_norm', 'evaluations', 'status', 'n_interactions', 'hess'])
RegimenSideEffects = namedtuple('RegimenSideEffects', ['score', 'relation', 'u', 'v'])
AddOnRisk = namedtuple('AddOnRisk', ['burden', 'candidate', 'ptr', 'best_burden', 'best_drug'])
# TIP.combination_risk's result: the total burden of every combination of alternatives and each query's k safest ones
CombinationRisk = namedtuple('CombinationRisk', ['burden', 'ptr', 'best_burden', 'best_combination', 'best_drugs'])
# TIP.drug_profile's result: per queried drug the expected number of unrecorded partners for every side effect column
DrugProfile = namedtuple('DrugProfile', ['expected', 'candidates', 'top_expected', 'top_relation'])
RankReport = namedtuple('RankReport', ['rank', 'logit', 'mrr', 'hits', 'per_relation', 'macro_mrr', 'unranked'])


class DecoderPosterior(namedtuple('DecoderPosterior', ['weight', 'factor', 'n_pairs', 'relation', 'known'])):
    """TIP.decoder_posterior's result: the Gaussian (Laplace) posterior N(weight[b], covariance()[b]) of B DistMult rows.
    factor [B, dim, dim]: W_b = P_b^(-1/2) chol(H_b)^-1 in the layout `ops.spd_factor` writes (factor[b, j, i] = W_b[i][j]);
    n_pairs int64 [B] = P_b; relation int64 [B]: the side-effect id of every row (global ids for the model's rows, 0..B-1 for
    given rows); known: None for the model's rows, else the given pairs as pair-major lists (`ops.known_relations_by_pair`)."""
    __slots__ = ()

    def covariance(self):
        """Sigma [B, dim, dim] = W^T W = (P_b H_b)^-1, rows and columns in the order of `weight`'s components."""
        return self.factor @ self.factor.transpose(1, 2)


# TIP.side_effects_confidence's result: per pair row the k best side effects by the chosen key, best first (padding:
# probabilities 0, logit -inf, std +inf, relation -1)
ConfidentSideEffects = namedtuple('ConfidentSideEffects', ['probability', 'mean_probability', 'logit', 'std', 'relation',
                                                           'dense_logit', 'dense_std'])


class Calibration(namedtuple('Calibration', ['scale', 'offset', 'loss', 'loss_raw', 'expected_raw', 'n_pos', 'n_neg', 'n_dropped',
                                             'evaluations', 'status', 'z', 'decoder'])):
    """TIP.calibrate's result: the Platt map logit' = scale[r] * logit + offset[r] of every side effect r (include/tipk.h
    section 4r) and the operands that apply it.  scale, offset, loss [R]: the fitted map and its objective; loss_raw,
    expected_raw [R]: the objective and the sum of sigma(logit) over the POS and NEG cells at the identity map -- how many
    positives the raw model expects where n_pos are held out; n_pos, n_neg, n_dropped int64 [R]; evaluations, status int64
    [R] (1 converged, 2 step underflow, 3 non-finite statistic, 0 not converged, 4 not fitted: the identity is kept).
    z [n_drug, dim + 4]: a detached SNAPSHOT of the embeddings widened by the columns (1, 0, 0, 0); decoder: a frozen
    `MultiInnerProductDecoder(dim + 4, R)`, not registered in the model, with the rows [scale w_r | offset 0 0 0], so every
    DistMult query on (z, decoder) computes scale * logit + offset."""
    __slots__ = ()

    def embed(self, x):
        """Rows [M, dim] of further drugs (e.g. `NewDrugs.z`) widened to [M, dim + 4] as `z` is."""
        x = torch.as_tensor(x).detach().to(self.z.device, self.z.dtype)
        if x.dim() != 2 or x.shape[1] != self.z.shape[1] - 4:
            raise ValueError('embed: rows [M, %d] expected, got %s' % (self.z.shape[1] - 4, tuple(x.shape)))
        pad = x.new_zeros((x.shape[0], 4))
        pad[:, 0] = 1.0
        return torch.cat([x, pad], 1)


def calibrated_operands(z, w, ab):
    """The operands that apply the maps ab [R, 2] = (scale, offset) to the DistMult logit of z [n, dim] and w [R, dim]: z' =
    [z | 1 0 0 0] and a frozen, unregistered `MultiInnerProductDecoder(dim + 4, R)` with the rows [scale w_r | offset 0 0 0].
    The constant column is the last term of the ascending fma chain of every entry."""
    n, dim = z.shape
    wide = z.new_zeros((n, dim + 4))
    wide[:, :dim], wide[:, dim] = z.detach(), 1.0
    dec = MultiInnerProductDecoder(dim + 4, w.shape[0]).to(z.device)
    dec.weight.data.zero_()
    dec.weight.data[:, :dim] = ab[:, :1].to(w.dtype) * w.detach()
    dec.weight.data[:, dim] = ab[:, 1].to(w.dtype)
    dec.weight.requires_grad_(False)
    return wide, dec


__all__ = ['GCNConv', 'MyRGCNConv', 'MyRGCNConv2', 'MyHierarchyConv', 'PPEncoder', 'FMEncoder',
           'FMEncoderCat', 'MultiInnerProductDecoder', 'NNDecoder', 'Setting', 'TIP', 'NewSideEffects', 'FittedDrugs',
           'CombinationRisk', 'DecoderPosterior', 'ConfidentSideEffects', 'Calibration']


# ---------------------------------------------------------------------------------------------
# plan caches
# ---------------------------------------------------------------------------------------------
class _PlanCache(DerivedCache):
    """One slot per layer (graphs are static; a changed tensor identity rebuilds); .value: the plans it handed out last.
    Never pickled (`DerivedCache`): `torch.save(model, ...)` as in the reference's tip.py:36 works after a forward pass."""

    def __init__(self, limit=1):
        super().__init__(limit)
        self.value = None

    def get(self, key_tensors, builder):
        self.value = super().get(key_tensors, None, builder)
        return self.value


def _is_identity_features(x):
    """True for the `sparse_id(n)` features of prepare.py:22-23 (cached on the tensor object)."""
    if x is None:
        return True
    flag = getattr(x, '_tipk_identity', None)
    if flag is None:
        flag = False
        if x.is_sparse and x.shape[0] == x.shape[1]:
            xc = x.coalesce()
            idx, val = xc.indices(), xc.values()
            n = x.shape[0]
            ar = torch.arange(n, device=idx.device)
            flag = bool(idx.shape[1] == n and (idx[0] == ar).all() and (idx[1] == ar).all() and (val == 1).all())
        try:
            x._tipk_identity = flag
        except Exception:
            pass
    return flag


def _sparse_feature_graph(x, chunk):
    """Plans for y = x_sparse @ table (general sparse features, e.g. mono side-effect columns)."""
    xc = x.coalesce()
    r, c, v = xc.indices()[0], xc.indices()[1], xc.values().to(torch.float32)
    n, m = x.shape
    return ops.AggGraph(build_gather_plan(r, c, n, m, v, chunk, 'feat.fwd'), build_gather_plan(c, r, m, n, v, chunk, 'feat.bwd'))


class _FeatureInput(nn.Module):
    """`x @ W` for identity / sparse / dense `x` -- the three feature kinds the reference's
    `torch.matmul(x_drug, embed)` (:532) and `GCNConv.lin` can meet."""

    def __init__(self):
        super().__init__()
        self._cache = _PlanCache()

    def apply_table(self, x, table):
        """table: [in, out] (already in x @ table orientation)."""
        if _is_identity_features(x):
            return table
        if x.is_sparse:
            graph = self._cache.get((x,), lambda: _sparse_feature_graph(x, DEFAULT_CHUNK))
            return ops.aggregate(table, graph)
        return ops.matmul(x, table)


# ---------------------------------------------------------------------------------------------
# A1  GCNConv / PPEncoder   (src/layers.py:380-395; GCNConv = PyG 2.0.1 semantics)
# ---------------------------------------------------------------------------------------------
class _Lin(nn.Module):
    """bias-free linear map with glorot weight [out, in] (PyG `Linear(weight_initializer='glorot')`)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        # shape [out, in] as in PyG (state_dicts load unchanged), MEMORY [in, out]: with identity features
        # lin(I) = W^T is then the parameter's own storage and d W = (d lin)^T a view of the gradient the
        # aggregation kernel wrote -- no transpose kernels on either pass (19 081 x 32 at BioSNAP)
        self.weight = Param(torch.empty(in_channels, out_channels).t())
        bound = math.sqrt(6.0 / (in_channels + out_channels))
        self.weight.data.uniform_(-bound, bound)


def gcn_norm_graph(edge_index, num_nodes, chunk=DEFAULT_CHUNK, d=None, rows=None):
    """Normalised adjacency D^-1/2 (A + I) D^-1/2 as a pair of gather plans: existing self loops
    are replaced by exactly one unit loop per node, deg = in-degree incl. the loop, inf -> 0.
    d: width of the rows the plans will aggregate (enables in-workgroup combination of split rows).
    rows: ascending int64 node ids -- only THESE output rows are produced, as a compact [len(rows), d] matrix (same
    weights, same edge order inside a row as in the full graph; the transposed plan reads the compact gradient and
    writes all num_nodes rows).  FMEncoder uses it for conv2: only the proteins that are P -> D sources are ever read."""
    G = group_slots_for(d) if d else 0
    row, col = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    keep = row != col
    loop = torch.arange(num_nodes, device=row.device)
    row, col = torch.cat([row[keep], loop]), torch.cat([col[keep], loop])
    deg = torch.bincount(col, minlength=num_nodes).to(torch.float32)
    dis = deg.pow(-0.5)
    dis[torch.isinf(dis)] = 0
    w = dis[row] * dis[col]
    if rows is not None:
        rows = rows.to(torch.int64).to(row.device)
        inv = torch.full((num_nodes,), -1, dtype=torch.int64, device=row.device)
        inv[rows] = torch.arange(rows.numel(), device=row.device)
        sel = inv[col] >= 0
        row_s, col_s, w_s = row[sel], inv[col[sel]], w[sel]
        n_s = int(rows.numel())
        return ops.AggGraph(build_gather_plan(col_s, row_s, n_s, num_nodes, w_s, chunk, 'pp.fwd.rows', G),
                            build_gather_plan(row_s, col_s, num_nodes, n_s, w_s, chunk, 'pp.bwd.rows', G))
    return ops.AggGraph(build_gather_plan(col, row, num_nodes, num_nodes, w, chunk, 'pp.fwd', G),
                        build_gather_plan(row, col, num_nodes, num_nodes, w, chunk, 'pp.bwd', G))


class GCNConv(nn.Module):
    """out = A_hat (x W^T) + bias.  `cached` is accepted for signature parity; plans are always
    cached by edge-tensor identity."""

    def __init__(self, in_channels, out_channels, cached=False, bias=True, chunk=DEFAULT_CHUNK):
        super().__init__()
        self.in_channels, self.out_channels, self.cached, self.chunk = in_channels, out_channels, cached, chunk
        self.lin = _Lin(in_channels, out_channels)
        if bias:
            self.bias = Param(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        self._feat = _FeatureInput()
        self._cache = _PlanCache()
        self._cache_rows = _PlanCache()

    def aggregates_first(self, x, rows):
        """True if forward(x, ..., rows=rows) takes the aggregate-first route (the only one that honours gate_input)."""
        return rows is not None and not x.is_sparse and not _is_identity_features(x) and \
            ops.gather_sum_lin_supported(self.in_channels, self.out_channels, group_slots_for(self.in_channels))

    def forward(self, x, edge_index, fuse_relu=False, rows=None, gate_input=False, link=None):
        """rows (extension): ascending int64 node ids -- return only these rows of the layer's output, [len(rows), out]
        (`gcn_norm_graph(rows=...)`: the rows nobody reads are neither aggregated nor back-propagated through).
        fuse_relu='gated_downstream' / gate_input / link (extension, `ops.GateLink`): the ReLU hand-over between this layer
        and the ONE consumer of its output (FMEncoder: conv1 -> conv2)."""
        n = x.shape[0]
        if gate_input and not self.aggregates_first(x, rows):
            raise NotImplementedError('gate_input is wired for the aggregate-first route only')
        if self.aggregates_first(x, rows):
            # few rows kept: aggregate first, the dense map on the kept rows in the gather's own launch (ops._GCNConvAggFirst);
            # the plans move rows of in_channels floats
            graph = self._cache_rows.get((edge_index, rows),
                                         lambda: gcn_norm_graph(edge_index, n, self.chunk, self.in_channels, rows))
            return ops.gcn_conv_agg_first(x, self.lin.weight, self.bias, graph, fuse_relu, gate_input, link)
        if rows is not None:
            graph = self._cache_rows.get((edge_index, rows), lambda: gcn_norm_graph(edge_index, n, self.chunk, self.out_channels, rows))
        else:
            graph = self._cache.get((edge_index,), lambda: gcn_norm_graph(edge_index, n, self.chunk, self.out_channels))
        if _is_identity_features(x):
            return ops.gcn_conv(None, self.lin.weight, self.bias, graph, fuse_relu, link)      # lin(I) = W^T
        if x.is_sparse:
            xl = self._feat.apply_table(x, ops.linear_t(None, self.lin.weight))
            return ops.aggregate(xl, graph, bias=self.bias, relu=fuse_relu)
        return ops.gcn_conv(x, self.lin.weight, self.bias, graph, fuse_relu, link)

    def __repr__(self):
        return 'GCNConv(%d, %d)' % (self.in_channels, self.out_channels)


class PPEncoder(nn.Module):
    def __init__(self, in_dim, hid1=32, hid2=16):
        super().__init__()
        self.out_dim = hid2
        self.conv1 = GCNConv(in_dim, hid1, cached=True)
        self.conv2 = GCNConv(hid1, hid2, cached=True)

    def forward(self, x, edge_index):
        x = self.conv1(x, edge_index, fuse_relu=True)                # ReLU fused into the epilogue
        return self.conv2(x, edge_index)


# ---------------------------------------------------------------------------------------------
# A2  MyHierarchyConv   (src/layers.py:196-247)
# ---------------------------------------------------------------------------------------------
def hier_graph(edge_index, n_all, n_source, chunk=DEFAULT_CHUNK, table_rows=None, d=None):
    """mean over incoming edges in the concatenated node space, rows [n_source:] only.
    table_rows: rows of the table actually handed to the kernel (n_all for the concatenated
    tensor, n_source when only the source block is passed and no edge starts beyond it)."""
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    keep = dst >= n_source
    src, dst = src[keep], dst[keep] - n_source
    n_t = n_all - n_source
    n_tab = n_all if table_rows is None else table_rows
    cnt = torch.bincount(dst, minlength=n_t).to(torch.float32).clamp_(min=1)
    G = group_slots_for(d) if d else 0
    scale = (1.0 / cnt).contiguous()
    # the transposed plan carries 1/count as per-edge weights: no scaling pass before the backward gather
    graph = ops.AggGraph(build_gather_plan(dst, src, n_t, n_tab, None, chunk, 'pd.fwd', G),
                         build_gather_plan(src, dst, n_tab, n_t, scale[dst], chunk, 'pd.bwd', G), scale,
                         bwd_scaled=True)
    # CSR by target (edge order kept inside a target) for the fused P -> D + drug-mix forward launch (ops.drug_mix_gather;
    # include/tipk.h section 3)
    i32 = lambda t: t.to(torch.int32).contiguous()
    of = torch.sort(dst, stable=True).indices
    ptr = lambda idx, n: i32(torch.cat([idx.new_zeros(1), torch.cumsum(torch.bincount(idx, minlength=n), 0)]))
    # workgroups of the forward launch (16 wavefronts): targets dealt by edge count -- one with more than 512 edges has a
    # workgroup to itself (W = 16 wavefronts on it: one BioSNAP drug has 2 834 protein targets), those with 65 ... 512 edges go
    # four to a workgroup (W = 4), the others sixteen (a wavefront each); desc = {first index into `order`, n | W << 8}
    order, wgs = drug_workgroups(torch.bincount(dst, minlength=n_t))
    fwd_wg = torch.tensor(wgs, dtype=torch.int32, device=src.device).view(-1, 2).contiguous()
    # (no edge ends at a target: an empty tensor has no address and the launchers refuse a NULL list -- one unread element)
    some = lambda t: t if t.numel() else t.new_zeros(1)
    graph.pd_csr = dict(fwd_ptr=ptr(dst, n_t), fwd_src=some(i32(src[of])), scale=scale, fwd_wg=fwd_wg, fwd_order=i32(order), n_src=int(n_tab),
                        n_edges=int(src.numel()))
    # CSR by SOURCE row (edge order kept inside a row) with 1 / count of the edge's target: the transposed gather inside the
    # fused backward launch of the stage (tipk_pd_stage_bwd, tip_amd/encoder.py)
    ot = torch.sort(src, stable=True).indices
    graph.pd_csr.update(t_ptr=ptr(src, n_tab), t_dst=some(i32(dst[ot])), t_w=some(scale[dst[ot]].contiguous()))
    # ... and the deal of the source rows to that launch's workgroups: consecutive rows, at most max_rows of them and at most
    # max_edges edges (a row with more edges than that has a workgroup to itself)
    if src.is_cuda:
        import ctypes
        mr, me = ctypes.c_int(0), ctypes.c_int(0)
        ops.lib().tipk_pd_stage_bwd_limits(ctypes.byref(mr), ctypes.byref(me))
        bounds = deal_rows_by_edges(torch.bincount(src, minlength=n_tab).tolist(), mr.value, me.value)
        graph.pd_csr['t_wg'] = torch.tensor(bounds, dtype=torch.int32, device=src.device)
    return graph


def deal_rows_by_edges(counts, max_rows, max_edges):
    """Boundaries [0, ..., len(counts)] of consecutive row blocks with at most max_rows rows and -- unless a single row alone has
    more -- at most max_edges edges each (the row workgroups of tipk_pd_stage_bwd).  BioSNAP's P -> D graph has ~100 consecutive
    proteins that 65 ... 94 drugs target: blocks of 64 ROWS gave three workgroups 2 200 ... 3 300 edges against a mean of 326."""
    bounds, rows_in, edges_in = [0], 0, 0
    for r_, c_ in enumerate(counts):
        if rows_in and (rows_in == max_rows or edges_in + c_ > max_edges):
            bounds.append(r_)
            rows_in, edges_in = 0, 0
        rows_in += 1
        edges_in += c_
    bounds.append(len(counts))
    return bounds


def drug_workgroups(counts):
    """(order, descs) of the forward P -> D launch: rows by decreasing edge count; desc = [first index into order, n | W << 8] --
    a row with more than 512 edges alone on the 16 wavefronts of a workgroup (W = 16), rows with 65 ... 512 edges four to a
    workgroup (W = 4), the others sixteen (W = 1).  Every row exactly once."""
    cnt_t = torch.as_tensor(counts)
    n_t = int(cnt_t.numel())
    order = torch.sort(cnt_t, descending=True, stable=True).indices
    cs = cnt_t[order].tolist()
    n_big = sum(1 for c_ in cs if c_ > 512)
    n_mid = sum(1 for c_ in cs if 64 < c_ <= 512)
    wgs = [[i, 1 | (16 << 8)] for i in range(n_big)]
    wgs += [[b0, min(4, n_big + n_mid - b0) | (4 << 8)] for b0 in range(n_big, n_big + n_mid, 4)]
    wgs += [[b0, min(16, n_t - b0) | (1 << 8)] for b0 in range(n_big + n_mid, n_t, 16)]
    return order, wgs


class MyHierarchyConv(nn.Module):
    """Directed protein -> drug mean aggregation followed by a dense map."""

    def __init__(self, in_dim, out_dim, unigue_source_num, unique_target_num,
                 is_after_relu=True, is_bias=False, chunk=DEFAULT_CHUNK):
        super().__init__()
        self.in_dim, self.out_dim = in_dim, out_dim
        self.unique_source_num, self.unique_target_num = unigue_source_num, unique_target_num
        self.is_after_relu, self.chunk = is_after_relu, chunk
        self.weight = Param(torch.empty(in_dim, out_dim))
        if is_bias:
            # the reference's bias branch cannot run (`if self.bias:` on a tensor, and an
            # out_dim-sized bias added to in_dim-wide rows, :236-237); every caller passes False
            raise NotImplementedError('MyHierarchyConv(is_bias=True) is not executable in the reference either')
        self.register_parameter('bias', None)
        self._cache = _PlanCache()
        self._cache_src = _PlanCache()
        self._cache_src_rows = _PlanCache()
        self._cache_rows = _PlanCache()
        self.reset_parameters()

    def reset_parameters(self):
        scale = 1.0 if self.is_after_relu else 2.0
        self.weight.data.normal_(std=scale / np.sqrt(self.in_dim))

    def forward(self, x, edge_index, range_list=None):
        n_all = x.shape[0]
        graph = self._cache.get((edge_index,), lambda: hier_graph(edge_index, n_all, self.unique_source_num,
                                                                  self.chunk, d=self.in_dim))
        mean = ops.aggregate(x, graph)
        out = ops.matmul(mean, self.weight)
        assert out.shape[0] == self.unique_target_num
        return out

    def forward_sources(self, x_src, edge_index):
        """Same result as `forward(cat(x_src, zeros[n_target]), edge_index, ...)` without building
        the concatenation (the reference's zero rows `hdrug`, :526, are never read when every edge
        starts at a source node).  Returns None if some edge starts beyond the source block."""
        n_src = self.unique_source_num
        n_all = n_src + self.unique_target_num

        def build():
            if edge_index.numel() and int(edge_index[0].max()) >= n_src:
                return None
            return hier_graph(edge_index, n_all, n_src, self.chunk, table_rows=n_src, d=self.in_dim)
        graph = self._cache_src.get((edge_index,), build)
        if graph is None:
            return None
        return ops.matmul(ops.aggregate(x_src, graph), self.weight)

    def source_rows(self, edge_index):
        """Ascending ids of the source nodes some edge starts at (the only rows of the source block the mean reads), or
        None if an edge starts beyond the source block.  Cached per edge tensor."""
        n_src = self.unique_source_num

        def build():
            if edge_index.numel() and int(edge_index[0].max()) >= n_src:
                return None
            return torch.unique(edge_index[0].to(torch.int64))
        return self._cache_rows.get((edge_index,), build)

    def mean_sources(self, x_src, edge_index, rows=None, graph_only=False):
        """The mean aggregate of `forward_sources` WITHOUT the dense map (the caller applies
        `self.weight` fused with what follows, ops.drug_mix_mm); None if unusable.
        rows: `source_rows(edge_index)` -- x_src then holds only those rows of the source block, in that order."""
        n_src = self.unique_source_num
        n_all = n_src + self.unique_target_num

        def build():
            if edge_index.numel() and int(edge_index[0].max()) >= n_src:
                return None
            if rows is None:
                return hier_graph(edge_index, n_all, n_src, self.chunk, table_rows=n_src, d=self.in_dim)
            inv = torch.full((n_src,), -1, dtype=torch.int64, device=edge_index.device)
            inv[rows] = torch.arange(rows.numel(), device=edge_index.device)
            src = inv[edge_index[0].to(torch.int64)]
            assert bool((src >= 0).all())
            n_c = int(rows.numel())                                        # compact source block + the targets behind it
            ei = torch.stack([src, edge_index[1].to(torch.int64) - n_src + n_c])
            return hier_graph(ei, n_c + self.unique_target_num, n_c, self.chunk, table_rows=n_c, d=self.in_dim)
        graph = (self._cache_src if rows is None else self._cache_src_rows).get((edge_index, rows), build)
        if graph is None:
            return None
        if graph_only:
            return graph
        return ops.aggregate(x_src, graph)

    def __repr__(self):
        return 'MyHierarchyConv(%d, %d)' % (self.in_dim, self.out_dim)


# ---------------------------------------------------------------------------------------------
# A4/A5  R-GCN layers   (src/layers.py:21-99, :102-193)
# ---------------------------------------------------------------------------------------------
def relation_of_edges(range_list, n_edges, device):
    rg = torch.as_tensor(range_list).to(torch.int64).cpu()
    if rg.numel() == 0:                                       # a rank without relations (more ranks than relations)
        if n_edges:
            raise ValueError('empty range_list for %d edges' % n_edges)
        return torch.zeros(0, dtype=torch.int64, device=device)
    sizes = rg[:, 1] - rg[:, 0]
    if not (int(sizes.sum()) == n_edges and int(rg[0, 0]) == 0 and bool((rg[1:, 0] == rg[:-1, 1]).all())):
        raise ValueError('range_list must be consecutive blocks covering all %d edges' % n_edges)
    return torch.repeat_interleave(torch.arange(rg.shape[0]), sizes).to(device)


def _shared_pair_bwd_plan(src, dst, rel, n_nodes, n_rel, scale, symmetric, n_wg, lanes, share=None):
    """`build_pair_bwd_plan`; the R-GCN layers of one model run on the same graph and share the plan (it does not depend on the
    layer's width).  share = (dict owned by the model, (edge_index, range_list) as the caller passed them): the dict holds the
    layers' one `DerivedCache` (two entries: a training and an evaluation graph), whose entry keeps those tensors alive, so
    their identity + version IS the edge list -- no checksums, no device sync, nothing global."""
    build = lambda: build_pair_bwd_plan(src, dst, rel, n_nodes, n_rel, scale, symmetric, n_wg, lanes, ops.rel_stream_piece())
    if share is None:
        return build()
    owned, owners = share
    cache = owned.get('pair_bwd')
    if cache is None:
        cache = owned['pair_bwd'] = DerivedCache(2)
    return cache.get(tuple(t if torch.is_tensor(t) else None for t in owners),
                     (int(n_nodes), int(n_rel), bool(symmetric), int(n_wg), int(lanes)), build)


def pair_link_words(src, dst, n_nodes):
    """uint32 words (as int32) [n_nodes padded to 8][ceil(n_nodes / 32)]: bit r of word (u, t) = some edge links u -> 32 t + r."""
    n8, n32 = -(-n_nodes // 8) * 8, -(-n_nodes // 32) * 32
    link = torch.zeros((n8, n32), dtype=torch.bool, device=src.device)
    link[src, dst] = True
    w = (link.view(n8, n32 // 32, 32).to(torch.int64) << torch.arange(32, device=src.device).view(1, 1, 32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def rgcn_graph(edge_index, rel, n_nodes, n_rel, chunk=DEFAULT_CHUNK, in_degree=None, d_out=None, n_bases=None, paired=False,
               plan_share=None):
    """fwd: destination <- row (rel*N + src) of Y;  bwd: (rel*N + src) <- destination row of g;
    scale = 1 / max(1, in-degree over ALL relations) (torch-scatter 'mean').  `in_degree`: [N]
    in-degree of the WHOLE graph when `edge_index` is only one rank's shard (tip_amd/dist.py)."""
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    rel = rel.to(torch.int64)
    if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= n_rel):
        raise IndexError('edge_type out of range')
    yrow = rel * n_nodes + src
    if in_degree is None:
        deg = torch.bincount(dst, minlength=n_nodes).to(torch.float32).clamp_(min=1)
    else:
        assert in_degree.numel() == n_nodes
        deg = in_degree.to(src.device).to(torch.float32).clamp_(min=1)
    rl_fwd = rl_bwd = rs_bwd = pair_fwd = pair_bwd = None
    if n_nodes <= 1024 and n_rel > 0 and src.numel() > 0:
        # relation-local plans for the LDS-resident kernels (used when a relation's table fits in LDS)
        n_cu = torch.cuda.get_device_properties(src.device).multi_processor_count if src.is_cuda else 256
        on_dev = bool(d_out and src.is_cuda)
        # workgroups of the pair-form gathers PER LAYER.  paired: the layer is one of the two of an FMEncoder, which gathers both
        # layers' cells, and both layers' d att, in one launch each (tip_amd/encoder.py) -- 2 x (CUs / 2) workgroups are one round
        # of the chip (140 KB of LDS: one workgroup per CU); with CUs per layer every CU staged its table twice (25.2 -> 21.1 us
        # and 28.0 -> 24.4 us at BioSNAP).  A layer on its own fills the chip by itself.  TIPK_PAIR_WGS: experiments
        pair_wgs = int(os.environ.get('TIPK_PAIR_WGS', 0)) or (max(1, n_cu // 2) if paired else n_cu)
        # launch = (workgroups x column blocks), sized for 1 or 2 workgroups per CU (tipk_rel_gather_occupancy)
        wg_f = (ops.rel_gather_wgs(n_nodes, d_out, False, n_cu) if on_dev else 0) or n_cu
        wg_b = (ops.rel_gather_wgs(n_nodes, d_out, True, n_cu) if on_dev else 0) or n_cu
        # lanes per slot of the launch (columns of one column block / 4): the plans order every run for
        # conflict-free LDS reads of that shape and pre-scale the ids to row offsets
        split_f = ops.rel_gather_split(n_nodes, d_out, False) if on_dev else 0
        split_b = ops.rel_gather_split(n_nodes, d_out, True) if on_dev else 0
        lanes_f = (d_out // split_f) // 4 if split_f else None
        lanes_b = (d_out // split_b) // 4 if split_b else None
        cap_f = None           # (cutting forward units to the id chunk was measured slower: smaller units fill fewer bands)
        rl_fwd = lambda: build_rel_plan(dst, src, rel, n_nodes, n_rel, wg_f, lanes=lanes_f, unit_cap=cap_f)
        # forward pass in pair form: cells (source, destination) <- sums of att rows (LDS-resident att table)
        split_p = ops.stream_gather_split(n_rel, n_bases) if on_dev and n_bases and n_nodes * n_nodes < 2 ** 24 else 0
        if split_p:
            # every relation symmetric (u -> v iff v -> u: BioSNAP) => cell (u, v) == cell (v, u): build the cells
            # with u <= v only, from half the edges; the product reads the mirrored ones at their transposed place
            k_fw = torch.sort((rel * n_nodes + src) * n_nodes + dst).values
            k_bw = torch.sort((rel * n_nodes + dst) * n_nodes + src).values
            symmetric = bool(torch.equal(k_fw, k_bw)) and bool(ops.lib().tipk_pair_product_supported(n_bases, d_out))
            keep = src <= dst if symmetric else torch.ones_like(src, dtype=torch.bool)
            pair_fwd = build_stream_plan_rows(src[keep] * n_nodes + dst[keep], rel[keep], n_nodes * n_nodes, n_rel, pair_wgs,
                                              (n_bases // split_p) // 4, ops.rel_stream_piece())
            pair_fwd.symmetric = symmetric
            # which pairs are linked at all, one bit per (source, destination): the product fetches only their cells
            # (uint32 [sources padded to 8][ceil(N / 32)], bit r of word (u, t) = pair (u, 32 t + r); tipk.h section 2c `links`)
            pair_fwd.links = pair_link_words(src, dst, n_nodes)
        # transposed pass: wave streams (no work units, no barriers) when g' fits in LDS, else relation-local units
        split_s = ops.rel_stream_split(n_nodes, d_out) if on_dev and n_rel * n_nodes < 2 ** 24 else 0
        if pair_fwd is not None and ops.pair_grads_supported(n_bases, d_out):
            # backward pass in pair form as well (round 5): the cells of the forward pass + one 128-byte gradient row per
            # linked pair; d att walks half the edges of a symmetric graph.  The plan does not depend on the layer's width:
            # the layers of a model share it.  Its d att gather stages 128-byte gradient rows in ONE column block (8 lanes a row,
            # what tipk_stream_gather_parts launches), whatever split the att table of the cell gather needs
            sym, lanes_p = pair_fwd.symmetric, n_bases // 4
            pair_bwd = lambda: _shared_pair_bwd_plan(src, dst, rel, n_nodes, n_rel, 1.0 / deg, sym, pair_wgs, lanes_p, plan_share)
        if split_s:
            # compact node-major rows when the products of dY can run on them (tipk_rgcn_node_products); with the pair-form
            # backward pass the plan is only built if some pass asks for it (a forward pass on the Y route of a sharded run)
            compact = bool(n_bases) and ops.node_products_slabs(n_nodes, d_out, n_rel, n_bases) > 0
            lanes_s = (d_out // split_s) // 4
            build_rs = lambda: build_stream_plan(src, dst, rel, n_nodes, n_rel, n_cu, lanes_s, ops.rel_stream_piece(), compact=compact)
            rs_bwd = build_rs if pair_bwd is not None else build_rs()
        else:
            rl_bwd = lambda: build_rel_plan(src, dst, rel, n_nodes, n_rel, wg_b, backward=True, lanes=lanes_b)
    # forward pass of LARGE node sets without Y (tipk_rgcn_dest_products): where Y = [R N, d_out] would not stay in the
    # Infinity Cache (config 5: 10 GB) and neither LDS route applies
    dest_fwd = row_fwd = row_bwd = None
    wide = False
    if src.is_cuda and d_out and n_bases and pair_fwd is None and n_rel * n_nodes * d_out * 4 > (192 << 20):
        bits = ops.dest_products_bits(n_nodes, n_rel, n_bases, 1)
        if bits:
            dest_fwd = lambda: build_dest_plan(src, dst, rel, n_nodes, n_rel, bits)
        # row sums assembled in LDS (tipk_rgcn_row_products): rows (relation, destination) <- sources for the forward pass,
        # rows (relation, source) <- destinations for the transposed pass.  Widths that are multiples of 64 take the
        # wave-uniform form (tipk_rgcn_row_products_s: any node count whose table stays below 2 GB); other multiples of 32 the
        # per-lane form (<= 65 536 nodes: a 16-bit node field in the entry word).  A plan is installed only where the
        # matching `_supported` query passes for THIS node count: the passes test `graph.row_fwd is not None`
        wide = bool(d_out) and d_out % 64 == 0 and ops.row_products_s_supported(n_nodes, n_rel, n_bases, d_out) \
            and n_nodes < (1 << 23) and n_nodes * d_out * 4 < 2 ** 31
        if wide:
            row_fwd = lambda: build_row_stream_plan_s(dst, src, rel, n_nodes, n_rel)
            row_bwd = lambda: build_row_stream_plan_s(src, dst, rel, n_nodes, n_rel)
        elif ops.row_products_supported(n_nodes, n_rel, n_bases, 32):
            row_fwd = lambda: build_row_stream_plan(dst, src, rel, n_nodes, n_rel)
            row_bwd = lambda: build_row_stream_plan(src, dst, rel, n_nodes, n_rel)

    def fwd_plan():
        # Y = [R N, d_out] beyond the Infinity Cache (config 5: 10 GB): launch the items relation block by
        # relation block, so that a row of Y gathered by several edges crosses the fabric once
        y_bytes = n_rel * n_nodes * (d_out or 0) * 4
        ordered = rel.numel() < 2 or bool((rel[1:] >= rel[:-1]).all())
        if y_bytes > (192 << 20) and ordered:
            per = relations_per_segment(n_nodes, d_out)
            return build_gather_plan_segmented(dst, yrow, rel // per, n_nodes, n_rel * n_nodes, chunk, 'dd.fwd')
        return build_gather_plan(dst, yrow, n_nodes, n_rel * n_nodes, None, chunk, 'dd.fwd')

    # the generic plans are built on first use: with the relation-local kernels they are never needed
    return ops.AggGraph(fwd_plan,
                        lambda: build_gather_plan(yrow, dst, n_rel * n_nodes, n_nodes, None, chunk, 'dd.bwd'),
                        (1.0 / deg).contiguous(), rl_fwd, rl_bwd,
                        csr_bwd=lambda: build_csr_plan(yrow, dst, n_rel * n_nodes, n_nodes, 'dd.bwd'), rs_bwd=rs_bwd,
                        pair_fwd=pair_fwd, pair_bwd=pair_bwd, dest_fwd=dest_fwd, row_fwd=row_fwd, row_bwd=row_bwd,
                        row_wave_uniform=wide)


class _RGCNBase(nn.Module):
    def __init__(self, in_channels, out_channels, num_relations, num_bases, after_relu, bias=False,
                 chunk=DEFAULT_CHUNK):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_relations, self.num_bases, self.after_relu, self.chunk = num_relations, num_bases, after_relu, chunk
        self.basis = Param(torch.empty(num_bases, in_channels, out_channels))
        self.att = Param(torch.empty(num_relations, num_bases))
        self.root = Param(torch.empty(in_channels, out_channels))
        if bias:
            self.bias = Param(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self._cache = _PlanCache()
        self.shard = None                       # tip_amd.dist.RelationShard for multi-GPU runs
        self.paired = False                     # one of the two layers of an FMEncoder (sizes the pair plans: rgcn_graph)
        self.plan_share = None                  # dict shared with the other layers on the same graph (pair backward plan)
        self.reset_parameters()

    def reset_parameters(self):
        self.att.data.normal_(std=1 / np.sqrt(self.num_bases))
        std = 2 / self.in_channels if self.after_relu else 1 / np.sqrt(self.in_channels)
        self.root.data.normal_(std=std)
        self.basis.data.normal_(std=std)
        if self.bias is not None:
            self.bias.data.zero_()

    def _global_degree(self):
        """in-degree over the relations of ALL ranks when this layer holds one shard of them."""
        return None if self.shard is None else self.shard.in_degree

    def _run(self, x, graph, fuse_relu=False, gate_input=False, defer_output=False, partner=None, cells_token=None):
        if self.bias is not None:
            out = ops.rgcn(x, self.basis, self.att, self.root, graph, self.shard) + self.bias
            if gate_input or fuse_relu == 'gated_downstream':
                raise NotImplementedError('ReLU-mask hand-over between layers is only wired for bias=False')
            return torch.relu(out) if fuse_relu else out
        return ops.rgcn(x, self.basis, self.att, self.root, graph, self.shard, relu=fuse_relu, gate_input=gate_input,
                        defer_output=defer_output, partner=partner, cells_token=cells_token)

    def __repr__(self):
        return '%s(%d, %d, num_relations=%d)' % (self.__class__.__name__, self.in_channels, self.out_channels,
                                                 self.num_relations)


class MyRGCNConv2(_RGCNBase):
    """Range-list variant (:102-193): relation r owns edges `range_list[r] = (start, end)`;
    `edge_type` is accepted and ignored, as in the reference."""

    def graph_for(self, n, edge_index, range_list):
        """The layer's cached plans of this D-D graph over n nodes (built on first use)."""
        def build():
            rel = relation_of_edges(range_list, edge_index.shape[1], edge_index.device)
            return rgcn_graph(edge_index, rel, n, self.num_relations, self.chunk, in_degree=self._global_degree(),
                              d_out=self.out_channels, n_bases=self.num_bases, paired=self.paired and self.shard is None,
                              plan_share=None if self.plan_share is None else (self.plan_share, (edge_index, range_list)))
        return self._cache.get((edge_index, range_list if torch.is_tensor(range_list) else None), build)

    def forward(self, x, edge_index, edge_type, range_list, fuse_relu=False, gate_input=False, defer_output=False, next_layer=None,
                cells_token=None):
        """`fuse_relu` (extension): apply the ReLU that follows the layer in FMEncoder
        (src/layers.py:547) inside the layer's last kernel; 'gated_downstream' additionally leaves
        the ReLU's backward mask to the one consumer, which is called with `gate_input=True`.
        `defer_output` (extension, only with 'gated_downstream'): the layer's final slab sum may be left to that consumer --
        an R-GCN layer of this package, which runs it in the launch of its own XB product; the returned tensor must not be
        read by anything else.
        `next_layer` (extension): the R-GCN layer that follows on the SAME graph -- its pair cells (they depend on its `att`
        alone) are gathered in this layer's cell launch."""
        n = x.shape[0]
        graph = self.graph_for(n, edge_index, range_list)
        partner = None
        if next_layer is not None and self.shard is None and next_layer.shard is None and next_layer.bias is None and \
                next_layer.num_relations == self.num_relations and next_layer.num_bases == self.num_bases:
            partner = (next_layer.att, next_layer.graph_for(n, edge_index, range_list), next_layer.out_channels, cells_token)
        return self._run(x, graph, fuse_relu, gate_input, defer_output, partner, cells_token if next_layer is None else None)

    def attribute(self, h, edge_index, range_list, q_node, probe, k):
        """Edge attribution (extension, `tipk_rgcn_attribution`): with z = this layer applied to h, the k in-edges of every
        node of q_node [Q] that contribute most to probe[q] . z[node] -> (contribution [Q, k], source int32 [Q, k], relation
        int32 [Q, k], own [Q], total [Q]) as `ops.rgcn_edge_attribution`; no autograd.  Exact only where nothing follows
        the layer's sum: a layer with a bias or a relation shard is refused."""
        if self.bias is not None or self.shard is not None:
            raise NotImplementedError('attribute splits the sum of a bias-free layer that holds every relation; this layer '
                                      'has a bias or a relation shard')
        in_edges = ops.in_edges_by_node(edge_index, range_list, h.shape[0])
        return ops.rgcn_edge_attribution(h.detach(), self.basis.detach(), self.att.detach(), self.root.detach(), in_edges,
                                         q_node, probe, k)


class MyRGCNConv(_RGCNBase):
    """Per-edge-type variant (:21-99): same arithmetic, relation id taken from `edge_type`; the
    reference gathers an E x in x out weight tensor here, this build needs no edge ordering."""

    def forward(self, x, edge_index, edge_type):
        n = x.shape[0]
        graph = self._cache.get((edge_index, edge_type),
                                lambda: rgcn_graph(edge_index, edge_type, n, self.num_relations, self.chunk,
                                                   in_degree=self._global_degree(), d_out=self.out_channels,
                                                   n_bases=self.num_bases))
        return self._run(x, graph)


# ---------------------------------------------------------------------------------------------
# A3 + composition  FMEncoder   (src/layers.py:471-553; FMEncoderCat :401-468 is its cat mode)
# ---------------------------------------------------------------------------------------------
class FMEncoder(nn.Module):
    def __init__(self, device, in_dim_drug, num_dd_et, in_dim_prot, uni_num_prot, uni_num_drug,
                 prot_drug_dim=64, num_base=32, n_embed=64, n_hid1=32, n_hid2=16, mod='cat'):
        super().__init__()
        assert mod in {'add', 'cat'}
        if mod == 'add':
            assert n_embed == prot_drug_dim
        self.num_et, self.out_dim, self.mod = num_dd_et, n_hid2, mod
        self.uni_num_drug, self.uni_num_prot = uni_num_drug, uni_num_prot
        self.pp_encoder = PPEncoder(in_dim_prot)
        self.embed = Param(torch.empty(in_dim_drug, n_embed))
        self.hgcn = MyHierarchyConv(self.pp_encoder.out_dim, prot_drug_dim, uni_num_prot, uni_num_drug)
        self.hdrug = torch.zeros((uni_num_drug, self.pp_encoder.out_dim), device=device)
        d_in = n_embed + self.hgcn.out_dim if mod == 'cat' else n_embed
        self.rgcn1 = MyRGCNConv2(d_in, n_hid1, num_dd_et, num_base, after_relu=False)
        self.rgcn2 = MyRGCNConv2(n_hid1, n_hid2, num_dd_et, num_base, after_relu=True)
        self.rgcn1.paired = self.rgcn2.paired = True
        self.rgcn1.plan_share = self.rgcn2.plan_share = {}
        self._drug_feat = _FeatureInput()
        self.prune_pp_rows = True               # conv2 of the P-P encoder only for the rows the P -> D stage reads (forward())
        self.reset_parameters()

    def reset_parameters(self):
        self.embed.data.normal_()

    def fused_plans(self, x_drug, dd_edge_index, dd_range_list, d_norm, x_prot, pp_edge_index, dp_edge_index):
        """(xd, encoder.EncoderPlans) if this call can run as ONE autograd node with its own launch schedule
        (tip_amd/encoder.py: identity protein features, pruned conv2, pair-form D-D graph on both layers, no relation
        sharding), else None.  The graphs are the layers' own cached plans: both routes build and share the same ones."""
        if switches.on('TIPK_NO_ENCODER_STEP') or not self.prune_pp_rows or not _is_identity_features(x_prot):
            return None
        r1, r2 = self.rgcn1, self.rgcn2
        if r1.shard is not None or r2.shard is not None or r1.bias is not None or r2.bias is not None:
            return None
        if not (torch.is_tensor(d_norm) and d_norm.is_cuda and self.embed.is_cuda):
            return None
        rows = self.hgcn.source_rows(dp_edge_index)
        n_prot = x_prot.shape[0]
        if rows is None or rows.numel() >= n_prot or rows.numel() == 0:
            return None
        c1, c2 = self.pp_encoder.conv1, self.pp_encoder.conv2
        pd = self.hgcn.mean_sources(None, dp_edge_index, rows=rows, graph_only=True)
        if pd is None:
            return None
        xd = self._drug_feat.apply_table(x_drug, self.embed)
        n = xd.shape[0]
        pp = c1._cache.get((pp_edge_index,), lambda: gcn_norm_graph(pp_edge_index, n_prot, c1.chunk, c1.out_channels))
        pp_rows = c2._cache_rows.get((pp_edge_index, rows), lambda: gcn_norm_graph(pp_edge_index, n_prot, c2.chunk, c2.in_channels, rows))
        plans = encoder.EncoderPlans(pp, pp_rows, pd, r1.graph_for(n, dd_edge_index, dd_range_list),
                                     r2.graph_for(n, dd_edge_index, dd_range_list), self.mod == 'cat')
        if not encoder.usable(plans, xd, self.hgcn.weight, d_norm, c2.lin.weight, c1.bias, c2.bias, r1.basis, r1.att, r2.basis, r2.att):
            return None
        return xd, plans

    def forward(self, x_drug, dd_edge_index, dd_edge_type, dd_range_list, d_norm,
                x_prot, pp_edge_index, dp_edge_index, dp_range_list):
        fused = self.fused_plans(x_drug, dd_edge_index, dd_range_list, d_norm, x_prot, pp_edge_index, dp_edge_index)
        self.last_route = 'encoder_step' if fused is not None else 'per_layer'      # (bench.py / tests read it)
        if fused is not None:
            # the whole pass as one autograd node: 8 + 8 launches, scheduled by tip_amd/encoder.py
            c1, c2, r1, r2 = self.pp_encoder.conv1, self.pp_encoder.conv2, self.rgcn1, self.rgcn2
            return encoder.encoder_step(fused[0], c1.lin.weight, c1.bias, c2.lin.weight, c2.bias, self.hgcn.weight, d_norm,
                                        r1.basis, r1.att, r1.root, r2.basis, r2.att, r2.root, fused[1])
        x0 = self.mixed_drug_features(x_drug, d_norm, x_prot, pp_edge_index, dp_edge_index, dp_range_list)
        # ReLU (:547) is applied by rgcn1's last kernel and its backward mask by rgcn2's (x1 has no other consumer)
        # ... and its final slab sum runs in rgcn2's first launch, together with rgcn2's XB / X root products
        # rgcn2's pair cells ride in rgcn1's cell launch
        tok = object()                                         # "rgcn1 gathered rgcn2's cells in THIS pass"
        x1 = self.rgcn1(x0, dd_edge_index, dd_edge_type, dd_range_list, fuse_relu='gated_downstream', defer_output=True,
                        next_layer=self.rgcn2, cells_token=tok)
        return self.rgcn2(x1, dd_edge_index, dd_edge_type, dd_range_list, gate_input=True, cells_token=tok)

    def encode_layers(self, x_drug, dd_edge_index, dd_edge_type, dd_range_list, d_norm,
                      x_prot, pp_edge_index, dp_edge_index, dp_range_list):
        """`forward`'s arguments -> (h, z) under no_grad: h = relu(rgcn1(x0)), the input of the last layer, and z = rgcn2(h),
        the embeddings, layer by layer (what `TIP.explain` splits).  z equals `forward`'s result up to the rounding between
        the per-layer and the fused route."""
        with torch.no_grad():
            x0 = self.mixed_drug_features(x_drug, d_norm, x_prot, pp_edge_index, dp_edge_index, dp_range_list)
            h = self.rgcn1(x0, dd_edge_index, dd_edge_type, dd_range_list, fuse_relu=True)
            return h, self.rgcn2(h, dd_edge_index, dd_edge_type, dd_range_list)

    def fold_in_tables(self, x_drug, dd_edge_index, dd_edge_type, dd_range_list, d_norm,
                       x_prot, pp_edge_index, dp_edge_index, dp_range_list):
        """`forward`'s arguments -> (h_prot_all, x0, h) under no_grad: the tables a drug outside the graph is embedded from
        (`ops.drug_fold_in`, `TIP.embed_new_drugs`).  h_prot_all: the P-P encoder's output for EVERY protein (the un-pruned
        `PPEncoder.forward`: a new drug may target a protein no training drug targets); x0: the mixed drug features; h =
        relu(rgcn1(x0)), the input of the last layer."""
        with torch.no_grad():
            h_prot_all = self.pp_encoder(x_prot, pp_edge_index)
            x0 = self.mixed_drug_features(x_drug, d_norm, x_prot, pp_edge_index, dp_edge_index, dp_range_list)
            return h_prot_all, x0, self.rgcn1(x0, dd_edge_index, dd_edge_type, dd_range_list, fuse_relu=True)

    def mixed_drug_features(self, x_drug, d_norm, x_prot, pp_edge_index, dp_edge_index, dp_range_list):
        """The input of the D-D layers (src/layers.py:522-539): P-P GCN x2 -> P -> D mean -> dense map, drug embedding /
        d_norm, cat | add.  (The part of the step a relation-sharded run repeats on every rank.)"""
        xd = self._drug_feat.apply_table(x_drug, self.embed)                          # x_drug @ embed
        # Only the proteins some P -> D edge starts at are ever read from the P-P encoder's output (BioSNAP: 3 640 of
        # 19 081; 294 k of its 1.29 M edges end there): conv2 aggregates -- and back-propagates through -- those rows only.
        # Exact: the rows left out feed nothing.  `PPEncoder.forward` as a module of its own still returns every row.
        rows = self.hgcn.source_rows(dp_edge_index) if self.prune_pp_rows else None
        if rows is not None and rows.numel() < x_prot.shape[0]:
            c1, c2 = self.pp_encoder.conv1, self.pp_encoder.conv2
            g_in = group_slots_for(c2.in_channels)
            if (_is_identity_features(x_prot) or not x_prot.is_sparse) and \
                    ops.gather_sum_lin_supported(c2.in_channels, c2.out_channels, g_in) and \
                    ops.lib().tipk_gather_sum_riders_supported(c2.in_channels, g_in):
                # conv2 runs aggregate-first and its transposed aggregation has 1024-thread workgroups: conv1's ReLU backward
                # and the partial rows of conv1's bias gradient are produced in THAT launch's epilogue (h1 has no other consumer)
                link = ops.GateLink() if c1.bias is not None else None
                h1 = c1(x_prot, pp_edge_index, fuse_relu='gated_downstream', link=link)
                # conv2 + the P -> D stage as ONE node with the fused launches of tip_amd/encoder.py where they apply (round 6:
                # what a relation-sharded run repeats on every rank takes 3 + 2 launches instead of 3 + 4)
                pd_g = self.hgcn.mean_sources(None, dp_edge_index, rows=rows, graph_only=True)
                n_p = x_prot.shape[0]
                g_rows = c2._cache_rows.get((pp_edge_index, rows), lambda: gcn_norm_graph(pp_edge_index, n_p, c2.chunk, c2.in_channels, rows))
                if not switches.on('TIPK_NO_ENCODER_STEP') and torch.is_tensor(d_norm) and \
                        encoder.pd_stage_usable(g_rows, pd_g, xd, self.hgcn.weight, d_norm, c2.lin.weight, c2.bias):
                    return encoder.pd_stage(h1, c2.lin.weight, c2.bias, xd, self.hgcn.weight, d_norm, g_rows, pd_g, self.mod == 'cat', link)
                h_prot = c2(h1, pp_edge_index, rows=rows, gate_input=True, link=link)     # [len(rows), hid2]
            else:
                h1 = c1(x_prot, pp_edge_index, fuse_relu=True)
                h_prot = c2(h1, pp_edge_index, rows=rows)                                  # [len(rows), hid2]
        else:
            rows = None
            h_prot = self.pp_encoder(x_prot, pp_edge_index)                           # P-P GCN x2
        pd_graph = self.hgcn.mean_sources(None, dp_edge_index, rows=rows, graph_only=True)
        if pd_graph is not None and ops.drug_mix_gather_supported(h_prot, self.hgcn.weight, d_norm):
            # P -> D mean, dense map, /d_norm and cat | add: ONE launch forward (tipk_drug_mix_gather_fwd), two backward
            x0 = ops.drug_mix_gather(xd, h_prot, self.hgcn.weight, d_norm, self.mod == 'cat', pd_graph)
            mean = None
        else:
            mean = self.hgcn.mean_sources(h_prot, dp_edge_index, rows=rows)           # P -> D mean, no cat (:526-528)
            x0 = None
        if x0 is not None:
            pass
        elif mean is not None:                                                        # dense map + /d_norm + cat|add fused
            x0 = ops.drug_mix_mm(xd, mean, self.hgcn.weight, d_norm, self.mod == 'cat')
        else:                                                                         # an edge starts at a drug row
            if self.hdrug.device != h_prot.device:
                self.hdrug = self.hdrug.to(h_prot.device)
            pd = self.hgcn(torch.cat((h_prot, self.hdrug)), dp_edge_index, dp_range_list)
            x0 = ops.drug_mix(xd, pd, d_norm, self.mod == 'cat')                      # /d_norm, cat|add
        return x0


class FMEncoderCat(FMEncoder):
    """cat-only constructor signature of `src/layers.py:403-405`."""

    def __init__(self, device, in_dim_drug, num_dd_et, in_dim_prot, uni_num_prot, uni_num_drug,
                 prot_drug_dim=16, num_base=32, n_embed=48, n_hid1=32, n_hid2=16):
        super().__init__(device, in_dim_drug, num_dd_et, in_dim_prot, uni_num_prot, uni_num_drug,
                         prot_drug_dim, num_base, n_embed, n_hid1, n_hid2, mod='cat')


# ---------------------------------------------------------------------------------------------
# A6  DistMult decoder   (src/layers.py:581-595)
# ---------------------------------------------------------------------------------------------
class MultiInnerProductDecoder(nn.Module):
    def __init__(self, in_dim, num_et):
        super().__init__()
        self.num_et, self.in_dim = num_et, in_dim
        self.weight = Param(torch.empty(num_et, in_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.weight.data.normal_(std=1 / np.sqrt(self.in_dim))

    def forward(self, z, edge_index, edge_type, sigmoid=True):
        return ops.distmult(z, self.weight, edge_index, edge_type, sigmoid)

    def objective(self, z, pos_index, neg_index, edge_type):
        """-mean log(sigma(pos)+eps) - mean log(1-sigma(neg)+eps), fused (K9+K10)."""
        return ops.distmult_objective(z, self.weight, pos_index, neg_index, edge_type)

    def probe(self, z, edge_index, edge_type, side='v'):
        """The logit of every triple (u, v, r) as a linear function of ONE drug's embedding (extension, `TIP.explain`) ->
        (node int64 [T], probe [T, in_dim], offset [T]) with logit = offset + probe . z[node]: side 'v' explains v with
        probe = z[u] * weight[r], side 'u' explains u with probe = z[v] * weight[r]; the offset is 0 (DistMult is bilinear).
        Plain torch ops under no_grad."""
        with torch.no_grad():
            u, v = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
            node, other = (v, u) if side == 'v' else (u, v)
            g = z.detach()[other] * self.weight.detach()[edge_type]
            return node, g, g.new_zeros(g.shape[0])

    def _rows(self, relations=None):
        """The weight rows the queries rank with, detached: all, or those of the candidate ids `relations`."""
        w = self.weight.detach()
        return w if relations is None else w[relations]

    def screen(self, z, k, relations=None, drugs=None, known=None):
        """Screen (extension, `tipk_distmult_screen`): the k best candidates per query by LOGIT -> (logits [Q, k],
        u int32 [Q, k], v int32 [Q, k]); no autograd.  relations: ids (None = all num_et).  drugs None: one relation query
        per relation (all pairs u < v); drugs given: one drug query per (drug, relation), DRUG-MAJOR -- row
        i * len(relations) + j is (drugs[i], relations[j]), its pairs (drugs[i], v).  known: (keys, ptr) of the pairs to
        drop (`ops.distmult_screen`)."""
        q = screen_queries(self.num_et, relations, drugs)
        return ops.distmult_screen(z.detach(), self.weight.detach(), q, k, known)

    def top_relations(self, z, pairs, k, known=None, relations=None):
        """Pair top-k (extension, `tipk_distmult_pair_topk`): the k best relations of every pair of `pairs` [2, P] by LOGIT ->
        (logits [P, k], relation int32 [P, k]); no autograd.  known: (pair_keys, pair_ptr, rel) to drop
        (`ops.known_relations_by_pair`).  relations: candidate ids (None = all); the returned ids are positions in it."""
        return ops.distmult_pair_topk(z.detach(), self._rows(relations), pairs, k, known)

    def relation_ranks(self, z, pairs, tgt_ptr, tgt_rel, known=None, relations=None):
        """Pair rank (extension, `tipk_distmult_pair_rank`): the rank of every target relation among the relations of its
        pair by LOGIT -> (rank int32 [T], logit [T]), rank 0 = not ranked; no autograd.  pairs [2, P], tgt_ptr [P + 1], tgt_rel
        [T]: `ops.targets_by_pair`.  known and relations as `top_relations`: with a candidate subset, tgt_rel and the known
        lists (`ops.restrict_known_relations`) hold positions in `relations`."""
        return ops.distmult_pair_rank(z.detach(), self._rows(relations), pairs, tgt_ptr, tgt_rel, known)

    def partner_ranks(self, z, q_rel, q_drug, tgt_ptr, tgt_node, known=None):
        """Partner rank (extension, `tipk_distmult_partner_rank`): the rank of every target drug among the partners of its
        (relation, drug) query by the screen's LOGIT -> (rank int32 [T], logit [T]), rank 0 = not ranked; no autograd.
        q_rel, q_drug [Q], tgt_ptr [Q + 1], tgt_node [T]: `ops.targets_by_query`.  known: (keys, ptr) as `screen`."""
        return ops.distmult_partner_rank(z.detach(), self.weight.detach(), q_rel, q_drug, tgt_ptr, tgt_node, known)

    def partner_sums(self, z, q_drug, k, relations=None, partner_w=None, known=None):
        """Partner sum (extension, `tipk_distmult_partner_sum`): per queried drug and relation the sum over the unrecorded
        partners c of partner_w[c] * sigma(LOGIT), their number, and the k relations of each drug with the largest sum ->
        (sum [Q, S], count int32 [Q, S], top_val [Q, k], top_pos int32 [Q, k]) as `ops.distmult_partner_sum`; no autograd.
        relations: the ids that are the columns (None = all; global ids, so `known` stays as it is); known: (keys, ptr) as
        `screen`, dropped in both directions."""
        return ops.distmult_partner_sum(z.detach(), self.weight.detach(), q_drug, k, relations, partner_w, known)

    def pair_ranks(self, z, q_rel, tgt_ptr, tgt_u, tgt_v, known=None):
        """Screen rank (extension, `tipk_distmult_screen_rank`): the rank of every target pair among all unordered pairs of
        its relation query by the screen's LOGIT -> (rank int32 [T], logit [T]), rank 0 = not ranked; no autograd.
        q_rel [Q], tgt_ptr [Q + 1], tgt_u, tgt_v [T]: `ops.targets_by_relation`.  known: (keys, ptr) as `screen`."""
        return ops.distmult_screen_rank(z.detach(), self.weight.detach(), q_rel, tgt_ptr, tgt_u, tgt_v, known)

    def top_regimen_relations(self, z, reg_drugs, reg_ptr, k, aggregate='max', known=None, relations=None):
        """Regimen top-k (extension, `tipk_distmult_regimen_topk`): the k best relations of every drug list of the CSR pair
        (reg_drugs, reg_ptr) by the aggregate of its pairs' LOGITS -> (score [G, k], relation int32 [G, k], pair_i, pair_j
        int32 [G, k]: list positions of the driving pair); no autograd.  known and relations as `top_relations`."""
        return ops.distmult_regimen_topk(z.detach(), self._rows(relations), reg_drugs, reg_ptr, k, aggregate, known)

    def addon_burden(self, z, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate='noisy_or', weights=None, known=None,
                     relations=None):
        """Add-on burden (extension, `tipk_distmult_addon_burden`): sum_r weights[r] * P_r of every candidate of every
        context of the CSR pairs (ctx_drugs, ctx_ptr) and (cand, cand_ptr) (cand_ptr None: one shared list), and the k
        candidates of each query with the lowest burden -> (burden, best_burden [Q, k], best_pos int32 [Q, k]) as
        `ops.distmult_addon_burden`; no autograd.  known and relations as `top_relations`; weights: one per candidate
        relation."""
        return ops.distmult_addon_burden(z.detach(), self._rows(relations), ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights, known)

    def combination_burden(self, z, plan, k, aggregate='noisy_or', weights=None, known=None, relations=None):
        """Combination burden (extension, `tipk_distmult_combo_burden`): sum_r weights[r] * P_r over ALL pairs of every
        regimen the queries of `plan` (`ops.combo_plan`) can form, and the k combinations of each query with the lowest
        burden -> (burden [n_comb], comb_ptr [Q + 1], best_burden [Q, k], best_comb int32 [Q, k]) as
        `ops.distmult_combo_burden`; no autograd.  known, relations and weights as `addon_burden`."""
        return ops.distmult_combo_burden(z.detach(), self._rows(relations), plan, k, aggregate, weights, known)


def normalize_regimens(regimens, n_drug, max_drugs):
    """Host normalisation of `TIP.regimen_side_effects`: a list of lists of drug ids, or a (drugs, ptr) pair of int tensors
    (regimen g = drugs[ptr[g]:ptr[g + 1]]) -> (drugs int32, ptr int64) on the host with every regimen sorted ascending and
    de-duplicated.  ValueError for an id outside [0, n_drug), a regimen of more than max_drugs distinct drugs, or lists
    that are not what the above says."""
    if isinstance(regimens, tuple) and len(regimens) == 2 and all(torch.is_tensor(t) for t in regimens):
        drugs, ptr = (t.detach().to('cpu') for t in regimens)
        if drugs.dim() != 1 or ptr.dim() != 1 or ptr.numel() < 1 or drugs.dtype.is_floating_point or ptr.dtype.is_floating_point:
            raise ValueError('regimens: int tensors (drugs [n_entries], ptr [G + 1]) expected, got %s %s and %s %s'
                             % (drugs.dtype, tuple(drugs.shape), ptr.dtype, tuple(ptr.shape)))
        ptr = ptr.to(torch.int64)
        size = ptr[1:] - ptr[:-1]
        if int(ptr[0]) != 0 or int(ptr[-1]) != drugs.numel() or bool((size < 0).any()):
            raise ValueError('regimens: ptr must ascend from 0 to the number of entries (%d)' % drugs.numel())
        drugs = drugs.to(torch.int64)
    else:
        try:
            lists = [[int(x) for x in g] for g in regimens]
        except (TypeError, ValueError):
            raise ValueError('regimens: a list of lists of drug ids, or a (drugs, ptr) tensor pair expected') from None
        size = torch.tensor([len(g) for g in lists], dtype=torch.int64)
        drugs = torch.tensor([x for g in lists for x in g], dtype=torch.int64)
    if drugs.numel():
        lo, hi = int(drugs.min()), int(drugs.max())
        if lo < 0 or hi >= n_drug:
            raise ValueError('drug id out of range: [%d, %d] for %d drugs' % (lo, hi, n_drug))
    owner = torch.repeat_interleave(torch.arange(size.numel()), size)
    uniq = torch.unique(owner * max(1, int(n_drug)) + drugs)            # sorted by (regimen, id), duplicates gone
    owner = torch.div(uniq, max(1, int(n_drug)), rounding_mode='floor')
    size = torch.bincount(owner, minlength=size.numel())
    if size.numel() and int(size.max()) > max_drugs:
        raise ValueError('a regimen of %d distinct drugs: at most %d are ranked' % (int(size.max()), max_drugs))
    ptr = torch.zeros(size.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(size, 0)
    return (uniq % max(1, int(n_drug))).to(torch.int32), ptr


def normalize_add_on_queries(regimens, candidates, replace, n_drug, max_context):
    """Host normalisation of `TIP.add_on_risk` -> (ctx_drugs int32, ctx_ptr int64 [G + 1], cand int32, cand_ptr int64
    [G + 1] or None) on the host.
    regimens: as `normalize_regimens` (each sorted ascending and de-duplicated).  replace: None, or one drug id per regimen
    (-1: none): that drug is taken out of the regimen, and what is left is the query's context; ValueError when it is not a
    member.  A context may be empty (its burdens are NaN) and holds at most max_context drugs.
    candidates: None = every drug, as the shared list 0 .. n_drug - 1 (cand_ptr None); a flat list or 1-d int tensor = one
    list shared by all regimens (cand_ptr None); a list of G lists = one list per regimen (CSR).  Candidate lists keep
    their order and their repeats.  For the two shared forms the G x C tasks are query-major: `burden.view(G, C)`.
    ValueError for an id outside [0, n_drug), a context of more than max_context drugs, or lists that are not what the
    above says."""
    drugs, ptr = normalize_regimens(regimens, n_drug, max_context + (0 if replace is None else 1))
    G = ptr.numel() - 1
    if replace is not None:
        try:
            rep = torch.as_tensor(replace).detach().to('cpu')
            bad = rep.dim() != 1 or rep.numel() != G or rep.dtype.is_floating_point or rep.dtype == torch.bool
        except (TypeError, ValueError, RuntimeError):
            bad = True
        if bad:
            raise ValueError('replace: one drug id per regimen (-1: none) expected, %d regimens' % G)
        rep = rep.to(torch.int64)
        owner = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
        hit = drugs.to(torch.int64) == rep[owner]
        found = torch.zeros(G, dtype=torch.int64).index_add_(0, owner, hit.to(torch.int64))
        missing = (rep != -1) & (found == 0)
        if bool(missing.any()):
            g = int(torch.nonzero(missing)[0])
            raise ValueError('replace: drug %d is not a member of regimen %d' % (int(rep[g]), g))
        drugs, owner = drugs[~hit], owner[~hit]
        size = torch.bincount(owner, minlength=G)
        ptr = torch.zeros(G + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(size, 0)
    size = ptr[1:] - ptr[:-1]
    if G and int(size.max()) > max_context:
        raise ValueError('a context of %d drugs: at most %d are scored' % (int(size.max()), max_context))
    cand_ptr = None
    if candidates is None:
        cand = torch.arange(int(n_drug), dtype=torch.int64)
    elif torch.is_tensor(candidates):
        cand = candidates.detach().to('cpu')
        if cand.dim() != 1 or cand.dtype.is_floating_point or cand.dtype == torch.bool:
            raise ValueError('candidates: a 1-d int tensor expected, got %s %s' % (cand.dtype, tuple(cand.shape)))
        cand = cand.to(torch.int64)
    else:
        try:
            items = list(candidates)
            nested = len(items) > 0 and all(isinstance(c, (list, tuple)) or (torch.is_tensor(c) and c.dim() == 1)
                                            for c in items)
            if nested:
                lists = [[int(x) for x in c] for c in items]
            else:
                cand = torch.tensor([int(x) for x in items], dtype=torch.int64)
        except (TypeError, ValueError):
            raise ValueError('candidates: None, a list of drug ids, or one list of drug ids per regimen expected') from None
        if nested:
            if len(lists) != G:
                raise ValueError('candidates: %d lists for %d regimens' % (len(lists), G))
            cand = torch.tensor([x for c in lists for x in c], dtype=torch.int64)
            cand_ptr = torch.zeros(G + 1, dtype=torch.int64)
            cand_ptr[1:] = torch.cumsum(torch.tensor([len(c) for c in lists], dtype=torch.int64), 0)
    if cand.numel():
        lo, hi = int(cand.min()), int(cand.max())
        if lo < 0 or hi >= n_drug:
            raise ValueError('candidate drug id out of range: [%d, %d] for %d drugs' % (lo, hi, n_drug))
    return drugs.to(torch.int32), ptr, cand.to(torch.int32), cand_ptr


def normalize_combination_queries(slots, fixed, n_drug, limits):
    """Host normalisation of `TIP.combination_risk` -> (fix_drugs int32, fix_ptr int64 [G + 1], alt int32, alt_ptr int64
    [n_slots + 1], slot_ptr int64 [G + 1]) on the host, the lists of include/tipk.h section 4n, in the order given.
    slots: ONE query as a list of slots, each a non-empty list of alternatives (a drug id, or -1 for "leave the slot
    empty"), or a list of G such queries; an empty list is a query without slots (`[[]]`: one such query).  fixed: None
    (no fixed drugs), one list of drug ids (one query, or shared by all G), or G lists.  limits: `ops.combo_limits()`.
    ValueError, with the query's number, for a fixed id outside [0, n_drug), a repeated fixed drug, an alternative outside
    [-1, n_drug), an empty slot, more than limits.max_fixed fixed drugs, limits.max_slots slots, limits.max_alternatives
    alternatives or limits.max_combinations combinations, or lists that are not what the above says.  A drug that is both
    fixed and an alternative, or an alternative of two slots, is legal: the combinations that take it twice come back NaN."""
    def plain(x):
        return x.tolist() if torch.is_tensor(x) else x

    def seq(x):
        return isinstance(x, (list, tuple))

    def ints(x, what):
        try:
            if not seq(x) or any(seq(v) or isinstance(v, (bool, float)) for v in x):
                raise TypeError
            return [int(v) for v in x]
        except (TypeError, ValueError):
            raise ValueError('%s: a list of drug ids expected, got %r' % (what, x)) from None

    slots = plain(slots)
    if not seq(slots):
        raise ValueError('slots: a list of slots (lists of alternatives), or a list of such queries expected')
    slots = [plain(e) for e in slots]
    # an entry is a QUERY when it is an empty list or a list of lists, a SLOT when it is a non-empty list of ids; a list of
    # queries needs every entry to be one, anything else is read as the slots of one query
    def is_query(e):
        return seq(e) and all(seq(plain(v)) for v in e)
    queries = [[plain(v) for v in e] for e in slots] if len(slots) > 0 and all(is_query(e) for e in slots) else [slots]
    G = len(queries)
    if fixed is None:
        fixed_lists = [[] for _ in range(G)]
    elif seq(plain(fixed)) and len(plain(fixed)) > 0 and all(seq(plain(f)) for f in plain(fixed)):
        fixed = [plain(f) for f in plain(fixed)]
        if len(fixed) != G:
            raise ValueError('fixed: %d lists for %d queries' % (len(fixed), G))
        fixed_lists = [ints(f, 'fixed (query %d)' % g) for g, f in enumerate(fixed)]
    else:
        shared = ints(plain(fixed), 'fixed')
        fixed_lists = [list(shared) for _ in range(G)]
    fix, fptr, alt, aptr, sptr = [], [0], [], [0], [0]
    for g, (q, f) in enumerate(zip(queries, fixed_lists)):
        if not isinstance(q, (list, tuple)):
            raise ValueError('query %d: a list of slots expected, got %r' % (g, q))
        if len(f) > limits.max_fixed:
            raise ValueError('query %d: %d fixed drugs, at most %d are scored' % (g, len(f), limits.max_fixed))
        if any(d < 0 or d >= n_drug for d in f):
            raise ValueError('query %d: fixed drug id out of range for %d drugs: %r' % (g, n_drug, [d for d in f if d < 0 or d >= n_drug]))
        if len(set(f)) != len(f):
            raise ValueError('query %d: a fixed drug is repeated' % g)
        if len(q) > limits.max_slots:
            raise ValueError('query %d: %d slots, at most %d' % (g, len(q), limits.max_slots))
        count, total = 1, 0
        for si, slot in enumerate(q):
            a = ints(slot, 'query %d, slot %d' % (g, si))
            if len(a) == 0:
                raise ValueError('query %d: slot %d is empty' % (g, si))
            if any(d < -1 or d >= n_drug for d in a):
                raise ValueError('query %d, slot %d: alternative out of range [-1, %d): %r'
                                 % (g, si, n_drug, [d for d in a if d < -1 or d >= n_drug]))
            alt += a
            aptr.append(len(alt))
            count, total = count * len(a), total + len(a)
        if total > limits.max_alternatives:
            raise ValueError('query %d: %d alternatives in all slots, at most %d' % (g, total, limits.max_alternatives))
        if count > limits.max_combinations:
            raise ValueError('query %d: %d combinations, at most %d' % (g, count, limits.max_combinations))
        fix += f
        fptr.append(len(fix))
        sptr.append(len(aptr) - 1)
    return (torch.tensor(fix, dtype=torch.int32), torch.tensor(fptr, dtype=torch.int64), torch.tensor(alt, dtype=torch.int32),
            torch.tensor(aptr, dtype=torch.int64), torch.tensor(sptr, dtype=torch.int64))


def screen_queries(num_et, relations=None, drugs=None):
    """int32 [Q, 2] (relation, drug | -1) on the host, in the order `MultiInnerProductDecoder.screen` documents."""
    rel = torch.arange(num_et, dtype=torch.int64) if relations is None \
        else torch.as_tensor(relations).to('cpu', torch.int64).reshape(-1)
    if drugs is None:
        q = torch.stack([rel, torch.full_like(rel, -1)], 1)
    else:
        dr = torch.as_tensor(drugs).to('cpu', torch.int64).reshape(-1)
        q = torch.stack([rel.repeat(dr.numel()), dr.repeat_interleave(rel.numel())], 1)
    return q.to(torch.int32)


_SCREEN_KEYS = DerivedCache(8)


def _screen_known(d, exclude):
    """(keys, ptr) of the pairs `TIP.screen` drops: the training positives ('train', the sampler's cached keys) or
    train + test ('all', merged once per (edge tensor, range list) of both and cached: `_cache.DerivedCache`)."""
    if exclude is None:
        return None
    from .neg_sampling import _cached_keys
    kt, pt = _cached_keys(d.dd_train_idx, d.n_drug, d.dd_train_range)[:2]
    if exclude == 'train':
        return kt, pt

    def build():
        ke, pe = _cached_keys(d.dd_test_idx, d.n_drug, d.dd_test_range)[:2]
        n_rel = pt.numel() - 1
        ids = torch.arange(n_rel, device=kt.device)
        rel = torch.cat([torch.repeat_interleave(ids, pt[1:] - pt[:-1]), torch.repeat_interleave(ids, pe[1:] - pe[:-1])])
        keys = torch.cat([kt, ke])
        order = torch.sort(rel * (int(d.n_drug) ** 2) + keys).indices
        ptr = torch.zeros(n_rel + 1, dtype=torch.int64, device=kt.device)
        ptr[1:] = torch.cumsum(torch.bincount(rel, minlength=n_rel), 0)
        return keys[order].contiguous(), ptr

    return _SCREEN_KEYS.get((d.dd_train_idx, keyable(d.dd_train_range), d.dd_test_idx, keyable(d.dd_test_range)),
                            int(d.n_drug), build)


_REKEYED = DerivedCache(8)


def _rekeyed_known(known, n, n_wide):
    """The relation-major lists `known` (keys u * n + v) as keys u * n_wide + v of a wider node set -- the same pairs in the
    same order --, cached per (keys, ptr) like `_SCREEN_KEYS`; None stays None."""
    if known is None:
        return None
    keys, ptr = known

    def build():
        kk = keys.to(torch.int64)
        return (torch.div(kk, int(n), rounding_mode='floor') * int(n_wide) + kk % int(n)).contiguous(), ptr

    return _REKEYED.get((keys, ptr), (int(n), int(n_wide)), build)


class NNDecoder(nn.Module):
    """The paper's DR-NN decoder (reference `src/layers.py:598-637`):
    score = sigma( relu(z[u] w1_l1) . w1_l2[r] + relu(z[v] w2_l1) . w2_l2[r] ).

    The reference gathers z[u], z[v] (E x in), multiplies E x in by in x l1 twice and gathers two
    E x l1 relation rows.  Here the node-level part is done once per node (two GEMMs with fused ReLU),
    the relation-specific dot products of ALL (node, relation) pairs are two small dense GEMMs
    (N x R tables, 2.8 MB), and a triple costs two scalar reads (`tipk_pair_table_fwd`)."""

    def __init__(self, in_dim, num_uni_edge_type, l1_dim=16):
        super().__init__()
        self.l1_dim = l1_dim
        self.w1_l1 = Param(torch.empty(in_dim, l1_dim))
        self.w1_l2 = Param(torch.empty(num_uni_edge_type, l1_dim))
        self.w2_l1 = Param(torch.empty(in_dim, l1_dim))
        self.w2_l2 = Param(torch.empty(num_uni_edge_type, l1_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.w1_l1.data.normal_()
        self.w2_l1.data.normal_()
        self.w1_l2.data.normal_(std=1 / np.sqrt(self.l1_dim))
        self.w2_l2.data.normal_(std=1 / np.sqrt(self.l1_dim))

    def _tables(self, z, relations=None, relation_major=False):
        """The two score tables: every (node, relation) dot product, node-major [N, R] as `forward` reads them or
        relation-major [R, N] as `objective` does.  relations: candidate ids (None = all), rows of w*_l2."""
        w1, w2 = (self.w1_l2, self.w2_l2) if relations is None else (self.w1_l2[relations], self.w2_l2[relations])
        p = torch.relu(ops.matmul(z, self.w1_l1))
        q = torch.relu(ops.matmul(z, self.w2_l1))
        if relation_major:
            return ops.matmul(w1, p.t()), ops.matmul(w2, q.t())
        return ops.matmul(p, w1.t()), ops.matmul(q, w2.t())

    def probe(self, z, edge_index, edge_type, side='v'):
        """`MultiInnerProductDecoder.probe` for this decoder -> (node int64 [T], probe [T, in_dim], offset [T]).  The
        decoder is bias-free and piecewise linear in z[node], so its part of the logit equals its own gradient times
        z[node]: side 'v': probe = w2_l1 (m * w2_l2[r]) with the ReLU mask m = (z[v] w2_l1 > 0), offset = the first drug's
        part relu(z[u] w1_l1) . w1_l2[r]; side 'u' is the mirror image with w1_* and the second drug's part as offset."""
        with torch.no_grad():
            u, v = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
            z = z.detach()
            first = (self.w1_l1.detach(), self.w1_l2.detach()[edge_type], u)
            second = (self.w2_l1.detach(), self.w2_l2.detach()[edge_type], v)
            (l1, l2, node), (o1, o2, other) = (second, first) if side == 'v' else (first, second)
            mask = (z[node] @ l1 > 0).to(z.dtype)
            return node, (mask * l2) @ l1.t(), (torch.relu(z[other] @ o1) * o2).sum(1)

    def forward(self, z, edge_index, edge_type):
        s1, s2 = self._tables(z)
        return ops.pair_table_score(s1, s2, edge_index, edge_type, sigmoid=True)

    def top_relations(self, z, pairs, k, known=None, relations=None):
        """Pair top-k (extension, `tipk_pair_table_pair_topk`) on the two tables `forward` forms -> (logits [P, k], relation
        int32 [P, k]); no autograd.  relations: candidate ids (None = all): columns of the tables, i.e. rows of w*_l2; the
        returned ids are positions in it."""
        with torch.no_grad():
            s1, s2 = self._tables(z.detach(), relations)
        return ops.pair_table_pair_topk(s1, s2, pairs, k, known)

    def relation_ranks(self, z, pairs, tgt_ptr, tgt_rel, known=None, relations=None):
        """Pair rank (extension, `tipk_pair_table_pair_rank`) on the two tables `forward` forms; arguments and result as
        `MultiInnerProductDecoder.relation_ranks`.  The pair's first drug is the decoder's first argument."""
        with torch.no_grad():
            s1, s2 = self._tables(z.detach(), relations)
        return ops.pair_table_pair_rank(s1, s2, pairs, tgt_ptr, tgt_rel, known)

    def partner_ranks(self, z, q_rel, q_drug, tgt_ptr, tgt_node, known=None):
        """Partner rank (extension, `tipk_pair_table_partner_rank`) on the two TRANSPOSED tables `objective` forms ([R, N]: a
        query's candidates are one contiguous row); arguments and result as `MultiInnerProductDecoder.partner_ranks`.  The
        queried drug is the decoder's first argument, the ranked partner its second."""
        with torch.no_grad():
            s1t, s2t = self._tables(z.detach(), relation_major=True)
        return ops.pair_table_partner_rank(s1t, s2t, q_rel, q_drug, tgt_ptr, tgt_node, known)

    def partner_sums(self, z, q_drug, k, relations=None, partner_w=None, known=None):
        """Partner sum (extension, `tipk_pair_table_partner_sum`) on the two TRANSPOSED tables `objective` forms ([R, N]);
        arguments and result as `MultiInnerProductDecoder.partner_sums`.  The queried drug is the decoder's first argument,
        the partner its second."""
        with torch.no_grad():
            s1t, s2t = self._tables(z.detach(), relation_major=True)
        return ops.pair_table_partner_sum(s1t, s2t, q_drug, k, relations, partner_w, known)

    def top_regimen_relations(self, z, reg_drugs, reg_ptr, k, aggregate='max', known=None, relations=None):
        """Regimen top-k (extension, `tipk_pair_table_regimen_topk`) on the two tables `forward` forms; arguments and result
        as `MultiInnerProductDecoder.top_regimen_relations`.  The earlier list position is the decoder's first argument."""
        with torch.no_grad():
            s1, s2 = self._tables(z.detach(), relations)
        return ops.pair_table_regimen_topk(s1, s2, reg_drugs, reg_ptr, k, aggregate, known)

    def addon_burden(self, z, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate='noisy_or', weights=None, known=None,
                     relations=None):
        """Add-on burden (extension, `tipk_pair_table_addon_burden`) on the two tables `forward` forms; arguments and result
        as `MultiInnerProductDecoder.addon_burden`.  The smaller drug id of a pair is the decoder's first argument."""
        with torch.no_grad():
            s1, s2 = self._tables(z.detach(), relations)
        return ops.pair_table_addon_burden(s1, s2, ctx_drugs, ctx_ptr, cand, cand_ptr, k, aggregate, weights, known)

    def combination_burden(self, z, plan, k, aggregate='noisy_or', weights=None, known=None, relations=None):
        """Combination burden (extension, `tipk_pair_table_combo_burden`) on the two tables `forward` forms; arguments and
        result as `MultiInnerProductDecoder.combination_burden`."""
        with torch.no_grad():
            s1, s2 = self._tables(z.detach(), relations)
        return ops.pair_table_combo_burden(s1, s2, plan, k, aggregate, weights, known)

    def objective(self, z, pos_index, neg_index, edge_type):
        """-mean log(sigma(pos)+eps) - mean log(1-sigma(neg)+eps) (src/layers.py:335-340 with this decoder as
        model/ddm-nn.py:65-102 trains it), fused: the tables are formed TRANSPOSED ([R, N]: a relation's scores are one
        contiguous row), one launch evaluates every positive and negative triple and leaves both table gradients
        (`tipk_pair_table_loss`); the four weight gradients and d z follow through the four small products."""
        p = torch.relu(ops.matmul(z, self.w1_l1))
        q = torch.relu(ops.matmul(z, self.w2_l1))
        if not ops.pair_table_loss_supported(z.shape[0]):
            # node sets whose two table rows (24 B per node) exceed the kernel's LDS: scores by the table kernels, the loss as the
            # reference spells it -- still every FLOP on the device, through tipk_pair_table_fwd / _bwd
            neg = ops.unpack_pairs(neg_index) if getattr(neg_index, '_tipk_packed_pairs', False) else neg_index
            pos_s = self(z, pos_index, edge_type)
            neg_s = self(z, neg, edge_type)
            return (-torch.log(pos_s + EPS).mean() - torch.log(1 - neg_s + EPS).mean()).view(1)
        s1t = ops.matmul(self.w1_l2, p.t())                      # [R, N]
        s2t = ops.matmul(self.w2_l2, q.t())
        return ops.pair_table_objective(s1t, s2t, pos_index, neg_index, edge_type)


# ---------------------------------------------------------------------------------------------
# The steps the TIP queries share.  Functions of the values they need: the query methods also run unbound, on a bare
# namespace, up to their last refusal.
# ---------------------------------------------------------------------------------------------
def _refuse_sharded(shard, what):
    """NotImplementedError for a relation-sharded model: the queries need every decoder row.  what: the noun the message
    ranks ('side effects', 'candidates', 'partners', 'pairs'), or 'screen'."""
    if shard is not None:
        how = 'screen the' if what == 'screen' else 'rank the %s with the' % what
        raise NotImplementedError('a relation-sharded model holds only its shard\'s decoder rows; %s unsharded model '
                                  '(tip_amd.dist.gather_state_dict)' % how)


def _check_known_mode(name, mode):
    """ValueError unless the `exclude` / `filter` argument `name` is 'train', 'all' or None."""
    if mode not in ('train', 'all', None):
        raise ValueError("%s must be 'train', 'all' or None, not %r" % (name, mode))


def _relation_ids(relations, dev):
    """The candidate side-effect ids `relations` as an int64 tensor on `dev`, or None (= all)."""
    return None if relations is None else torch.as_tensor(relations).to(device=dev, dtype=torch.int64).reshape(-1)


def _pair_known(d, mode, rel):
    """The pair-major known lists (`ops.known_relations_by_pair`) an `exclude` / `filter` mode drops: the training side
    effects of every pair ('train'), train and test ones merged ('all'), or None (None).  rel: the candidate ids on the
    lists' device or None -- the lists hold global ids, so with candidates they keep the candidates' entries only,
    renumbered to positions in `rel` (`ops.restrict_known_relations`)."""
    if mode is None:
        return None
    extra = (d.dd_test_idx, d.dd_test_range) if mode == 'all' else None
    known = ops.known_relations_by_pair(d.dd_train_idx, d.dd_train_range, d.n_drug, extra=extra)
    return known if rel is None else ops.restrict_known_relations(known, rel, d.n_dd_et)


def _training_pairs_of(d, rel):
    """The training pairs of the side effects `rel` (int64, host), each unordered pair once, in the (edge_index, ptr) form
    `ops.fit_pairs_csr` takes: relation i of the result is side effect rel[i]."""
    idx = d.dd_train_idx.to('cpu', torch.int64)
    rng = torch.as_tensor(d.dd_train_range).to('cpu', torch.int64).reshape(-1, 2)
    n = int(d.n_drug)
    cols, counts = [], []
    for r in rel.tolist():
        e = idx[:, int(rng[r, 0]):int(rng[r, 1])]
        key = torch.unique(torch.minimum(e[0], e[1]) * n + torch.maximum(e[0], e[1]))
        cols.append(torch.stack([torch.div(key, n, rounding_mode='floor'), key % n]))
        counts.append(key.numel())
    ptr = torch.zeros(len(counts) + 1, dtype=torch.int64)
    if counts:
        ptr[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
    return (torch.cat(cols, 1) if cols else torch.zeros((2, 0), dtype=torch.int64)), ptr


def _pair_major_known(fp, n, dev):
    """The distinct recorded pairs of a `FitPairs` as pair-major known lists on `dev` (include/tipk.h section 4d): keys
    u * n + v (u <= v) ascending, ptr, and inside a pair's block the ascending ids of the relations that list it."""
    b = fp.ptr.numel() - 1
    rel = torch.repeat_interleave(torch.arange(b, dtype=torch.int64), fp.ptr[1:] - fp.ptr[:-1])
    c = torch.unique((fp.u.to(torch.int64) * int(n) + fp.v.to(torch.int64)) * max(b, 1) + rel)
    keys, counts = torch.unique_consecutive(torch.div(c, max(b, 1), rounding_mode='floor'), return_counts=True)
    ptr = torch.zeros(keys.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(counts, 0)
    return keys.to(dev), ptr.to(dev), (c % max(b, 1)).to(torch.int32).to(dev)


def _checked_triples(triples, d, dev):
    """The triples a rank evaluation ranks -> (edge_index [2, T], edge_type int64 [T]) on `dev`: the held-out set of `d` for
    None, else the given (edge_index, edge_type), refused with ValueError unless int tensors of these shapes with ids in
    range."""
    idx, et = (d.dd_test_idx, d.dd_test_et) if triples is None else triples
    idx, et = torch.as_tensor(idx).to(dev), torch.as_tensor(et).to(dev)
    if idx.dim() != 2 or idx.shape[0] != 2 or et.dim() != 1 or et.numel() != idx.shape[1] \
            or idx.dtype.is_floating_point or et.dtype.is_floating_point:
        raise ValueError('triples: int tensors (edge_index [2, T], edge_type [T]) expected, got %s %s and %s %s'
                         % (idx.dtype, tuple(idx.shape), et.dtype, tuple(et.shape)))
    if et.numel():
        lo, hi, rlo, rhi = torch.stack([idx.min(), idx.max(), et.min(), et.max()]).tolist()
        if lo < 0 or hi >= d.n_drug:
            raise ValueError('drug id out of range: [%d, %d] for %d drugs' % (lo, hi, d.n_drug))
        if rlo < 0 or rhi >= d.n_dd_et:
            raise ValueError('side-effect id out of range: [%d, %d] for %d side effects' % (rlo, rhi, d.n_dd_et))
    return idx, et.to(torch.int64)


def _rank_result(order, r, s, et, n_rel, ks):
    """The RankReport of a rank entry's (rank r, logit s) in grouped order: both scattered back through `order` (the
    `ops.targets_by_*` permutation) to the triples' order, and `utils.rank_report` of the ranks by side effect `et`."""
    rank = torch.empty_like(r, dtype=torch.int64)
    rank[order] = r.to(torch.int64)
    logit = torch.empty_like(s)
    logit[order] = s
    return RankReport(rank, logit, **rank_report(rank, et, n_rel, ks))


def _csr_of_lists(lists, width, limits, names, what):
    """A list of per-row lists of `width`-tuples (bare ints for width 1) -> (ptr int64 [len + 1], then `width` int32 id
    tensors) on the host; ValueError unless column c holds ints in [0, limits[c]) -- `names[c]` says what it is."""
    ptr, cols = [0], [[] for _ in range(width)]
    for row in lists:
        for item in (row if row is not None else ()):
            item = (item,) if width == 1 else tuple(item)
            if len(item) != width:
                raise ValueError('%s: entries of %d ids expected, got %r' % (what, width, item))
            for c in range(width):
                v = int(item[c])
                if v < 0 or v >= limits[c]:
                    raise ValueError('%s: %s id out of range: %d for %d' % (what, names[c], v, limits[c]))
                cols[c].append(v)
        ptr.append(len(cols[0]))
    return (torch.tensor(ptr, dtype=torch.int64),) + tuple(torch.tensor(c, dtype=torch.int32) for c in cols)


def _ids_at(pos, lookup, first=None):
    """Positions a kernel returned -> the int64 ids `lookup` holds there; padding (pos < 0) stays -1.  first: the offset of
    each row's list in `lookup` (CSR), for positions that count inside a row's list."""
    at = pos.to(torch.int64) if first is None else first + pos
    if lookup.numel() == 0:                                              # only padding can point into an empty list
        lookup = lookup.new_zeros(1)
    return torch.where(pos >= 0, lookup[at.clamp(min=0, max=lookup.numel() - 1)], torch.full_like(at, -1))


def _scoring_operands(model, calibration):
    """(z, decoder) a decoder query runs on: the model's own for None, else the widened snapshot and decoder of the
    `Calibration`, refused unless they fit this model: NotImplementedError for the NN decoder or a relation-sharded
    model, ValueError for another number of side effects, drugs or columns."""
    if calibration is None:
        return model.embeddings, model.decoder
    if model.decoder_kind == 'nn':
        raise NotImplementedError('a calibration widens DistMult operands; this model scores with the NN decoder '
                                  '(include/tipk.h 4r)')
    _refuse_sharded(model.shard, 'calibrated side effects')
    if not isinstance(calibration, Calibration):
        raise ValueError('calibration: the Calibration of TIP.calibrate expected, got %s' % type(calibration).__name__)
    z, dec = calibration.z, calibration.decoder
    if z.device != model.embeddings.device or dec.weight.device != z.device:
        raise ValueError('calibration: its operands are on %s, the model is on %s' % (z.device, model.embeddings.device))
    want = (model.data.n_drug, model.decoder.in_dim + 4)
    if tuple(z.shape) != want or dec.num_et != model.decoder.num_et or dec.in_dim != want[1]:
        raise ValueError('calibration: made for %d drugs, %d columns and %d side effects; this model has %d, %d + 4 and %d'
                         % (z.shape[0], z.shape[1], dec.num_et, want[0], want[1] - 4, model.decoder.num_et))
    return z, dec


# ---------------------------------------------------------------------------------------------
# A9  training framework   (src/layers.py:260-375)
# ---------------------------------------------------------------------------------------------
class Setting(object):
    def __init__(self, sp_rate=0.9, lr=0.01, prot_drug_dim=16, n_embed=48, n_hid1=32, n_hid2=16, num_base=32):
        self.sp_rate, self.lr = sp_rate, lr
        self.prot_drug_dim, self.n_embed = prot_drug_dim, n_embed
        self.n_hid1, self.n_hid2, self.num_base = n_hid1, n_hid2, num_base


class TIP(nn.Module):
    """`TIP(settings, device, mod='cat', data_path='./data/data_dict.pkl')` as in the reference.

    data_path: a pickle written by the reference's `prepare.py` loads as is; if the DEFAULT file
    does not exist (or data_path is None), the BioSNAP graph bundled with this package is split with
    seed 1111; any other missing path raises FileNotFoundError.  `.data_source` says which was used.
    `data` (extension): an already built data dict.  `fused_loss=False` computes the loss with
    torch ops on the decoder scores exactly as `src/layers.py:335-340` spells it."""

    def __init__(self, settings, device, mod='cat', data_path='./data/data_dict.pkl', data=None, fused_loss=True,
                 shard=None, decoder='distmult'):
        """shard (extension): a `tip_amd.dist.RelationShard` -- this process holds only its relations'
        edges, `rgcn*.att` rows and `decoder.weight` rows; see tip_amd/dist.py.
        decoder (extension): 'distmult' (tip.py, src/layers.py:581-595) | 'nn' -- the NNDecoder of src/layers.py:598-637 in
        the same training framework, as the reference's model/ddm-nn.py:65-102 trains it (l1_dim = 16)."""
        super().__init__()
        assert mod in {'cat', 'add'} and decoder in {'distmult', 'nn'}
        if decoder == 'nn' and shard is not None:
            raise NotImplementedError('the relation-sharded step holds decoder.weight rows only (tip_amd/dist.py)')
        self.mod, self.device, self.settings, self.fused_loss = mod, device, settings, fused_loss
        self.shard, self.decoder_kind = shard, decoder
        self.data = self.__prepare_data(data_path, settings.sp_rate, data).to(device)
        self.__prepare_model()

    DEFAULT_DATA_PATH = './data/data_dict.pkl'

    def __prepare_data(self, data_path, sp_rate, data_dict):
        if data_dict is None:
            if data_path is not None and os.path.exists(data_path):
                with open(data_path, 'rb') as f:
                    data_dict = pickle.load(f)
                self.data_source = os.path.abspath(data_path)
            elif data_path is None or data_path == self.DEFAULT_DATA_PATH:
                # only the reference's DEFAULT location may be absent (this package bundles the graph
                # that file is made from); an explicitly given path that does not exist is an error,
                # as in the reference (src/layers.py:284-285 raises FileNotFoundError)
                data_dict = build_data_dict(sp_rate=0.9)
                self.data_source = 'bundled BioSNAP blob (tip_amd/data/biosnap_v1.npz), split seed 1111'
            else:
                raise FileNotFoundError(data_path)
        else:
            self.data_source = 'data dict passed by the caller'
        data_dict = dict(data_dict)
        if sp_rate != 0.9:                                                   # :290-291
            (data_dict['dd_train_idx'], data_dict['dd_train_et'], data_dict['dd_train_range'],
             data_dict['dd_test_idx'], data_dict['dd_test_et'], data_dict['dd_test_range']) = \
                process_edges(data_dict['dd_edge_index'], p=sp_rate)
        if self.shard is not None:                                           # this rank's relations only
            from .dist import shard_data_dict
            data_dict = shard_data_dict(data_dict, self.shard)
        data = Data.from_dict(data_dict)
        self._test_neg_host = None
        return data

    def __getstate__(self):
        """`torch.save(model, ...)` (tip.py:36): the embeddings of the last forward are saved as data,
        not with their autograd history."""
        st = self.__dict__.copy()
        if torch.is_tensor(st.get('embeddings')):
            st['embeddings'] = st['embeddings'].detach()
        return st

    def __encode(self):
        d = self.data
        return self.encoder(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm,
                            d.p_feat, d.pp_train_indices, d.dp_edge_index, d.dp_range_list)

    def __prepare_model(self):
        d, s = self.data, self.settings
        self.test_neg_index = typed_negative_sampling(d.dd_test_idx, d.n_drug, d.dd_test_range,    # :293
                                                      pos_offset=getattr(d, 'dd_test_pos_offset', None))
        self.encoder = FMEncoder(self.device, d.n_drug_feat, d.n_dd_et, d.n_prot, d.n_prot, d.n_drug,
                                 s.prot_drug_dim, s.num_base, s.n_embed, s.n_hid1, s.n_hid2,
                                 mod=self.mod).to(self.device)
        if self.shard is not None:
            from .dist import attach_shard
            attach_shard(self.encoder, self.shard)
        with torch.no_grad():                            # initial pass (:319, with self.device); it only
            self.embeddings = self.__encode()            # fills .embeddings and the plan caches
        if self.decoder_kind == 'nn':
            self.decoder = NNDecoder(s.n_hid2, d.n_dd_et, l1_dim=16).to(self.device)
        else:
            self.decoder = MultiInnerProductDecoder(s.n_hid2, d.n_dd_et).to(self.device)

    def forward(self, neg_index=None):
        """One full-batch training objective (:328-342).  `neg_index` (extension) injects fixed
        negatives for parity tests; by default they are drawn on device every call."""
        d = self.data
        self.embeddings = self.__encode()
        pos_index = d.dd_train_idx
        if neg_index is None:
            # (the fused objective reads pairs as 32-bit words: the sampler emits that form directly -- same draws)
            neg_index = typed_negative_sampling(d.dd_train_idx, d.n_drug, d.dd_train_range,
                                                pos_offset=getattr(d, 'dd_train_pos_offset', None),
                                                packed=bool(self.fused_loss and d.n_drug <= 65535 and pos_index.shape[1] > 0))
        if not getattr(neg_index, '_tipk_packed_pairs', False):
            neg_index = neg_index.type_as(pos_index)
        if self.shard is not None:
            return self.__sharded_objective(pos_index, neg_index)
        if self.fused_loss:
            return self.decoder.objective(self.embeddings, pos_index, neg_index, d.dd_train_et)
        pos_score = self.decoder(self.embeddings, pos_index, d.dd_train_et)
        neg_score = self.decoder(self.embeddings, neg_index, d.dd_train_et)
        return -torch.log(pos_score + EPS).mean() - torch.log(1 - neg_score + EPS).mean()

    def __sharded_objective(self, pos_index, neg_index):
        """The objective over ALL ranks' triples from shard-local work: both means of
        :338-340 run over the global triple count, so a rank's local objective (means over ITS E_k
        triples) enters with weight E_k / E; one scalar all-reduce going forward, one d z all-reduce
        going back (`sum_grad_over_ranks`), d decoder.weight rows stay local."""
        from .dist import all_reduce_sum, sum_grad_over_ranks
        z = sum_grad_over_ranks(self.embeddings, self.shard)
        if pos_index.shape[1] == 0:                                          # a rank without relations
            local = z.sum() * 0.0
        elif self.fused_loss:
            local = self.decoder.objective(z, pos_index, neg_index, self.data.dd_train_et)
        else:
            pos_score = self.decoder(z, pos_index, self.data.dd_train_et)
            neg_score = self.decoder(z, neg_index, self.data.dd_train_et)
            local = -torch.log(pos_score + EPS).mean() - torch.log(1 - neg_score + EPS).mean()
        return all_reduce_sum(local * self.shard.loss_weight, self.shard)

    def pred(self, dd_idx, dd_et):
        return self.decoder(self.embeddings, dd_idx, dd_et)

    def pred_topk(self, dd_pairs, k=10, max_triples=1 << 24):
        """Serving helper (extension): for every drug pair (u, v) of
        `dd_pairs` [2, P] the k most likely side effects -> (scores [P, k], relation ids [P, k]).
        All num_et relations of a pair are scored by the decoder kernel in one launch (pairs are
        processed in slices of at most `max_triples` triples).  `side_effects` answers the same question from one fused
        launch and can leave out the side effects already recorded for a pair."""
        R = self.data.n_dd_et
        k = min(int(k), R)
        pairs = dd_pairs.to(self.embeddings.device).to(torch.int64)
        P = pairs.shape[1]
        et_all = torch.arange(R, device=pairs.device)
        vals, ids = [], []
        step = max(1, max_triples // R)
        with torch.no_grad():
            for p0 in range(0, P, step):
                sl = pairs[:, p0:p0 + step]
                n = sl.shape[1]
                s = self.decoder(self.embeddings, sl.repeat_interleave(R, dim=1), et_all.repeat(n)).view(n, R)
                top = torch.topk(s, k, dim=1)
                vals.append(top.values)
                ids.append(top.indices)
        if not vals:
            return (torch.zeros((0, k), device=pairs.device), torch.zeros((0, k), dtype=torch.int64, device=pairs.device))
        return torch.cat(vals), torch.cat(ids)

    def side_effects(self, pairs, k=10, exclude=None, relations=None, sigmoid=True, calibration=None):
        """Serving (extension): the k side effects the model scores highest for every drug pair of `pairs` [2, P], among
        those not already recorded for the pair (`decoder.top_relations`: one `tipk_distmult_pair_topk` /
        `tipk_pair_table_pair_topk` launch on `self.embeddings`, under no_grad; both decoder kinds).
        exclude: 'train' drops the pair's training side effects (held-out ones can and do appear), 'all' drops train and
        test ones, None drops nothing; a recorded side effect is dropped in either pair direction.  relations: candidate
        side-effect ids (None = all); the returned ids are global.  Ranking is on the logit, ties by ascending position in
        `relations`; sigmoid = True applies sigma afterwards (padding: score sigma(-inf) = 0, relation -1).
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> SideEffects(score [P, k], relation int64 [P, k]) on the model's device."""
        _refuse_sharded(self.shard, 'side effects')
        _check_known_mode('exclude', exclude)
        d = self.data
        dev = self.embeddings.device
        pairs = torch.as_tensor(pairs).to(dev)
        if pairs.dim() != 2 or pairs.shape[0] != 2 or pairs.dtype.is_floating_point:
            raise ValueError('pairs: an int tensor [2, P] expected, got %s %s' % (pairs.dtype, tuple(pairs.shape)))
        if pairs.numel():
            lo, hi = torch.stack([pairs.min(), pairs.max()]).tolist()
            if lo < 0 or hi >= d.n_drug:
                raise ValueError('drug id out of range: [%d, %d] for %d drugs' % (lo, hi, d.n_drug))
        rel = _relation_ids(relations, dev)
        known = _pair_known(d, exclude, rel)
        with torch.no_grad():
            z, decoder = _scoring_operands(self, calibration)
            logit, idx = decoder.top_relations(z, pairs, k, known, rel)
            score = torch.sigmoid(logit) if sigmoid else logit
            idx = idx.to(torch.int64) if rel is None else _ids_at(idx, rel)
        return SideEffects(score, idx)

    def regimen_side_effects(self, regimens, k=10, aggregate='noisy_or', exclude=None, relations=None, probability=True,
                             calibration=None):
        """Serving (extension): the k side effects the model expects most from every drug REGIMEN (a medication list), and the
        two drugs of the list that drive each (`decoder.top_regimen_relations`: one `tipk_distmult_regimen_topk` /
        `tipk_pair_table_regimen_topk` launch on `self.embeddings`, under no_grad; both decoder kinds).
        regimens: a list of lists of drug ids, or a (drugs, ptr) pair of int tensors (CSR).  Every regimen is sorted
        ascending and de-duplicated on the host (`normalize_regimens`), so u < v always; a regimen of 0 or 1 drugs gives a
        padded row.  aggregate: 'noisy_or' ranks a side effect by sum softplus(logit) over the regimen's pairs, i.e. by the
        probability that at least one pair causes it; 'max' by its largest pair logit.  exclude / relations: as
        `side_effects` -- a recorded (pair, side effect) does not contribute.  probability = True maps the score after the
        kernel: sigmoid(A) for 'max', -expm1(-A) for 'noisy_or' (padding: score 0, relation -1, u = v = -1).
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> RegimenSideEffects(score [G, k], relation int64 [G, k], u int64 [G, k], v int64 [G, k]) on the model's device."""
        _refuse_sharded(self.shard, 'side effects')
        _check_known_mode('exclude', exclude)
        if aggregate not in ops.REGIMEN_AGGREGATES:
            raise ValueError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
        d = self.data
        drugs, ptr = normalize_regimens(regimens, d.n_drug, ops.regimen_max_drugs())
        dev = self.embeddings.device
        both = torch.cat([ptr, drugs.to(torch.int64)]).to(dev)          # one upload
        ptr_d, drugs_d = both[:ptr.numel()], both[ptr.numel():]
        rel = _relation_ids(relations, dev)
        known = _pair_known(d, exclude, rel)
        with torch.no_grad():
            z, decoder = _scoring_operands(self, calibration)
            score, idx, pi, pj = decoder.top_regimen_relations(z, drugs_d, ptr_d, k, aggregate, known, rel)
            if probability:
                score = torch.sigmoid(score) if aggregate == 'max' \
                    else torch.where(idx >= 0, -torch.expm1(-score), torch.zeros_like(score))   # (padding: -expm1(inf))
            idx = idx.to(torch.int64) if rel is None else _ids_at(idx, rel)
            u, v = _ids_at(pi, drugs_d, ptr_d[:-1, None]), _ids_at(pj, drugs_d, ptr_d[:-1, None])
        return RegimenSideEffects(score, idx, u, v)

    def add_on_risk(self, regimens, candidates=None, k=10, replace=None, aggregate='noisy_or', weights=None, relations=None,
                    exclude=None, calibration=None):
        """Serving (extension): which CANDIDATE drug adds the least expected side-effect burden to every drug regimen
        (`decoder.addon_burden`: one `tipk_distmult_addon_burden` / `tipk_pair_table_addon_burden` call on
        `self.embeddings`, under no_grad; both decoder kinds).  The burden of candidate c for a patient on drugs S is
        sum_r weights[r] * P_r, P_r the probability of side effect r from the pairs (c, s), s in S: 1 - prod (1 - sigma) under
        'noisy_or', sigma(largest logit) under 'max' -- the expected weighted number of side effects c brings itself.
        regimens: as `regimen_side_effects` (each sorted and de-duplicated).  replace: None, or one drug id per regimen
        (-1: none): that drug is taken out of the context before scoring -- the substitution question; it may itself be a
        candidate, and its burden is then the baseline to compare against; ValueError when it is not a member.
        candidates: None = every drug (members of a regimen come back NaN); one list = shared by all regimens; a list of
        lists = one list per regimen (`normalize_add_on_queries`).  weights: None (every side effect counts 1) or one
        finite weight >= 0 per side effect -- per entry of `relations` when that is given --, e.g. a severity.
        exclude / relations: as `regimen_side_effects` -- a recorded (pair, side effect) does not contribute.
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> AddOnRisk(burden float32 [T], candidate int64 [T], ptr int64 [G + 1], best_burden float32 [G, k], best_drug
        int64 [G, k]) on the model's device: regimen g owns the tasks ptr[g]:ptr[g + 1] (flat CSR; for the two shared
        candidate forms `burden.view(G, C)`), burden NaN where a candidate is not applicable (a member of the context, an
        empty context, a NaN logit); best_*: the k candidates with the lowest burden, ascending, ties by position in the
        regimen's candidate list, padded with (+inf, -1)."""
        _refuse_sharded(self.shard, 'candidates')
        _check_known_mode('exclude', exclude)
        if aggregate not in ops.REGIMEN_AGGREGATES:
            raise ValueError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
        k = int(k)
        if k < 0:
            raise ValueError('k must be >= 0, not %d' % k)
        d = self.data
        drugs, ptr, cand, cand_ptr = normalize_add_on_queries(regimens, candidates, replace, d.n_drug,
                                                              ops.addon_max_context())
        rel_host = _relation_ids(relations, 'cpu')
        n_w = d.n_dd_et if rel_host is None else rel_host.numel()
        if weights is not None:
            try:
                weights = torch.as_tensor(weights).detach().to(torch.float32)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError('weights: one number per side effect expected') from None
            if weights.dim() != 1 or weights.numel() != n_w:
                raise ValueError('weights: %d entries expected (one per side effect%s), got shape %s'
                                 % (n_w, '' if rel_host is None else ' of `relations`', tuple(weights.shape)))
            if not bool((torch.isfinite(weights) & (weights >= 0)).all()):
                raise ValueError('weights must be finite and >= 0')
        dev = self.embeddings.device
        G, C = ptr.numel() - 1, cand.numel()
        if cand_ptr is None:
            cand_flat, task_ptr = cand.to(torch.int64).repeat(G), C * torch.arange(G + 1, dtype=torch.int64)
        else:
            cand_flat, task_ptr = cand.to(torch.int64), cand_ptr
        both = torch.cat([ptr, task_ptr, drugs.to(torch.int64), cand_flat]).to(dev)            # one upload
        ptr_d, task_ptr_d = both[:G + 1], both[G + 1:2 * G + 2]
        drugs_d, cand_flat_d = both[2 * G + 2:2 * G + 2 + drugs.numel()], both[2 * G + 2 + drugs.numel():]
        cand_d = cand_flat_d[:C] if cand_ptr is None else cand_flat_d
        rel = None if rel_host is None else rel_host.to(dev)
        known = _pair_known(d, exclude, rel)
        with torch.no_grad():
            w_d = None if weights is None else weights.to(dev)
            z, decoder = _scoring_operands(self, calibration)
            burden, best_b, best_p = decoder.addon_burden(z, drugs_d, ptr_d, cand_d,
                                                          None if cand_ptr is None else task_ptr_d, k, aggregate, w_d,
                                                          known, rel)
            if k == 0:
                best_b = torch.empty((G, 0), dtype=torch.float32, device=dev)
                best_drug = torch.empty((G, 0), dtype=torch.int64, device=dev)
            else:
                best_drug = _ids_at(best_p, cand_flat_d, task_ptr_d[:-1, None])
        return AddOnRisk(burden.reshape(-1), cand_flat_d, task_ptr_d, best_b, best_drug)

    def combination_risk(self, slots, fixed=None, k=10, aggregate='noisy_or', weights=None, relations=None, exclude=None,
                         calibration=None):
        """Serving (extension): the TOTAL expected side-effect burden of every regimen that takes one alternative per open
        slot on top of the fixed drugs, and the k safest combinations (`decoder.combination_burden`:
        `tipk_distmult_combo_burden` / `tipk_pair_table_combo_burden` on `self.embeddings`, under no_grad; both decoder
        kinds).  The burden of a regimen is sum_r weights[r] * P_r with P_r over ALL its pairs -- 1 - prod (1 - sigma) under
        'noisy_or', sigma(largest logit) under 'max' --, which is not additive over drugs: every combination is scored.
        slots / fixed: as `normalize_combination_queries` -- one query (a list of slots) or a list of queries; an
        alternative of -1 leaves its slot empty, so `[[d, -1] for d in drugs]` asks which drugs of a list to stop.
        weights / relations / exclude: exactly as `add_on_risk`.
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> CombinationRisk(burden float32 [T], ptr int64 [G + 1], best_burden float32 [G, k], best_combination int64 [G, k],
        best_drugs int64 [G, k, S_max]) on the model's device: query g owns burden[ptr[g]:ptr[g + 1]], a combination's index
        is its position there, the last slot running fastest (itertools.product); NaN where a combination takes a drug
        twice (two slots, or a slot and the fixed list) or a logit is NaN.  best_*: ascending burden, ties by combination
        index, padded with (+inf, -1); best_drugs: the drug chosen in every slot, -1 for an empty slot, for a slot the query
        does not have (S_max is the largest slot count) and for padding."""
        _refuse_sharded(self.shard, 'combinations')
        _check_known_mode('exclude', exclude)
        if aggregate not in ops.REGIMEN_AGGREGATES:
            raise ValueError("aggregate must be 'max' or 'noisy_or', not %r" % (aggregate,))
        k = int(k)
        if k < 0:
            raise ValueError('k must be >= 0, not %d' % k)
        d = self.data
        fix, fptr, alt, aptr, sptr = normalize_combination_queries(slots, fixed, d.n_drug, ops.combo_limits())
        rel_host = _relation_ids(relations, 'cpu')
        n_w = d.n_dd_et if rel_host is None else rel_host.numel()
        if weights is not None:
            try:
                weights = torch.as_tensor(weights).detach().to(torch.float32)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError('weights: one number per side effect expected') from None
            if weights.dim() != 1 or weights.numel() != n_w:
                raise ValueError('weights: %d entries expected (one per side effect%s), got shape %s'
                                 % (n_w, '' if rel_host is None else ' of `relations`', tuple(weights.shape)))
            if not bool((torch.isfinite(weights) & (weights >= 0)).all()):
                raise ValueError('weights must be finite and >= 0')
        dev = self.embeddings.device
        plan = ops.combo_plan(fix, fptr, alt, aptr, sptr, dev)
        G = plan.n_q
        rel = None if rel_host is None else rel_host.to(dev)
        known = _pair_known(d, exclude, rel)
        with torch.no_grad():
            w_d = None if weights is None else weights.to(dev)
            z, decoder = _scoring_operands(self, calibration)
            burden, ptr_d, best_b, best_c = decoder.combination_burden(z, plan, k, aggregate, w_d, known, rel)
            size = sptr[1:] - sptr[:-1]
            s_max = int(size.max()) if G else 0
            if k == 0:
                best_b = torch.empty((G, 0), dtype=torch.float32, device=dev)
                best_c = torch.empty((G, 0), dtype=torch.int64, device=dev)
                best_drugs = torch.empty((G, 0, s_max), dtype=torch.int64, device=dev)
            else:
                # digit s of a combination index, last slot fastest: (c // prod_{t > s} A_t) % A_s
                A = torch.ones((G, s_max + 1), dtype=torch.int64)
                first = torch.zeros((G, max(s_max, 1)), dtype=torch.int64)
                for g in range(G):
                    s0, n_s = int(sptr[g]), int(size[g])
                    A[g, :n_s] = aptr[s0 + 1:s0 + n_s + 1] - aptr[s0:s0 + n_s]
                    first[g, :n_s] = aptr[s0:s0 + n_s]
                A[:, s_max] = 1
                after = torch.flip(torch.cumprod(torch.flip(A, [1]), 1), [1])[:, 1:] if s_max else A[:, :0]
                A_d, after_d, first_d = A[:, :s_max].to(dev), after.to(dev), first[:, :s_max].to(dev)
                best_c = best_c.to(torch.int64)
                digit = torch.div(best_c[:, :, None].clamp(min=0), after_d[:, None, :], rounding_mode='floor') % A_d[:, None, :]
                has = (torch.arange(s_max)[None, :] < size[:, None]).to(dev)[:, None, :] & (best_c >= 0)[:, :, None]
                alt_d = torch.cat([plan.alt.to(torch.int64), plan.alt.new_zeros(1, dtype=torch.int64)])
                best_drugs = torch.where(has, alt_d[(first_d[:, None, :] + digit).clamp(max=alt_d.numel() - 1)],
                                         torch.full_like(digit, -1))
        return CombinationRisk(burden, ptr_d, best_b, best_c, best_drugs)

    def rank_side_effects(self, triples=None, filter='all', ks=(1, 3, 10), relations=None):
        """Evaluation of what `side_effects` serves (extension): where each given (drug, drug, side effect) triple lands
        among the side effects not recorded for its pair, and filtered MRR / Hits@k over the triples
        (`decoder.relation_ranks`: one `tipk_distmult_pair_rank` / `tipk_pair_table_pair_rank` launch on `self.embeddings`,
        under no_grad; both decoder kinds).
        triples: None = the held-out set (data.dd_test_idx, data.dd_test_et), else (edge_index int [2, T], edge_type int
        [T]); a triple is ranked for its pair as given, (u, v) and (v, u) apart.  filter: 'all' drops the pair's other train
        and test side effects (the standard filtered setting), 'train' only its training ones -- what
        `side_effects(exclude='train')` shows: other held-out side effects compete -- and None nothing (the raw rank); a
        recorded side effect is dropped in either pair direction, the triple's own never.  relations: candidate side-effect
        ids (None = all); a triple whose side effect is not among them is not ranked.  Ranks are 1-based on the logit, ties
        by ascending position in `relations`: rank - 1 is the triple's position in `side_effects` under the same filter.
        -> RankReport(rank int64 [T] (0 = not ranked), logit [T] (NaN there), mrr, hits {k: share of ranks <= k},
        per_relation {'count' [R], 'mrr' [R], 'hits' [len(ks), R]}, macro_mrr, unranked): `utils.rank_report` of the ranks;
        the tensors are on the model's device, in the triples' order."""
        _refuse_sharded(self.shard, 'side effects')
        _check_known_mode('filter', filter)
        d = self.data
        dev = self.embeddings.device
        idx, et = _checked_triples(triples, d, dev)
        rel = _relation_ids(relations, dev)
        known = _pair_known(d, filter, rel)
        tgt = et
        if rel is not None:
            pos = torch.full((d.n_dd_et,), -1, dtype=torch.int64, device=dev)
            pos[rel] = torch.arange(rel.numel(), device=dev)
            tgt = pos[et]                                                # -1: not a candidate, not ranked
        with torch.no_grad():
            pairs, tgt_ptr, tgt_rel, order = ops.targets_by_pair(idx, tgt, d.n_drug)
            r, s = self.decoder.relation_ranks(self.embeddings, pairs, tgt_ptr, tgt_rel, known, rel)
            return _rank_result(order, r, s, et, d.n_dd_et, ks)

    def rank_partners(self, triples=None, filter='all', ks=(1, 3, 10)):
        """Evaluation of what `screen(drugs=...)` serves (extension): where the partner v of each given (drug u, drug v, side
        effect r) triple lands among all drugs when u is screened for r, and the entity-ranking filtered MRR / Hits@k over
        the triples (`decoder.partner_ranks`: one `tipk_distmult_partner_rank` / `tipk_pair_table_partner_rank` launch on
        `self.embeddings`, under no_grad; both decoder kinds).
        triples: None = the held-out set (data.dd_test_idx, data.dd_test_et), which is stored in both directions, so every
        pair is ranked as head and as tail; else (edge_index int [2, T], edge_type int [T]): v is ranked for the query
        (r, u) as given.  filter: 'all' drops u's other train and test partners for r (the standard filtered setting),
        'train' only its training ones -- exactly what `screen(exclude='train')` shows: rank - 1 is the triple's position
        there -- and None nothing (the raw rank); the keys are `screen`'s, a recorded pair is dropped in either direction,
        the triple's own partner never.  u itself is no candidate, and a triple with v == u is not ranked.  Ranks are
        1-based on the logit, ties by ascending drug id.
        -> RankReport(rank int64 [T] (0 = not ranked), logit [T] (NaN there), mrr, hits {k: share of ranks <= k},
        per_relation {'count' [R], 'mrr' [R], 'hits' [len(ks), R]} -- the per-side-effect partner MRR --, macro_mrr,
        unranked): `utils.rank_report` of the ranks; the tensors are on the model's device, in the triples' order."""
        _refuse_sharded(self.shard, 'partners')
        _check_known_mode('filter', filter)
        d = self.data
        dev = self.embeddings.device
        idx, et = _checked_triples(triples, d, dev)
        known = _screen_known(d, filter)
        with torch.no_grad():
            q_rel, q_drug, tgt_ptr, tgt_node, order = ops.targets_by_query(idx, et, d.n_drug)
            r, s = self.decoder.partner_ranks(self.embeddings, q_rel, q_drug, tgt_ptr, tgt_node, known)
            return _rank_result(order, r, s, et, d.n_dd_et, ks)

    def rank_pairs(self, triples=None, filter='all', ks=(1, 10, 50)):
        """Evaluation of what the relation screen `screen()` serves (extension): where the pair {u, v} of each given (drug u,
        drug v, side effect r) triple lands among ALL drug pairs not recorded for r, and filtered MRR / Hits@k over the
        triples, micro and per side effect (`decoder.pair_ranks`: one `tipk_distmult_screen_rank` call on `self.embeddings`,
        under no_grad; DistMult only, as `screen`).
        triples: None = the held-out set (data.dd_test_idx, data.dd_test_et), which is stored in both directions, so every
        pair appears twice with equal ranks; else (edge_index int [2, T], edge_type int [T]): (u, v) and (v, u) are one pair.
        filter: 'all' drops the train and test positives of r (the standard filtered setting), 'train' only its training
        ones -- exactly what `screen(exclude='train')` shows: rank - 1 is the pair's position there, and Hits@50 of side
        effect r is the share of its held-out pairs among that screen's 50 best -- and None nothing (the raw rank); the keys
        are `screen`'s, a recorded pair is dropped in either direction, the triple's own pair is never counted against itself.
        A triple with v == u is not ranked.  Ranks are 1-based on the screen's logit, ties by ascending key min * n + max.
        -> RankReport(rank int64 [T] (0 = not ranked), logit [T] (NaN there), mrr, hits {k: share of ranks <= k},
        per_relation {'count' [R], 'mrr' [R], 'hits' [len(ks), R]}, macro_mrr, unranked): `utils.rank_report` of the ranks;
        the tensors are on the model's device, in the triples' order."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('rank_pairs ranks DistMult logits over all pairs; the NN decoder has no screen kernel')
        _refuse_sharded(self.shard, 'pairs')
        _check_known_mode('filter', filter)
        d = self.data
        dev = self.embeddings.device
        idx, et = _checked_triples(triples, d, dev)
        known = _screen_known(d, filter)
        with torch.no_grad():
            q_rel, tgt_ptr, tgt_u, tgt_v, order = ops.targets_by_relation(idx, et, d.n_dd_et)
            r, s = self.decoder.pair_ranks(self.embeddings, q_rel, tgt_ptr, tgt_u, tgt_v, known)
            return _rank_result(order, r, s, et, d.n_dd_et, ks)

    def explain(self, triples=None, k=10, side='v', direction='raise'):
        """Why the model predicts what it predicts (extension): the logit of every given (drug u, drug v, side effect r)
        triple, split EXACTLY over the recorded interactions of one of its drugs.  The last encoder layer has no ReLU behind
        it and both decoders are linear in one drug's embedding with the other held fixed, so
            logit = offset + own + neighbours,   neighbours = the sum of one contribution per training interaction of the drug,
        and the k largest contributions are listed (`MyRGCNConv2.attribute`: one `tipk_rgcn_attribution` launch, no E x d
        temporary; both decoder kinds).
        triples: None = the held-out set, else (edge_index int [2, T], edge_type int [T]), as `rank_pairs`.  side: 'v'
        explains the second drug of every triple, 'u' the first.  direction: 'raise' lists the interactions that push the
        logit up most, largest first; 'lower' those that pull it down most, most negative first.
        The model is RE-ENCODED with its current parameters, layer by layer (`FMEncoder.encode_layers`, under no_grad);
        `self.embeddings` is not overwritten.  After a `forward()` with no optimiser step since, `logit` equals `pred`'s
        logit up to the rounding between the per-layer and the fused encoder route.
        -> Explanation(logit [T]: the decoder's logit of the re-encoded embeddings; offset [T]: the other drug's part (NN
        decoder; 0 for DistMult); own [T]: the part of the drug's own features; neighbours [T]: the sum of ALL its
        interactions' contributions; contribution [T, k], partner int64 [T, k], relation int64 [T, k]: the listed
        interactions -- the partner drug and side effect of each --, padded with (-inf, or +inf under 'lower'; -1; -1);
        degree int64 [T]: the drug's number of training interactions) on the model's device, in the triples' order."""
        _refuse_sharded(self.shard, 'interactions')
        if side not in ('u', 'v'):
            raise ValueError("side must be 'u' or 'v', not %r" % (side,))
        if direction not in ('raise', 'lower'):
            raise ValueError("direction must be 'raise' or 'lower', not %r" % (direction,))
        d = self.data
        dev = self.embeddings.device
        idx, et = _checked_triples(triples, d, dev)
        with torch.no_grad():
            h, z = self.encoder.encode_layers(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm,
                                              d.p_feat, d.pp_train_indices, d.dp_edge_index, d.dp_range_list)
            node, probe, offset = self.decoder.probe(z, idx, et, side)
            if self.decoder_kind == 'nn':
                logit = ops.pair_table_score(*self.decoder._tables(z), idx, et, sigmoid=False)
            else:
                logit = self.decoder(z, idx, et, sigmoid=False)
            lower = direction == 'lower'
            c, src, rel, own, total = self.encoder.rgcn2.attribute(h, d.dd_train_idx, d.dd_train_range, node,
                                                                   -probe if lower else probe, k)
            if lower:
                c, own, total = -c, -own, -total
            in_ptr = ops.in_edges_by_node(d.dd_train_idx, d.dd_train_range, h.shape[0])[0]
            return Explanation(logit, offset, own, total, c, src.to(torch.int64), rel.to(torch.int64),
                               in_ptr[node + 1] - in_ptr[node])

    def explain_proteins(self, triples=None, k=10, side='v', direction='raise', max_workspace_bytes=1 << 30):
        """Which protein targets a prediction rests on (extension): the logit of every given (drug u, drug v, side effect r)
        triple, split EXACTLY over every targeted protein -- the targets of the explained drug and those of the drugs it
        interacts with, two hops back -- and every drug's own feature row.  Both R-GCN layers are bias-free, the only
        non-linearity between the drug inputs and z is the ReLU behind rgcn1 and the P -> D stage is linear in the protein
        embeddings, so for the ReLU pattern of this model
            logit = offset + features + proteins,   proteins = the sum of one contribution per targeted protein,
        and the k largest contributions are listed (`ops.protein_attribution`: one `tipk_protein_attribution` call, a fused
        reverse pass on the fp32 matrix cores; both decoder kinds, both `mod`s).
        triples, side, direction: as `explain` ('lower' lists the proteins that pull the logit down most, most negative
        first).  The model is RE-ENCODED with its current parameters (`FMEncoder.fold_in_tables`, `encode_layers`, under
        no_grad); `self.embeddings` is not overwritten.
        -> ProteinExplanation(logit [T], offset [T] as `explain`; features [T]: the part of ALL drugs' own feature rows;
        proteins [T]: the sum over ALL targeted proteins; contribution [T, k], protein int64 [T, k], direct [T, k]: the
        listed proteins, and the part of each contribution that arrives through the explained drug's own targets (0 for a
        protein it does not target), padded with (-inf, or +inf under 'lower'; -1; 0); targets int64 [T]: the explained
        drug's number of P -> D edges) on the model's device, in the triples' order.
        NotImplementedError for a relation-sharded model, a layer with a bias, sizes `tipk_protein_attribution_supported`
        refuses, or a workspace above max_workspace_bytes; ValueError for a bad side or direction."""
        _refuse_sharded(self.shard, 'proteins')
        if side not in ('u', 'v'):
            raise ValueError("side must be 'u' or 'v', not %r" % (side,))
        if direction not in ('raise', 'lower'):
            raise ValueError("direction must be 'raise' or 'lower', not %r" % (direction,))
        d, enc = self.data, self.encoder
        r1, r2 = enc.rgcn1, enc.rgcn2
        if r1.bias is not None or r2.bias is not None or r1.shard is not None or r2.shard is not None:
            raise NotImplementedError('explain_proteins splits the sums of bias-free layers that hold every relation; a layer '
                                      'has a bias or a relation shard')
        ne, cat = enc.embed.shape[1], enc.mod == 'cat'
        p, pd = enc.pp_encoder.out_dim, enc.hgcn.out_dim
        if not ops.protein_attribution_supported(d.n_drug, d.n_prot, d.n_dd_et, r1.num_bases, ne, pd, p, r1.out_channels,
                                                 r2.out_channels, cat, k):
            raise NotImplementedError('explain_proteins: tipk_protein_attribution does not take these sizes (include/tipk.h 4o)')
        dev = self.embeddings.device
        idx, et = _checked_triples(triples, d, dev)
        need = ops.protein_attribution_workspace_bytes(d.n_drug, r1.num_bases, r1.out_channels, p, et.numel())
        if need > int(max_workspace_bytes):
            raise NotImplementedError('explain_proteins: the dense pair cells need a workspace of %d bytes, above '
                                      'max_workspace_bytes = %d' % (need, int(max_workspace_bytes)))
        with torch.no_grad():
            args = (d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm, d.p_feat, d.pp_train_indices,
                    d.dp_edge_index, d.dp_range_list)
            h_prot, x0, h = enc.fold_in_tables(*args)
            z = enc.encode_layers(*args)[1]
            node, probe, offset = self.decoder.probe(z, idx, et, side)
            if self.decoder_kind == 'nn':
                logit = ops.pair_table_score(*self.decoder._tables(z), idx, et, sigmoid=False)
            else:
                logit = self.decoder(z, idx, et, sigmoid=False)
            if cat:
                xe = x0[:, :ne]                                           # the rows the model itself read
            else:
                xe = enc._drug_feat.apply_table(d.d_feat, enc.embed).detach()
                if d.d_norm is not None:
                    xe = xe / torch.as_tensor(d.d_norm).to(device=dev, dtype=torch.float32).reshape(-1, 1)
            lower = direction == 'lower'
            targets = ops.targets_by_protein(d.dp_edge_index, d.n_prot, d.n_drug)
            c, prot, direct, features, proteins = ops.protein_attribution(
                h_prot, enc.hgcn.weight.detach(), xe, h, (r1.basis.detach(), r1.att.detach(), r1.root.detach()),
                (r2.basis.detach(), r2.att.detach(), r2.root.detach()),
                ops.in_edges_by_pair(d.dd_train_idx, d.dd_train_range, d.n_drug), targets, cat, node,
                -probe if lower else probe, k)
            if lower:
                c, features, proteins = -c, -features, -proteins
                direct = torch.where(prot >= 0, -direct, direct)
            return ProteinExplanation(logit, offset, features, proteins, c, prot.to(torch.int64), direct,
                                      targets[3].to(dev)[node])

    def embed_new_drugs(self, targets, interactions=None, features=None, d_norm=None):
        """Embed drugs that are NOT nodes of the training graph (extension): a compound known by its protein targets and
        perhaps a few recorded interactions, with the trained model frozen (`ops.drug_fold_in`: one `tipk_drug_fold_in`
        launch for all M drugs, no per-edge temporary).
        targets: a list of M lists of protein ids (possibly empty).  interactions: None, or a list of M lists of (partner
        drug id, side-effect id): each is one in-edge partner -> new drug; partners are EXISTING drugs; duplicates count.
        features: None = no drug feature (xd = 0), else dense or sparse [M, n_drug_feat]; xd = features @ encoder.embed /
        d_norm[:, None] (torch ops).  d_norm [M]: defaults to ones.
        A row of an R-GCN layer depends on the node's own input row and its in-neighbours' rows only, so the new rows come
        from the tables of `FMEncoder.fold_in_tables`: the model is RE-ENCODED with its current parameters (under no_grad);
        `self.embeddings` is not overwritten.
        The approximation: the existing drugs' embeddings are held fixed, as if the new edges were directed INTO the new
        drug only -- neither their degrees nor their neighbourhoods change, and new drugs do not see each other.
        -> NewDrugs(x0 [M, d0], h [M, n_hid1], z [M, n_hid2], degree int64 [M], n_targets int64 [M]) on the model's
        device.  The decoders take z as an argument, so with
            z_ext = torch.cat([model.embeddings, new.z])
        new drug i is node n_drug + i of `model.decoder(z_ext, idx, et)` and of the decoders' other queries.
        ValueError for an id out of range; NotImplementedError for a relation-sharded model, a layer with a bias, or widths
        `tipk_drug_fold_in_supported` refuses.  Both `mod`s."""
        _refuse_sharded(self.shard, 'new drugs')
        d, enc = self.data, self.encoder
        m = len(targets)
        if interactions is None:
            interactions = [()] * m
        if len(interactions) != m:
            raise ValueError('interactions: one list per new drug expected, got %d for %d' % (len(interactions), m))
        tgt = _csr_of_lists(targets, 1, (d.n_prot,), ('protein',), 'targets')
        inter = _csr_of_lists(interactions, 2, (d.n_drug, d.n_dd_et), ('partner drug', 'side-effect'), 'interactions')
        r1, r2 = enc.rgcn1, enc.rgcn2
        if r1.bias is not None or r2.bias is not None:
            raise NotImplementedError('embed_new_drugs folds into bias-free R-GCN layers')
        ne, cat = enc.embed.shape[1], enc.mod == 'cat'
        if not ops.drug_fold_in_supported(d.n_drug, d.n_prot, d.n_dd_et, r1.num_bases, ne, enc.pp_encoder.out_dim,
                                          enc.hgcn.out_dim, r1.out_channels, r2.out_channels, cat):
            raise NotImplementedError('embed_new_drugs: tipk_drug_fold_in does not take these widths (include/tipk.h 4k)')
        dev = self.embeddings.device
        with torch.no_grad():
            if features is None:
                xd = torch.zeros((m, ne), dtype=torch.float32, device=dev)
            else:
                features = torch.as_tensor(features).to(dev)
                if features.dim() != 2 or tuple(features.shape) != (m, enc.embed.shape[0]):
                    raise ValueError('features: [%d, %d] expected, got %s' % (m, enc.embed.shape[0], tuple(features.shape)))
                mm = torch.sparse.mm if features.is_sparse else torch.mm
                xd = mm(features.to(torch.float32), enc.embed.detach())
                if d_norm is not None:
                    xd = xd / torch.as_tensor(d_norm).to(device=dev, dtype=torch.float32).reshape(m, 1)
            h_prot, x0, h = enc.fold_in_tables(d.d_feat, d.dd_train_idx, d.dd_train_et, d.dd_train_range, d.d_norm,
                                               d.p_feat, d.pp_train_indices, d.dp_edge_index, d.dp_range_list)
            tgt, inter = tuple(t.to(dev) for t in tgt), tuple(t.to(dev) for t in inter)
            x0n, hn, zn = ops.drug_fold_in(h_prot, enc.hgcn.weight.detach(), x0, h,
                                           (r1.basis.detach(), r1.att.detach(), r1.root.detach()),
                                           (r2.basis.detach(), r2.att.detach(), r2.root.detach()), xd.contiguous(), tgt, inter, cat)
            return NewDrugs(x0n, hn, zn, inter[0][1:] - inter[0][:-1], tgt[0][1:] - tgt[0][:-1])

    def calibrate(self, pairs=None, relations=None, l2=1e-6, init=None, max_iter=32, gtol=1e-6):
        """Calibrate the side-effect probabilities (extension): per side effect r a Platt map logit' = a_r logit + b_r, fitted
        on held-out positives against ALL unrecorded pairs at their true prevalence (`ops.distmult_calibrate`: one
        `tipk_distmult_calibrate` call enqueues every Newton step for all side effects; under no_grad on `self.embeddings`;
        include/tipk.h section 4r).  The model is trained on one uniform negative per positive, so sigma(logit) sits at a
        1:1 class balance: rankings are sound, expected counts are inflated.  The map keeps every ranking inside a side
        effect (a_r > 0) and fixes the level.
        pairs: None = the held-out set (data.dd_test_idx, data.dd_test_et), else (edge_index [2, T], edge_type [T]); both
        directions and repeats are one pair, self pairs are dropped, a pair that is a training pair of its side effect is
        dropped and counted.  relations: the side effects to fit (None = all); the others keep (1, 0) and status 4, and so
        does one without a positive or without a negative.  For side effect r with POS its given cells, NEG every other
        unordered pair that is not a training pair of r, M = |POS| + |NEG| and t = a s + b:
            1/M [ sum_POS softplus(-t) + sum_NEG softplus(t) ] + l2/2 (a - 1)^2,
        convex in (a, b).  l2 only bounds a on a separable list; 1e-6 is a modelling default.  init: None = (1, log((n_pos +
        .5) / (n_neg + .5))), the prevalence start, or [R, 2].  gtol: the fit ends when max |gradient| <= gtol; the default
        sits above the noise floor of the fp32 gradient.
        -> `Calibration`; pass it as `calibration=` to `side_effects`, `regimen_side_effects`, `add_on_risk`,
        `combination_risk`, `drug_profile` and `screen`.  It is a snapshot: calibrate again after further training.
        NotImplementedError for the NN decoder, a relation-sharded model, or sizes `tipk_distmult_calibrate_supported`
        refuses (include/tipk.h 4r); ValueError for l2 < 0, gtol < 0, max_iter < 0, an id out of range or an `init` of the
        wrong shape."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('calibrate fits a map of the DistMult logit; this model scores with the NN decoder '
                                      '(include/tipk.h 4r)')
        _refuse_sharded(self.shard, 'calibrated side effects')
        if not float(l2) >= 0:
            raise ValueError('l2 must be >= 0, not %r' % (l2,))
        if not float(gtol) >= 0:
            raise ValueError('gtol must be >= 0, not %r' % (gtol,))
        if int(max_iter) < 0:
            raise ValueError('max_iter must be >= 0, not %r' % (max_iter,))
        d = self.data
        n, n_rel, dim = d.n_drug, d.n_dd_et, self.decoder.in_dim
        if init is not None:
            init = torch.as_tensor(init)
            if tuple(init.shape) != (n_rel, 2):
                raise ValueError('init: [%d, 2] expected, got %s' % (n_rel, tuple(init.shape)))
        idx, et = _checked_triples(pairs, d, 'cpu')
        rel = torch.arange(n_rel, dtype=torch.int64) if relations is None else _relation_ids(relations, 'cpu')
        if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= n_rel):
            raise ValueError('side-effect id out of range: [%d, %d] for %d side effects' % (int(rel.min()), int(rel.max()), n_rel))
        rel = torch.unique(rel)
        if not ops.distmult_calibrate_supported(n, dim, n_rel) or not ops.distmult_calibrate_supported(n, dim + 4, n_rel):
            raise NotImplementedError('calibrate: tipk_distmult_calibrate does not take n = %d, dim = %d, %d side effects '
                                      '(include/tipk.h 4r)' % (n, dim, n_rel))
        with torch.no_grad():
            z, w = self.embeddings.detach(), self.decoder.weight.detach()
            dev = z.device
            train = (d.dd_train_idx, d.dd_train_et)
            every = ops.calibration_lists(train, (idx, et), n, n_rel)                  # ONE pass over the triples: all side effects
            ident = torch.zeros((n_rel, 2), dtype=torch.float32, device=dev)
            ident[:, 0] = 1.0
            loss_raw, grad_raw, _ = ops.distmult_calibrate_stats(z, w, ident, every, 0.0)
            m_all = (every.n_pos + every.n_neg).to(dev)
            n_pos_d = every.n_pos.to(dev)
            # dL/db = (sum of sigma over POS and NEG - n_pos) / M
            expected_raw = grad_raw[:, 1].double() * m_all.double() + n_pos_d.double()
            fit_rel = rel[(every.n_pos[rel] > 0) & (every.n_neg[rel] > 0)]
            ab = ident.clone()
            loss = loss_raw.clone()
            evals = torch.zeros(n_rel, dtype=torch.int64, device=dev)
            status = torch.full((n_rel,), 4, dtype=torch.int64, device=dev)
            if fit_rel.numel():
                cl = ops.calibration_queries(every, fit_rel)                         # query r of `every` is side effect r
                if init is None:
                    start = torch.stack([torch.ones(fit_rel.numel(), dtype=torch.float64),
                                         torch.log((cl.n_pos.double() + .5) / (cl.n_neg.double() + .5))], 1)
                else:
                    start = init.detach().to('cpu')[fit_rel]
                got, l_fit, _, info = ops.distmult_calibrate(z, w, cl, l2, start.to(dev, torch.float32), int(max_iter),
                                                             float(gtol))
                at = fit_rel.to(dev)
                ab[at], loss[at] = got, l_fit
                evals[at], status[at] = info[:, 1].to(torch.int64), info[:, 0].to(torch.int64)
            wide, dec = calibrated_operands(z, w, ab)
            return Calibration(ab[:, 0].clone(), ab[:, 1].clone(), loss, loss_raw, expected_raw.to(torch.float32),
                               n_pos_d, every.n_neg.to(dev), every.n_dropped.to(dev), evals, status, wide, dec)

    def fit_side_effects(self, pairs, l2=1e-4, neg_weight=1.0, init=None, max_iter=16, gtol=1e-5, new=None):
        """Learn side effects the model was NOT trained on (extension): one row of the DistMult decoder per new side effect
        from its recorded drug pairs, with the embeddings frozen (`ops.distmult_fit`: one `tipk_distmult_fit` call enqueues
        every Newton step for all B rows; under no_grad on `self.embeddings`).
        pairs: a list of B lists of (u, v), or (edge_index [2, P], ptr [B + 1]) (`ops.fit_pairs_csr`): unordered, duplicates
        count.  The row minimises the expectation of the training objective over its negative draw,
            1/P_b sum_listed softplus(-s) + neg_weight/N_b sum_{ordered (u, v) not recorded} softplus(s) + l2/2 |w|^2,
        a convex problem in dim unknowns.  init: None (zeros) or [B, dim], e.g. the row of a related side effect.
        new: the `NewDrugs` of `embed_new_drugs`; ids n_drug + i are then allowed and the fit runs on
        torch.cat([self.embeddings, new.z]) -- every drug of the wider set is a negative partner too.
        -> NewSideEffects(weight [B, dim], loss [B], grad_norm [B] (max |gradient|), evaluations int64 [B], status int64 [B]
        (1 converged, 2 step underflow, 3 non-finite statistic, 0 not converged in max_iter + 1 evaluations), n_pairs int64
        [B], decoder, known).  decoder: a detached `MultiInnerProductDecoder` of the B rows alone -- its relation i is new side
        effect i; it is not registered in the model -- and known: the (keys, ptr) lists of the given pairs, both directions,
        so that decoder.screen(z, k, known=known) lists the most likely UNRECORDED pairs of each new side effect and
        decoder.partner_sums(...) gives its liability column.
        NotImplementedError for the NN decoder (the rows fitted are DistMult rows), a relation-sharded model, or widths
        `tipk_distmult_fit_supported` refuses; ValueError for l2 < 0, neg_weight <= 0, max_iter < 0, an id out of range or an
        `init` of the wrong shape."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('fit_side_effects fits DistMult rows; this model scores with the NN decoder')
        _refuse_sharded(self.shard, 'new side effects')
        if not float(l2) >= 0:
            raise ValueError('l2 must be >= 0, not %r' % (l2,))
        if not float(neg_weight) > 0:
            raise ValueError('neg_weight must be > 0, not %r' % (neg_weight,))
        if int(max_iter) < 0:
            raise ValueError('max_iter must be >= 0, not %r' % (max_iter,))
        if not float(gtol) >= 0:
            raise ValueError('gtol must be >= 0, not %r' % (gtol,))
        n_all = self.data.n_drug + (0 if new is None else int(new.z.shape[0]))
        fp = ops.fit_pairs_csr(pairs, n_all, neg_weight)
        b, dim = fp.dense_w.numel(), self.decoder.in_dim
        if init is not None:
            init = torch.as_tensor(init)
            if tuple(init.shape) != (b, dim):
                raise ValueError('init: [%d, %d] expected, got %s' % (b, dim, tuple(init.shape)))
        if not ops.distmult_fit_supported(n_all, dim, max(b, 1)):
            raise NotImplementedError('fit_side_effects: tipk_distmult_fit does not take n = %d, dim = %d, %d side effects '
                                      '(include/tipk.h 4m)' % (n_all, dim, b))
        with torch.no_grad():
            z = self.embeddings.detach()
            dev = z.device
            if new is not None:
                z = torch.cat([z, new.z.detach().to(dev)])
            if init is not None:
                init = init.detach().to(dev, torch.float32)
            w, loss, grad, info = ops.distmult_fit(z, fp, l2, init, int(max_iter), float(gtol))
            dec = MultiInnerProductDecoder(dim, b).to(dev)
            dec.weight.data.copy_(w)
            dec.weight.requires_grad_(False)
            info = info.to(torch.int64)
            gn = grad.abs().amax(dim=1) if b else grad.new_zeros(0)
            return NewSideEffects(w, loss, gn, info[:, 1], info[:, 0], fp.n_pairs.to(dev), dec,
                                  tuple(t.to(dev) for t in fp.known))

    def fit_new_drugs(self, interactions, prior=None, init=None, l2=1e-4, neg_weight=1.0, max_iter=16, gtol=1e-5):
        """Fit the embedding of drugs that are NOT nodes of the training graph directly to the (partner drug, side effect)
        reports recorded for them (extension): the dual of `fit_side_effects`, with the embeddings AND the DistMult decoder
        frozen (`ops.distmult_drug_fit`: one `tipk_distmult_drug_fit` call enqueues every Newton step for all M drugs; under
        no_grad on `self.embeddings` and `self.decoder.weight`).
        interactions: a list of M lists of (partner drug id, side-effect id), or (index [2, P], ptr [M + 1])
        (`ops.drug_fit_csr`): partners are EXISTING drugs; duplicates count.  Row x of drug a minimises the expectation of the
        training objective over its negative draw,
            1/P_a sum_listed softplus(-s) + neg_weight/N_a sum_{(v, r) not recorded} softplus(s) + l2/2 |x - c_a|^2,
        s(v, r) = sum_k x[k] z[v,k] w[r,k]: a convex problem in dim unknowns.  The drug's pair with itself and pairs among new
        drugs are not part of it -- the approximation of `embed_new_drugs`.
        prior: the centres c_a -- None (zeros), a tensor [M, dim] or the `NewDrugs` of `embed_new_drugs`, whose .z is used;
        init: the start, given the same way; None starts at the prior.  The intended call
            new = model.embed_new_drugs(targets, interactions)
            fit = model.fit_new_drugs(interactions, prior=new, l2=...)
        starts from the fold-in row and moves it as far as the evidence says: l2 weighs the fold-in against the reports.
        -> FittedDrugs(z [M, dim], loss [M], grad_norm [M] (max |gradient|), evaluations int64 [M], status int64 [M] (1
        converged, 2 step underflow, 3 non-finite statistic, 0 not converged in max_iter + 1 evaluations), n_interactions int64
        [M], hess [M, dim, dim]: the Hessian of the objective at z).  Every `new=` argument of the queries reads .z only, so the
        result goes wherever a `NewDrugs` goes, and torch.cat([model.embeddings, fit.z]) through every decoder query.
        NotImplementedError for the NN decoder (its logit is not linear in z: the fit is not convex), a relation-sharded model,
        or widths `tipk_distmult_drug_fit_supported` refuses; ValueError for l2 < 0, neg_weight <= 0, max_iter < 0, gtol < 0,
        an id out of range, or a `prior` / `init` of the wrong shape."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('fit_new_drugs fits against DistMult rows; this model scores with the NN decoder')
        _refuse_sharded(self.shard, 'new drugs')
        if not float(l2) >= 0:
            raise ValueError('l2 must be >= 0, not %r' % (l2,))
        if not float(neg_weight) > 0:
            raise ValueError('neg_weight must be > 0, not %r' % (neg_weight,))
        if int(max_iter) < 0:
            raise ValueError('max_iter must be >= 0, not %r' % (max_iter,))
        if not float(gtol) >= 0:
            raise ValueError('gtol must be >= 0, not %r' % (gtol,))
        n, n_rel, dim = self.data.n_drug, self.data.n_dd_et, self.decoder.in_dim
        fl = ops.drug_fit_csr(interactions, n, n_rel, neg_weight)
        m = fl.dense_w.numel()
        rows = {}
        for name, given in (('prior', prior), ('init', init)):
            if given is not None:
                given = torch.as_tensor(given.z if hasattr(given, 'z') else given)
                if tuple(given.shape) != (m, dim):
                    raise ValueError('%s: [%d, %d] expected, got %s' % (name, m, dim, tuple(given.shape)))
            rows[name] = given
        if not ops.distmult_drug_fit_supported(n, dim, n_rel, max(m, 1)):
            raise NotImplementedError('fit_new_drugs: tipk_distmult_drug_fit does not take n = %d, %d side effects, dim = %d, '
                                      '%d drugs (include/tipk.h 4q)' % (n, n_rel, dim, m))
        with torch.no_grad():
            z, w = self.embeddings.detach(), self.decoder.weight.detach()
            dev = z.device
            rows = {k: None if v is None else v.detach().to(dev, torch.float32) for k, v in rows.items()}
            x, loss, grad, info, hess = ops.distmult_drug_fit(z, w, fl, rows['prior'], l2, rows['init'], int(max_iter),
                                                              float(gtol))
            info = info.to(torch.int64)
            gn = grad.abs().amax(dim=1) if m else grad.new_zeros(0)
            return FittedDrugs(x, loss, gn, info[:, 1], info[:, 0], fl.n_interactions.to(dev), hess)

    def decoder_posterior(self, pairs=None, weight=None, relations=None, l2=1e-4, neg_weight=1.0, new=None):
        """How sure the decoder is of its rows (extension): a Gaussian (Laplace) posterior N(w_b, (P_b H_b)^-1) of DistMult
        rows, from the exact Hessian H_b of the objective `fit_side_effects` minimises (`ops.distmult_posterior`:
        `tipk_distmult_fit_stats`, then `tipk_spd_factor`; under no_grad on `self.embeddings`).  The objective is a mean, so
        counted in observations the negative log posterior is P_b L_b: P_b positives, neg_weight P_b observations' worth of
        weight on the unrecorded pairs, and a Gaussian prior of precision l2 P_b.
        pairs = None: the model's trained rows with, per side effect, its training pairs -- each unordered pair once;
        `relations` restricts the rows (None = all) and `relation` of the result holds global ids.  This is the same formula
        at the trained row: the Hessian is that of the objective the row was trained on, but l2 is a CHOSEN prior -- the
        model itself trains without one -- and the trained row need not be the optimum.
        Otherwise pairs is what `fit_side_effects` takes and weight [B, dim] the rows, e.g. `fitted.weight`: for a fitted row
        this is the Laplace approximation at its optimum (same l2 and neg_weight).  `relation` is 0..B-1 and `known` the
        given lists in pair-major form.  new: the `NewDrugs` of `embed_new_drugs`, as in `fit_side_effects`.
        The embeddings are treated as exact.  The reported spread is therefore a lower bound on the model's uncertainty.
        -> DecoderPosterior(weight [B, dim], factor [B, dim, dim], n_pairs int64 [B], relation int64 [B], known).
        ValueError for l2 <= 0, neg_weight <= 0, an id out of range, a `weight` of the wrong shape, a row without pairs, or
        rows whose factorisation failed (their ids are named); NotImplementedError for the NN decoder, a relation-sharded
        model, or sizes `tipk_distmult_fit_supported` refuses.  Reads the factor's status: one synchronisation."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('decoder_posterior is the posterior of DistMult rows; this model scores with the NN decoder')
        _refuse_sharded(self.shard, 'side effects')
        if not float(l2) > 0:
            raise ValueError('l2 must be > 0 (the prior keeps the Hessian positive definite), not %r' % (l2,))
        if not float(neg_weight) > 0:
            raise ValueError('neg_weight must be > 0, not %r' % (neg_weight,))
        d = self.data
        n_all = d.n_drug + (0 if new is None else int(new.z.shape[0]))
        dim = self.decoder.in_dim
        if pairs is None:
            if weight is not None:
                raise ValueError('weight: rows are given together with their pairs')
            rel = torch.arange(d.n_dd_et, dtype=torch.int64) if relations is None \
                else torch.as_tensor(relations).to('cpu', torch.int64).reshape(-1)
            if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= d.n_dd_et):
                raise ValueError('side-effect id out of range: [%d, %d] for %d side effects' % (int(rel.min()), int(rel.max()), d.n_dd_et))
            pairs = _training_pairs_of(d, rel)
        else:
            if relations is not None:
                raise ValueError('relations selects rows of the model; given rows are numbered 0..B-1')
            rel = None
        fp = ops.fit_pairs_csr(pairs, n_all, neg_weight)
        b = fp.dense_w.numel()
        if rel is None:
            rel = torch.arange(b, dtype=torch.int64)
            if weight is None:
                raise ValueError('weight: the rows [%d, %d] of the given pairs are needed' % (b, dim))
            weight = torch.as_tensor(weight)
            if tuple(weight.shape) != (b, dim):
                raise ValueError('weight: [%d, %d] expected, got %s' % (b, dim, tuple(weight.shape)))
        if not ops.distmult_fit_supported(n_all, dim, max(b, 1)):
            raise NotImplementedError('decoder_posterior: tipk_distmult_fit_stats does not take n = %d, dim = %d, %d side effects '
                                      '(include/tipk.h 4m)' % (n_all, dim, b))
        empty = torch.nonzero(fp.n_pairs == 0).reshape(-1)
        if empty.numel():
            raise ValueError('a posterior needs at least one recorded pair; side effects without: %s' % rel[empty].tolist()[:20])
        with torch.no_grad():
            z = self.embeddings.detach()
            dev = z.device
            if new is not None:
                z = torch.cat([z, new.z.detach().to(dev)])
            custom = weight is not None
            w = weight.detach().to(dev, torch.float32) if custom else self.decoder.weight.detach()[rel.to(dev)]
            w = w.contiguous()
            factor, _, status, _ = ops.distmult_posterior(z, w, fp, float(l2))
            bad = torch.nonzero(status == 0).reshape(-1).cpu()
            if bad.numel():
                raise ValueError('the Hessian of %d row(s) is not positive definite or not finite; side effects: %s'
                                 % (bad.numel(), rel[bad].tolist()[:20]))
            known = _pair_major_known(fp, n_all, dev) if custom else None
            return DecoderPosterior(w, factor, fp.n_pairs.to(dev), rel.to(dev), known)

    def side_effects_confidence(self, pairs, posterior, k=10, rank_by='moderated', z_score=1.645, exclude=None, dense=False,
                                new=None):
        """Serving (extension): `side_effects` with error bars -- for every drug pair of `pairs` [2, P] the k side effects of
        `posterior` (a `DecoderPosterior`) that rank highest once the spread of each logit under the posterior is taken into
        account (one `tipk_distmult_pair_conf_topk` launch on `self.embeddings`, under no_grad).  For the triple (u, v, b)
        with phi = z[u] * z[v]: logit s = phi . w_b, variance var = |W_b phi|^2.
        rank_by: 'moderated' ranks by MacKay's moderated probability sigma(s / sqrt(1 + pi var / 8)) -- an uncertain logit is
        pulled towards 1/2; 'lower' by s - z_score sqrt(var) (what the model is confident of); 'upper' by
        s + z_score sqrt(var) (what it cannot rule out).
        exclude: for the model's rows as `side_effects` ('train', 'all', None); only the posterior's side effects are
        candidates and global ids are returned.  For given rows True drops the pairs the rows were given with, None nothing.
        dense = True also returns every side effect's logit and std [P, B] (recorded ones included, columns in the
        posterior's order).  new: the `NewDrugs` the posterior was made with; ids n_drug + i are then allowed.
        The embeddings are treated as exact.  The reported spread is therefore a lower bound on the model's uncertainty.
        -> ConfidentSideEffects(probability [P, k] = the moderated probability, mean_probability = sigma(s), logit, std =
        sqrt(var), relation int64 [P, k], dense_logit, dense_std); padding: probabilities 0, logit -inf, std +inf, relation -1.
        ValueError for a bad rank_by, a z_score that is not finite, k outside 0..128, an id out of range or a bad exclude;
        NotImplementedError for the NN decoder, a relation-sharded model or sizes the entry refuses."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('side_effects_confidence ranks with DistMult rows; this model scores with the NN decoder')
        _refuse_sharded(self.shard, 'side effects')
        if rank_by not in ('moderated', 'lower', 'upper'):
            raise ValueError("rank_by must be 'moderated', 'lower' or 'upper', not %r" % (rank_by,))
        if not math.isfinite(float(z_score)):
            raise ValueError('z_score must be finite, not %r' % (z_score,))
        k = int(k)
        if k < 0 or k > 128:
            raise ValueError('k must be in 0..128, not %d' % k)
        custom = posterior.known is not None
        if custom:
            if exclude not in (True, False, None):
                raise ValueError('exclude must be True or None for given rows, not %r' % (exclude,))
        else:
            _check_known_mode('exclude', exclude)
        d = self.data
        n_all = d.n_drug + (0 if new is None else int(new.z.shape[0]))
        pairs = torch.as_tensor(pairs)
        if pairs.dim() != 2 or pairs.shape[0] != 2 or pairs.dtype.is_floating_point:
            raise ValueError('pairs: an int tensor [2, P] expected, got %s %s' % (pairs.dtype, tuple(pairs.shape)))
        if pairs.numel():
            lo, hi = torch.stack([pairs.min(), pairs.max()]).tolist()
            if lo < 0 or hi >= n_all:
                raise ValueError('drug id out of range: [%d, %d] for %d drugs' % (lo, hi, n_all))
        b, dim = posterior.weight.shape
        if b < 1 or not ops.distmult_pair_conf_topk_supported(n_all, dim, b, k):
            raise NotImplementedError('side_effects_confidence: tipk_distmult_pair_conf_topk does not take n = %d, dim = %d, '
                                      '%d side effects (include/tipk.h 4p)' % (n_all, dim, b))
        with torch.no_grad():
            z = self.embeddings.detach()
            dev = z.device
            if new is not None:
                z = torch.cat([z, new.z.detach().to(dev)])
            pairs = pairs.to(dev)
            if custom:
                known = posterior.known if exclude else None
            else:
                full = posterior.relation.numel() == d.n_dd_et and \
                    bool((posterior.relation == torch.arange(d.n_dd_et, device=posterior.relation.device)).all())
                known = _pair_known(d, exclude, None if full else posterior.relation.to(dev))
                if known is not None and n_all != d.n_drug:              # the lists are keyed u * n_drug + v: same pairs, same order
                    keys = known[0].to(torch.int64)
                    known = (torch.div(keys, d.n_drug, rounding_mode='floor') * n_all + keys % d.n_drug,) + tuple(known[1:])
            mode, c = (0, 0.0) if rank_by == 'moderated' else (1, -float(z_score) if rank_by == 'lower' else float(z_score))
            _, idx, logit, var, d_logit, d_var = ops.distmult_pair_conf_topk(z, posterior.weight, posterior.factor, pairs, k,
                                                                             mode, c, known, dense)
            have = idx >= 0
            zero = torch.zeros_like(logit)
            prob = torch.where(have, torch.sigmoid(logit / torch.sqrt(1.0 + (math.pi / 8) * var)), zero)
            mean = torch.where(have, torch.sigmoid(logit), zero)
            return ConfidentSideEffects(prob, mean, logit, torch.sqrt(var), _ids_at(idx, posterior.relation.to(dev)), d_logit,
                                        None if d_var is None else torch.sqrt(d_var))

    def drug_profile(self, drugs=None, k=10, exclude='all', relations=None, partner_weights=None, new=None, calibration=None):
        """Serving (extension): the liability profile of single drugs -- for every side effect, with how many OTHER drugs the
        model expects the drug to cause it, beyond the pairs already recorded (`decoder.partner_sums`: one
        `tipk_distmult_partner_sum` / `tipk_pair_table_partner_sum` call on `self.embeddings`, under no_grad; no N x N x R
        temporary; both decoder kinds).
            expected[q, j] = sum over partners c of partner_weights[c] * sigma(logit(relations[j], drugs[q], c)),
        over the drugs c != drugs[q] with a weight != 0 whose pair with drugs[q] is not recorded for the side effect.
        drugs: ids (None = all training drugs; repeats allowed).  exclude: 'all' drops the train and test pairs of the side
        effect, 'train' the training pairs, None nothing; a recorded pair is dropped in either direction.  relations:
        side-effect ids that become the columns (None = all), as `side_effects`; the returned ids are global.
        partner_weights: None (every partner counts 1, `expected` is a number of drugs) or one finite weight >= 0 per training
        drug, e.g. a co-prescription frequency.  The queried drug is the decoder's first argument.
        new: the `NewDrugs` of `embed_new_drugs`; an id n_drug + i in `drugs` then queries new drug i, on
        torch.cat([self.embeddings, new.z]).  The partners are the EXISTING drugs only (new drugs weigh 0, so they are never
        partners, of each other or of a training drug), and a new drug has no recorded list: nothing is dropped from its row.
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> DrugProfile(expected float32 [Q, R'], candidates int64 [Q, R']: the number of partners summed over, top_expected
        float32 [Q, k], top_relation int64 [Q, k]: the k side effects of each drug with the largest expectation, descending,
        ties by position in `relations`, padded with (-inf, -1)) on the model's device."""
        _refuse_sharded(self.shard, 'partners')
        _check_known_mode('exclude', exclude)
        d = self.data
        k = int(k)
        if k < 0 or k > 128:
            raise ValueError('k must be in 0..128, not %d' % k)
        n_new = 0 if new is None else int(new.z.shape[0])
        n_all = d.n_drug + n_new
        if drugs is None:
            q_host = torch.arange(d.n_drug, dtype=torch.int64)
        else:
            q_host = torch.as_tensor(drugs).to('cpu')
            if q_host.dtype.is_floating_point or q_host.dtype == torch.bool:
                raise ValueError('drugs: int ids expected, got %s' % q_host.dtype)
            q_host = q_host.to(torch.int64).reshape(-1)
        if q_host.numel() and (int(q_host.min()) < 0 or int(q_host.max()) >= n_all):
            raise ValueError('drug id out of range: [%d, %d] for %d drugs%s'
                             % (int(q_host.min()), int(q_host.max()), d.n_drug, ' and %d new ones' % n_new if new is not None else ''))
        rel_host = _relation_ids(relations, 'cpu')
        if rel_host is not None and rel_host.numel() and (int(rel_host.min()) < 0 or int(rel_host.max()) >= d.n_dd_et):
            raise ValueError('side-effect id out of range: [%d, %d] for %d side effects'
                             % (int(rel_host.min()), int(rel_host.max()), d.n_dd_et))
        if partner_weights is not None:
            try:
                partner_weights = torch.as_tensor(partner_weights).detach().to('cpu', torch.float32)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError('partner_weights: one number per drug expected') from None
            if partner_weights.dim() != 1 or partner_weights.numel() != d.n_drug:
                raise ValueError('partner_weights: %d entries expected (one per drug), got shape %s'
                                 % (d.n_drug, tuple(partner_weights.shape)))
            if not bool((torch.isfinite(partner_weights) & (partner_weights >= 0)).all()):
                raise ValueError('partner_weights must be finite and >= 0')
        dev = self.embeddings.device
        known = _screen_known(d, exclude)
        with torch.no_grad():
            z, decoder = _scoring_operands(self, calibration)
            pw = None if partner_weights is None else partner_weights.to(dev)
            if new is not None:
                z = torch.cat([z.detach(), new.z.detach().to(dev) if calibration is None else calibration.embed(new.z)])
                ones = torch.ones(d.n_drug, dtype=torch.float32, device=dev) if pw is None else pw
                pw = torch.cat([ones, torch.zeros(n_new, dtype=torch.float32, device=dev)])
                known = _rekeyed_known(known, d.n_drug, n_all)
            rel = None if rel_host is None else rel_host.to(dev)
            total, count, top_v, top_p = decoder.partner_sums(z, q_host.to(dev), k, rel, pw, known)
            top_rel = top_p.to(torch.int64) if rel is None else _ids_at(top_p, rel)
        return DrugProfile(total, count.to(torch.int64), top_v, top_rel)

    def screen(self, k=10, relations=None, drugs=None, exclude='train', sigmoid=True, calibration=None):
        """Serving (extension): the k drug pairs the model scores highest per side effect, among pairs not known to cause it
        (`MultiInnerProductDecoder.screen`, one `tipk_distmult_screen` call on `self.embeddings`, under no_grad).
        relations: side-effect ids (None = all); drugs: None = relation screen (pairs u < v), else the best partners v of
        each drug, drug-major.  exclude: 'train' drops the training positives (held-out test pairs can and do appear),
        'all' drops train and test positives (truly novel pairs), None drops nothing.  Ranking is on the logit; sigmoid
        = True applies sigma afterwards (padding: score sigma(-inf) = 0, u = v = -1).
        calibration: None, or the `Calibration` of `calibrate`: the query then runs on its widened operands, so every logit
        is scale[r] * logit + offset[r].  It is a SNAPSHOT of the embeddings -- calibrate again after further training --
        and rankings within one side effect do not change for scale > 0.
        -> ScreenResult(score [Q, k], u [Q, k], v [Q, k], relation [Q, k]) on the model's device."""
        if self.decoder_kind == 'nn':
            raise NotImplementedError('screen ranks DistMult logits over all pairs; the NN decoder has no screen kernel')
        _refuse_sharded(self.shard, 'screen')
        _check_known_mode('exclude', exclude)
        known = _screen_known(self.data, exclude)
        q = screen_queries(self.decoder.num_et, relations, drugs)
        with torch.no_grad():
            z, decoder = _scoring_operands(self, calibration)
            logit, u, v = decoder.screen(z, k, relations, drugs, known)
            score = torch.sigmoid(logit) if sigmoid else logit
        relation = q[:, 0].to(device=logit.device, dtype=torch.int64)[:, None].expand(-1, logit.shape[1])
        return ScreenResult(score, u, v, relation)

    def test(self, print_output=True):
        self.eval()
        d = self.data
        with torch.no_grad():
            pos_score = self.decoder(self.embeddings, d.dd_test_idx, d.dd_test_et)
            neg_score = self.decoder(self.embeddings, self.test_neg_index, d.dd_test_et)
        if self.shard is not None:
            return self.__sharded_test(pos_score, neg_score, print_output)
        return self.compute_auprc_auroc_ap_by_et(pos_score, neg_score, d.dd_test_range, print_output)

    def __sharded_test(self, pos_score, neg_score, print_output):
        """Per-relation metrics of the local relations, all-gathered into the full [3, R] record."""
        import torch.distributed as dist
        sh = self.shard
        local = auprc_auroc_ap_by_range(pos_score, neg_score, self.data.dd_test_range) if sh.rel_ids.numel() \
            else np.zeros((3, 0))
        parts = [None] * sh.world
        if dist.is_initialized():
            dist.all_gather_object(parts, (sh.rel_ids.cpu().numpy(), np.asarray(local)), group=sh.group)
        else:
            parts = [(sh.rel_ids.cpu().numpy(), np.asarray(local))]
        record = np.zeros((3, sh.n_relations))
        for ids, rec in parts:
            record[:, ids] = rec
        if print_output and sh.rank == 0:
            auprc, auroc, ap = record.sum(axis=1) / sh.n_relations
            print('On test set: auprc:{:0.4f}   auroc:{:0.4f}   ap@50:{:0.4f}    '.format(auprc, auroc, ap))
        return record

    def compute_auprc_auroc_ap_by_et(self, pos_score, neg_score, dd_range, print_out):
        record = auprc_auroc_ap_by_range(pos_score, neg_score, dd_range)      # [3, R]
        if print_out:
            auprc, auroc, ap = record.sum(axis=1) / self.data.n_dd_et
            print('On test set: auprc:{:0.4f}   auroc:{:0.4f}   ap@50:{:0.4f}    '.format(auprc, auroc, ap))
        return record
