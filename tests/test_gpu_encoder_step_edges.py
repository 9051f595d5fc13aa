"""The fused encoder step (tip_amd/encoder.py `_EncoderStep`) and its C handle (include/tipk.h section 10d) against fp64 on the edge
graphs of tests/encoder_cases.py (-m gpu): empty and one-edge relations, drugs without targets or in-edges, a hub, duplicate
triples, node counts that are no multiple of a tile, the 1 024-drug limit, the last R of one LDS column block, a dense and a
one-edge D-D graph, a 9-drug graph.

Every tensor -- z and all twelve gradients -- is compared elementwise, nothing excluded: |got - want| <= k 2^-24 A with A and k
from the case (`encoder_cases.magnitude`, `chain_lengths`); tests/test_host_encoder_cases.py shows on the CPU that both ReLUs
are clear of their kink and that one dropped, doubled or misfiled edge moves some element by at least 10 bounds.  The C handle
must give the bits of the Python step (the header's promise), for both weight layouts and both index widths, and must refuse
exactly what `encoder.usable` refuses.  Every comparison prints its ratio (`-s`); profiles/encoder_step_errors.md records them."""
import ctypes as C
import os
import sys
import time

import pytest
import torch

import encoder_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import c_abi_encoder_host as host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SMALL = 'cat_sym_41'                                     # the case the one-off variations run on


@pytest.fixture(scope='module')
def lib():
    return host.load_library()


def _graphs(case):
    d = case.data
    rel = E.O._relation_of_edges(d['dd_train_range'], d['dd_train_idx'].shape[1])
    return {k: d[k].to(DEV) for k in ('pp_train_indices', 'dp_edge_index', 'dd_train_idx', 'dd_train_range')}, rel.to(DEV), d['d_norm'].to(DEV)


def _module(case, params=None):
    from tip_amd.layers import FMEncoder
    enc = FMEncoder(DEV, case.n_drug, case.R, case.n_prot, case.n_prot, case.n_drug, prot_drug_dim=case.pd_dim, num_base=E.NB,
                    n_embed=case.n_embed, n_hid1=E.HID1, n_hid2=case.n_hid2, mod=case.mod)
    sd = enc.state_dict()
    assert set(sd) == set(E.STATE)
    enc.load_state_dict({k: (params or case.params)[k].clone() for k in sd})
    return enc.to(DEV)


def _args(case, g, rel, d_norm):
    from tip_amd.utils import sparse_id
    return (sparse_id(case.n_drug).to(DEV), g['dd_train_idx'], rel, g['dd_train_range'], d_norm, sparse_id(case.n_prot).to(DEV),
            g['pp_train_indices'], g['dp_edge_index'], None)


def _python_pass(enc, args, up):
    """one forward + backward pass -> (z, {state_dict name: gradient}, launches, route)."""
    from tip_amd import ops
    enc.zero_grad(set_to_none=True)
    ops.timing_start()
    try:
        z = enc(*args)
        z.backward(up)
        torch.cuda.synchronize()
    finally:
        rec = ops.timing_stop()
    grads = {k: p.grad.clone() for k, p in enc.named_parameters()}
    return z.detach().clone(), grads, sum(v[0] for v in rec.values()), enc.last_route


def _check(case, name, got, where):
    r = case.ratio(name, got)
    print('RATIO %s %s %s %.4f (k = %d)' % (case.id, where, name, r, case.k[name]))
    assert r <= 1, (case.id, where, name, r, case.k[name])


def _dims(case):
    return host.Dims(case.n_embed, case.pd_dim, E.HID1, case.n_hid2, E.NB, int(case.mod == 'cat'))


def _handle(lib, case, g, idx_bytes=8):
    return host.Encoder(lib, g['pp_train_indices'], g['dp_edge_index'], g['dd_train_idx'], g['dd_train_range'], case.n_prot, case.n_drug,
                        _dims(case), DEV, idx_bytes)


def _state(enc, layout):
    """the 12 tensors: as the module stores them (GCN weights [in, out] in memory: lin_layout 1) or contiguous (lin_layout 0)."""
    sd = dict(enc.named_parameters())
    t = {k: sd[s].detach() for k, s in zip(host.NAMES, host.STATE)}
    return t if layout else {k: v.contiguous() for k, v in t.items()}


def _c_step(h, prm, layout, d_norm, up, flags=host.FROM_FWD):
    p = h.params(prm, layout)
    z = torch.full(tuple(up.shape), float('nan'), device=DEV)
    grads = {k: torch.empty_strided(v.shape, v.stride(), device=DEV).fill_(float('nan')) for k, v in prm.items()}
    assert h.forward(p, d_norm, z) == 0
    assert h.backward(p, d_norm, up, grads, flags) == 0
    torch.cuda.synchronize()
    return z, grads


def _same_bits(case, what, z, grads, z_py, g_py):
    assert torch.equal(z, z_py), (case.id, what, 'z')
    for k, s in zip(host.NAMES, host.STATE):
        assert grads[k].shape == g_py[s].shape and torch.equal(grads[k], g_py[s]), (case.id, what, s)


@pytest.mark.parametrize('cid', E.CASE_IDS)
def test_step_and_handle(cid, lib, monkeypatch):
    monkeypatch.delenv('TIPK_NO_ENCODER_STEP', raising=False)
    t0 = time.time()
    case = E.case(cid)
    g, rel, d_norm = _graphs(case)
    enc = _module(case)
    args = _args(case, g, rel, d_norm)
    up = case.upstream.to(DEV)
    # the two decisions: `encoder.usable` (through the module's own plans) and tipk_encoder_build
    fused = enc.fused_plans(args[0], args[1], args[3], args[4], args[5], args[6], args[7]) is not None
    h = _handle(lib, case, g)
    try:
        assert h.status in (0, host.TIPK_EUNSUPPORTED), h.status
        assert (h.status == 0) == bool(h.h.value)
        assert fused == (h.status == 0), (cid, 'usable', fused, 'tipk_encoder_build', h.status)
        if case.expect != 'any':
            assert fused == (case.expect == 'fused'), (cid, fused)
        # the module, on whatever route it takes
        z, grads, launches, route = _python_pass(enc, args, up)
        assert route == ('encoder_step' if fused else 'per_layer')
        if fused:
            assert launches == 16, launches
        _check(case, 'z', z, route)
        for s in E.STATE:
            _check(case, 'grad.' + s, grads[s], route)
        # a second pass on the cached plans: the same bits
        z_b, grads_b, launches_b, _ = _python_pass(enc, args, up)
        assert launches_b == launches and torch.equal(z_b, z)
        for s in E.STATE:
            assert torch.equal(grads_b[s], grads[s]), s
        if not fused:
            print('WALL %s %.2f s (%s)' % (cid, time.time() - t0, route))
            return
        # the C handle: the Python step's bits, for both layouts of the GCN weights and both index widths
        for idx_bytes in (8, 4):
            h2 = h if idx_bytes == 8 else _handle(lib, case, g, 4)
            try:
                assert h2.status == 0, (idx_bytes, h2.status)
                for layout in (1, 0):
                    zc, gc = _c_step(h2, _state(enc, layout), layout, d_norm, up)
                    _same_bits(case, (idx_bytes, layout), zc, gc, z, grads)
            finally:
                if h2 is not h:
                    h2.close()
        _check(case, 'z', zc, 'c_handle')
    finally:
        h.close()
    print('WALL %s %.2f s (encoder_step + 4 handle passes)' % (cid, time.time() - t0))


def test_null_d_norm_is_a_norm_of_ones(lib):
    """d_norm = NULL ("nullable = 1"): the bits of a tensor of ones, and within the bound of the fp64 reference with d_norm = 1."""
    case = E.case(SMALL, unit_norm=True)
    g, rel, d_norm = _graphs(case)
    assert bool((d_norm == 1).all())
    enc = _module(case)
    up = case.upstream.to(DEV)
    h = _handle(lib, case, g)
    try:
        assert h.status == 0
        z1, g1 = _c_step(h, _state(enc, 1), 1, d_norm, up)
        z0, g0 = _c_step(h, _state(enc, 1), 1, None, up)
        assert torch.equal(z0, z1)
        for k in host.NAMES:
            assert torch.equal(g0[k], g1[k]), k
        _check(case, 'z', z0, 'null_d_norm')
        for k, s in zip(host.NAMES, host.STATE):
            _check(case, 'grad.' + s, g0[k], 'null_d_norm')
    finally:
        h.close()


def test_flags_0_recomputes_the_bits_of_from_fwd(lib):
    """flags 0 recomputes XB and the pair cells from the parameters it is given: after the forward pass of OTHER parameters rewrote
    the workspace (and the right forward pass restored the activations) the gradients are those of FROM_FWD, bit for bit."""
    case = E.case(SMALL)
    g, rel, d_norm = _graphs(case)
    enc = _module(case)
    other = _module(case, {k: v * 0.75 + 0.01 for k, v in case.params.items()})
    up = case.upstream.to(DEV)
    h = _handle(lib, case, g)
    try:
        assert h.status == 0
        right, wrong = _state(enc, 1), _state(other, 1)
        z_ref, g_ref = _c_step(h, right, 1, d_norm, up)
        _check(case, 'z', z_ref, 'from_fwd')
        for first in (wrong, right):
            z = torch.empty_like(z_ref)
            assert h.forward(h.params(first, 1), d_norm, z) == 0
            assert h.forward(h.params(right, 1), d_norm, z) == 0
            grads = {k: torch.empty_strided(v.shape, v.stride(), device=DEV).fill_(float('nan')) for k, v in right.items()}
            assert h.backward(h.params(right, 1), d_norm, up, grads, 0) == 0
            torch.cuda.synchronize()
            assert torch.equal(z, z_ref)
            for k in host.NAMES:
                assert torch.equal(grads[k], g_ref[k]), k
    finally:
        h.close()


def test_build_refuses_a_graph_without_relations_or_edges(lib):
    case = E.case(SMALL)
    g, _, _ = _graphs(case)
    pp, dp, dd, rg = (g[k].contiguous() for k in ('pp_train_indices', 'dp_edge_index', 'dd_train_idx', 'dd_train_range'))
    dims = _dims(case)
    empty = torch.zeros_like(rg)
    for dd_ptr, n_dd, rg_ptr, n_rel in ((dd.data_ptr(), 0, empty.data_ptr(), case.R), (None, 0, None, 0), (None, 0, empty.data_ptr(), case.R)):
        h = host.P()
        st = lib.tipk_encoder_build(pp.data_ptr(), pp.shape[1], dp.data_ptr(), dp.shape[1], dd_ptr, n_dd, rg_ptr, n_rel, 8, case.n_prot,
                                    case.n_drug, C.byref(dims), C.byref(h))
        assert st == host.TIPK_EUNSUPPORTED and not h.value, (n_dd, n_rel, st)
