"""`tipk_pd_stage_bwd_riders` (tip_amd/csrc/tipk_drugmix.hip) against `tipk_pd_stage_bwd` followed by `tipk_sum_slabs_group` on
the same inputs: every output of the stage and every rider's sum must be bitwise equal, with 0 ... 3 riders behind the stage's
workgroups -- a rider of one workgroup, riders of several (the 16-byte forms of the 4-lane and of the 16-lane sum), and one
with count == 0, which is skipped.  What the stage computes is pinned against fp64 elsewhere (tests/test_gpu_kernels.py
`test_pd_stage_bwd`, tests/test_gpu_protein_routes.py); here only "the riders change nothing, and nothing changes the riders".

5 and 70 drugs, 3 and 130 kept source rows: `protein_cases.protein_graph` starts at 40 drugs and 300 proteins, so the P -> D
graph is drawn directly, as `test_pd_stage_bwd` does; `protein_cases.pd_limits` says how many rows a row workgroup takes (130
rows are more than one)."""
import pytest
import torch

import protein_cases as P
from tip_amd import _lib, ops
from tip_amd.layers import hier_graph

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -1234.5
p_, q_, ne_, c1_ = 16, 16, 48, 32


class _Stage(object):
    def __init__(self, n, n_src):
        g = torch.Generator().manual_seed(1000 * n + n_src)
        E = 6 * n + n_src
        src = torch.cat([torch.randint(0, n_src, (6 * n,), generator=g), torch.arange(n_src)])      # every kept row has an edge
        dst = torch.randint(0, n, (E,), generator=g)
        self.n, self.n_src = n, n_src
        self.graph = hier_graph(torch.stack([src, dst + n_src]).to(DEV), n_src + n, n_src, table_rows=n_src, d=p_)
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)
        self.g_x0 = r(n, ne_ + q_ + 3)[:, 1:-2]                               # a strided upstream gradient
        self.mean, self.w_h, self.agg = r(n, p_), r(p_, q_), r(n_src, c1_)
        self.d_norm, self.scale = (torch.rand(n, generator=g) + 0.5).to(DEV), (torch.rand(n_src, generator=g) + 0.5).to(DEV)
        self.w2 = r(c1_, p_).t()                                              # [in, out] storage behind the [out, in] shape
        self.n_row_wg = int(self.graph.pd_csr['t_wg'].numel()) - 1

    def run(self, entry, riders=None):
        """-> the five outputs of the stage, written into sentinel-filled buffers."""
        csr, n, n_src, L = self.graph.pd_csr, self.n, self.n_src, _lib.lib()
        full = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)
        outs = [full(n, ne_), full(int(L.tipk_pd_stage_bwd_wh_slabs()), p_, q_), full(n_src, c1_), full(self.n_row_wg, c1_, p_),
                full(self.n_row_wg, p_)]
        g_xd, g_w, gw, dw2, db2 = outs
        ptr = _lib.ptr
        args = [ptr(self.g_x0), self.g_x0.stride(0), ptr(self.d_norm), ptr(self.mean), ptr(self.w_h), p_, q_, n, ne_, 1, ptr(g_xd),
                g_xd.stride(0), ptr(g_w), ptr(csr['t_ptr']), ptr(csr['t_dst']), ptr(csr['t_w']), n_src, ptr(csr['t_wg']), self.n_row_wg,
                ptr(self.agg), self.agg.stride(0), c1_, ptr(self.w2), self.w2.stride(0), self.w2.stride(1), ptr(self.scale), ptr(gw),
                gw.stride(0), ptr(dw2), ptr(db2)]
        if entry == 'riders':
            arr = (_lib.SlabSumDesc * max(1, len(riders)))(*[j.desc for j in riders])
            args += [arr if riders else None, len(riders)]
        _lib.check(getattr(L, 'tipk_pd_stage_bwd' + ('_riders' if entry == 'riders' else ''))(*args, _lib.stream_ptr(self.g_x0.device)), entry)
        return outs


_STAGES = {}


def _stage(n, n_src):
    if (n, n_src) not in _STAGES:
        _STAGES[(n, n_src)] = _Stage(n, n_src)
    return _STAGES[(n, n_src)]


def _rider_values():
    g = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    gate = r(9, 1028)
    gate.view(-1)[::5] = float('nan')
    gate.view(-1)[1::5] = -0.0
    return {'one_wg': dict(slabs=r(5, 10, 4), alpha=0.5, addend=r(10, 4), relu=True),          # 4 lanes, dwords: 1 workgroup
            'lanes16': dict(slabs=r(63, 257, 4), row_scale=torch.rand(257, generator=g).to(DEV) + 0.5),   # 16-byte 16-lane form: 5 workgroups
            'lanes4': dict(slabs=r(9, 9, 1028), gate=gate),                                      # 16-byte 4-lane form: 3 workgroups
            'empty': dict(slabs=torch.empty(3, 0, device=DEV))}


_SETS = {0: (), 1: ('lanes16',), 2: ('one_wg', 'lanes4'), 3: ('lanes16', 'empty', 'one_wg')}
_VALUES = {}


def _jobs(names):
    if not _VALUES:
        _VALUES.update(_rider_values())
    return [ops.slab_job(**_VALUES[k]) for k in names]


@pytest.mark.parametrize('n_riders', sorted(_SETS))
@pytest.mark.parametrize('n_src', (3, 130))
@pytest.mark.parametrize('n', (5, 70))
def test_riders_equal_stage_then_slab_sums(n, n_src, n_riders):
    s = _stage(n, n_src)
    max_rows, _ = P.pd_limits()
    assert (s.n_row_wg > 1) == (n_src > max_rows)
    want = s.run('old')
    apart = _jobs(_SETS[n_riders])
    ops.gemm_group([], apart)                                                 # tipk_sum_slabs_group
    riding, again = _jobs(_SETS[n_riders]), _jobs(_SETS[n_riders])
    got = s.run('riders', riding)
    got2 = s.run('riders', again)
    torch.cuda.synchronize()
    names = ('g_xd', 'g_w slabs', 'gw', 'd W2 slabs', 'd b2 slabs')
    for name, a, b, c in zip(names, want, got, got2):
        assert not bool((a == SENT).any()), name + ': not every element is written'
        assert torch.equal(a, b), name + ': the riders changed the stage'
        assert torch.equal(b, c), name + ': not repeatable'
    for k, a, b, c in zip(_SETS[n_riders], apart, riding, again):
        assert torch.equal(a.out, b.out), k + ': a riding sum differs from tipk_sum_slabs_group'
        assert torch.equal(b.out, c.out), k + ': not repeatable'


@pytest.mark.parametrize('n_src', (3, 130))
@pytest.mark.parametrize('n', (5, 70))
def test_no_riders_is_the_old_entry(n, n_src):
    """n_sums == 0 (a null descriptor array): the launch of `tipk_pd_stage_bwd`, bit for bit."""
    s = _stage(n, n_src)
    want, got = s.run('old'), s.run('riders', [])
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
