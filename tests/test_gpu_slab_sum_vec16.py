"""The 16-byte form of the 16-lane ordered slab sum (`slab_sum_body`, tip_amd/csrc/tipk_slabs.h) against its dword form, bit for
bit, and against fp64 within the bound of the slab-sum tests of `tests/dense_cases.py`: per element |kernel - fp64| <= kr * 2^-24
* Abs with kr = n_slabs + 4 (`slab_reference`).

Which form runs is not observable from outside; the host rule (`fill_slab_args`) takes the 16-byte form when `count` and
`slab_stride` are multiples of 4 and `in`, `out`, `addend`, `gate` are 16-byte aligned (`cols % 4 == 0` with a row_scale).  So
every case is built twice from the same values: once with every operand aligned, once with the slabs at a base pointer shifted
by ONE float, which must go down the dword path.  Where the rule refuses the 16-byte form anyway (count 258, a slab stride that
is no multiple of 4, cols = 6) both run the dword form and must still agree.  The sums run through `tipk_sum_slabs_group` and as
riders of `tipk_gemm_wg_group`; NaN guards around the slabs, sentinels around the output, every launch made twice."""
import pytest
import torch

import dense_cases as D
from tip_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 8                                                    # guard floats in front of a view (32 bytes: the view stays aligned)

# the lane rule's lower edge (16 lanes from 32 slabs), one short of the 4 x 16 unroll, on it, one over
N_SLABS = (32, 33, 47, 63, 64, 65)
# one workgroup of 256 elements, one quad over, 16 workgroups, one quad over; 258: not a multiple of 4
COUNTS = (256, 260, 4096, 4100, 258)
STRIDES = ('equal', 'larger', 'not_4')                     # slab_stride = count, count + 8, count + 5 (+ 3 at count 258: 261)
EPILOGUES = [('none', dict()), ('alpha', dict(alpha=-0.5)), ('row_scale4', dict(cols=4)), ('row_scale6', dict(cols=6)),
             ('addend', dict(addend=True)), ('accumulate', dict(accumulate=True)), ('relu', dict(relu=True)), ('gate', dict(gate=True)),
             ('all', dict(alpha=1.5, cols=4, addend=True, accumulate=True, relu=True, gate=True))]


def _values(n_slabs, count, epi, cid):
    g = D._gen(cid)
    v = dict(slabs=torch.randn(n_slabs, count, generator=g), row_scale=None, addend=None, prev=None, gate=None)
    if epi.get('cols'):
        v['row_scale'] = torch.rand(-(-count // epi['cols']), generator=g) + 0.5
    if epi.get('addend'):
        v['addend'] = torch.randn(count, generator=g)
    if epi.get('accumulate'):
        v['prev'] = torch.randn(count, generator=g)
    if epi.get('gate'):
        v['gate'] = D.gate_values([count], g)                # NaN, -0, +0, negative, -inf: closed
    return v


def _reference(v, epi):
    """(fp64 result, Abs, kr) of out = gate?(relu?(alpha * row_scale[i / cols] * sum_s slabs[s][i] + addend + prev))."""
    count = v['slabs'].shape[1]
    out = []
    for f, alpha in D._BOTH(epi.get('alpha', 1.0)):
        s = f(v['slabs']).sum(0) * alpha
        if v['row_scale'] is not None:
            s = s * f(v['row_scale'])[torch.arange(count) // epi['cols']]
        if v['addend'] is not None:
            s = s + f(v['addend'])
        if v['prev'] is not None:
            s = s + f(v['prev'])
        out.append(s)
    want = torch.relu(out[0]) if epi.get('relu') else out[0]
    if v['gate'] is not None:
        open_ = v['gate'] > 0
        want, out[1] = want * open_, out[1] * open_
    return want, out[1], v['slabs'].shape[0] + 4


class _Sum(object):
    """One slab sum on the device.  shift: the slabs start one float past a 16-byte boundary."""

    def __init__(self, v, epi, stride_kind, shift):
        self.v, self.epi = v, epi
        n, count = v['slabs'].shape
        self.n, self.count = n, count
        self.stride = count if stride_kind == 'equal' else count + 8 if stride_kind == 'larger' else count + (5 if count % 4 == 0 else 3)
        off = PAD + (1 if shift else 0)
        host = torch.full((off + n * self.stride + PAD,), D.NAN)
        host[off:off + n * self.stride].view(n, self.stride)[:, :count] = v['slabs']
        self.host_in, self.big_in = host, host.to(DEV)
        self.slabs = self.big_in[off:]
        self.keep = {k: v[k].to(DEV) for k in ('row_scale', 'addend', 'gate') if v[k] is not None}
        self.big_out = torch.full((count + 2 * PAD,), D.SENT, device=DEV)
        self.out = self.big_out[PAD:PAD + count]
        if v['prev'] is not None:
            self.out.copy_(v['prev'])
        for t in [self.out] + list(self.keep.values()):
            assert t.data_ptr() % 16 == 0
        assert self.slabs.data_ptr() % 16 == (4 if shift else 0)

    def desc(self):
        e, d, k = self.epi, _lib.SlabSumDesc(), self.keep
        d.in_, d.n_slabs, d.slab_stride, d.count = self.slabs.data_ptr(), self.n, self.stride, self.count
        d.alpha, d.accumulate = e.get('alpha', 1.0), int(bool(e.get('accumulate')))
        d.row_scale, d.cols = (k['row_scale'].data_ptr() if 'row_scale' in k else None), e.get('cols', 0)
        d.addend = k['addend'].data_ptr() if 'addend' in k else None
        d.relu, d.out = int(bool(e.get('relu'))), self.out.data_ptr()
        d.gate = k['gate'].data_ptr() if 'gate' in k else None
        return d

    def check(self, name, ref):
        big = self.big_out.cpu()
        assert bool((big[:PAD] == D.SENT).all()) and bool((big[PAD + self.count:] == D.SENT).all()), name + ': a write outside the output'
        assert torch.equal(self.big_in.cpu().nan_to_num(7.0), self.host_in.nan_to_num(7.0)), name + ': the slabs changed'
        want, mag, kr = ref
        r = D.ratio(self.out, want, mag)
        print('RATIO %s %.3f (kr = %d, used = %.4f)' % (name, r, kr, r / kr))
        assert r / kr <= 1.0, (name, r, kr)
        if self.v['gate'] is not None:
            assert bool((self.out.cpu()[~(self.v['gate'] > 0)] == 0).all()), name + ': NaN, -0 and negative gates are closed'


def _group(items):
    arr = (_lib.SlabSumDesc * len(items))(*[s.desc() for s in items])
    _lib.check(_lib.lib().tipk_sum_slabs_group(arr, len(items), _lib.stream_ptr(items[0].out.device)), 'tipk_sum_slabs_group')


def _riders(items):
    arr = (_lib.SlabSumDesc * len(items))(*[s.desc() for s in items])
    _lib.check(_lib.lib().tipk_gemm_wg_group(None, 0, arr, len(items), _lib.stream_ptr(items[0].out.device)), 'tipk_gemm_wg_group')


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('n_slabs', N_SLABS)
def test_vec16_equals_dword_and_fp64(n_slabs, count):
    for ename, epi in EPILOGUES:
        v = _values(n_slabs, count, epi, 'vec16_%d_%d_%s' % (n_slabs, count, ename))
        ref = _reference(v, epi)
        for kind in STRIDES:
            name = 'vec16_%dx%d_%s_%s' % (n_slabs, count, kind, ename)
            outs = []
            for launch in (_group, _riders):
                first, again = [[_Sum(v, epi, kind, shift) for shift in (False, True)] for _ in range(2)]
                launch(first)
                launch(again)
                torch.cuda.synchronize()
                for s, tag in zip(first, ('aligned', 'shifted')):
                    s.check('%s[%s,%s]' % (name, launch.__name__[1:], tag), ref)
                assert torch.equal(first[0].out, first[1].out), name + ': 16-byte and dword form differ'
                assert torch.equal(first[0].out, again[0].out) and torch.equal(first[1].out, again[1].out), name + ': not repeatable'
                outs.append(first[0].out)
            assert torch.equal(outs[0], outs[1]), name + ': a rider and a grouped sum differ'


def test_vec16_equals_the_single_launch():
    """The 63 x 35 136 shape of BioSNAP's d att slabs, cut to 8 workgroups and a quad: the bits of tipk_sum_slabs_ex."""
    n_slabs, count = 63, 2052
    epi = dict(alpha=0.5, cols=4, addend=True, relu=True)
    v = _values(n_slabs, count, epi, 'vec16_single')
    vec, one = _Sum(v, epi, 'equal', False), _Sum(v, epi, 'equal', False)
    _group([vec])
    k = one.keep
    _lib.check(_lib.lib().tipk_sum_slabs_ex(_lib.ptr(one.slabs), n_slabs, one.stride, count, 0.5, 0, _lib.ptr(k['row_scale']), 4,
                                            _lib.ptr(k['addend']), 1, _lib.ptr(one.out), _lib.stream_ptr(one.out.device)), 'tipk_sum_slabs_ex')
    torch.cuda.synchronize()
    vec.check('vec16_single', _reference(v, epi))
    assert torch.equal(vec.out, one.out)
