"""`tipk_pd_stage_bwd_riders` (include/tipk.h section 3) on the host: what it refuses, it refuses before anything is launched, so
these calls need no device -- every pointer below is host memory that no kernel ever sees.  The entry is purely additive: the
ABI version stays where it was."""
import ctypes as C

import numpy as np
import pytest

from tip_amd import _lib

TIPK_EINVAL, TIPK_EUNSUPPORTED = -1, -2
_BUF = np.zeros(64, dtype=np.float32)
_IDX = np.zeros(64, dtype=np.int32)
F, I = _BUF.ctypes.data, _IDX.ctypes.data


def _stage_args(g=F, p=16, q=16, rows=5, ne=16, n_src=3, n_row_wg=1):
    """The arguments `tipk_pd_stage_bwd` takes (without the stream), valid as far as the host checks go."""
    return [g, 32, F, F, F, p, q, rows, ne, 1, F, 16, F, I, I, F, n_src, I, n_row_wg, F, 32, 32, F, 1, 16, None, F, 32, F, F]


def _desc(**kw):
    d = _lib.SlabSumDesc()
    d.in_, d.n_slabs, d.slab_stride, d.count, d.alpha, d.out = F, 3, 8, 8, 1.0, F
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _riders(descs, n_sums=None, stage=None):
    arr = (_lib.SlabSumDesc * max(1, len(descs)))(*descs)
    n = len(descs) if n_sums is None else n_sums
    return _lib.lib().tipk_pd_stage_bwd_riders(*(stage or _stage_args()), arr if descs else None, n, None)


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 30 and _lib.lib().tipk_abi_version() == 30
    assert 'tipk_pd_stage_bwd_riders' in _lib.SIGNATURES
    old, new = _lib.SIGNATURES['tipk_pd_stage_bwd'], _lib.SIGNATURES['tipk_pd_stage_bwd_riders']
    assert new[0] is old[0] and new[1][:-3] == old[1][:-1] and new[1][-1] is old[1][-1]       # the same arguments + (sums, n_sums)
    assert new[1][-3:-1] == [C.POINTER(_lib.SlabSumDesc), C.c_int32]


@pytest.mark.parametrize('n_sums', (-1, 4, 1000))
def test_rider_count_outside_0_to_3(n_sums):
    assert _riders([_desc()] * 3, n_sums=n_sums) == TIPK_EINVAL


@pytest.mark.parametrize('n_sums', (1, 2, 3))
def test_null_riders(n_sums):
    assert _riders([], n_sums=n_sums) == TIPK_EINVAL


BAD = [('negative_n_slabs', dict(n_slabs=-1)), ('negative_count', dict(count=-1)), ('row_scale_without_cols', dict(row_scale=F, cols=0)),
       ('no_output', dict(out=None)), ('slabs_without_input', dict(in_=None))]


@pytest.mark.parametrize('where', (0, 1, 2))
@pytest.mark.parametrize('name,kw', BAD, ids=[b[0] for b in BAD])
def test_bad_descriptor(name, kw, where):
    """A descriptor `tipk_sum_slabs_group` refuses, in every position, next to good ones."""
    descs = [_desc(), _desc(), _desc()]
    descs[where] = _desc(**kw)
    assert _riders(descs) == TIPK_EINVAL
    arr = (_lib.SlabSumDesc * 3)(*descs)
    assert _lib.lib().tipk_sum_slabs_group(arr, 3, None) == TIPK_EINVAL


def test_the_stage_checks_still_answer_with_riders():
    """Good riders do not hide what the stage itself refuses (the statuses of `tipk_pd_stage_bwd`), with and without riders."""
    L = _lib.lib()
    for stage, want in ((_stage_args(g=None), TIPK_EINVAL), (_stage_args(rows=-1), TIPK_EINVAL), (_stage_args(n_src=0), TIPK_EINVAL),
                        (_stage_args(n_row_wg=0), TIPK_EINVAL), (_stage_args(p=3), TIPK_EUNSUPPORTED),
                        (_stage_args(rows=0), TIPK_EUNSUPPORTED)):
        assert L.tipk_pd_stage_bwd(*stage, None) == want
        assert _riders([], stage=stage) == want
        assert _riders([_desc(), _desc(count=0)], stage=stage) == want
