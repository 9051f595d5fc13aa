"""-m gpu: `tipk_distmult_screen` (include/tipk.h section 4c) held to the EXACT order at its edges.  The inputs come from
tests/screen_cases.py: tests/test_host_screen_cases.py shows for each that fp32 and fp64 logits agree exactly and that ties
straddle the cut, so the result is compared with `exact_screen` on the device by `torch.equal` -- score bits, u and v, no
tolerance.  A wrong tie order, a candidate that equals the threshold and is dropped, a merge that mis-ranks equal logits
across parts and a buffer cut one entry late all show here.  Groups f and g also tie the screen to the screen rank (rank j + 1
at slot j, the same logit bits); groups a, c and i run twice and must repeat bit for bit.  Each case launches the screen once
or twice."""
import functools

import pytest
import torch

import screen_cases as cases
from screen_spec import assert_screen_exact, exact_screen
from tip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _on_device(cid):
    """(z, w, known) on the device and the exact answer, computed once per input (g-724-search shares g-724's)"""
    return _on_device_once(cid[:-len('-search')] if cid.endswith('-search') else cid)


@functools.lru_cache(maxsize=None)
def _on_device_once(cid):
    c = cases.case(cid)
    z, w = c.z.to(DEV), c.w.to(DEV)
    known = None if c.known is None else (c.known[0].to(DEV), c.known[1].to(DEV))
    return z, w, known, exact_screen(z, w, c.queries, c.k, known)


def _screen(cid):
    c = cases.case(cid)
    z, w, known, _ = _on_device(cid)
    got = ops.distmult_screen(z, w, torch.tensor(c.queries), c.k, known=known)
    assert got[0].shape == (len(c.queries), c.k)
    return got


def _check(cid, repeat=False):
    got = _screen(cid)
    assert_screen_exact(got, _on_device(cid)[3])
    if repeat:
        for x, y, name in zip(got, _screen(cid), ('score', 'u', 'v')):
            assert torch.equal(x, y), 'run to run: ' + name
    return got


def _check_rank(cid, got):
    """The relation queries' returned pairs under the screen rank: rank j + 1 at slot j and the screen's logit bits."""
    c = cases.case(cid)
    z, w, known, _ = _on_device(cid)
    s, u, v = got
    rel = torch.tensor([du < 0 for _, du in c.queries], device=DEV)
    q_rel = torch.tensor([r for r, _ in c.queries], dtype=torch.int32, device=DEV)[rel]
    s, u, v = s[rel], u[rel], v[rel]
    ok = u >= 0
    ptr = torch.zeros(ok.shape[0] + 1, dtype=torch.int64, device=DEV)
    ptr[1:] = torch.cumsum(ok.sum(1), 0)
    slot = torch.arange(c.k, device=DEV).expand_as(u)[ok]
    assert slot.numel() > 0
    rank, logit = ops.distmult_screen_rank(z, w, q_rel, ptr, u[ok], v[ok], known)
    assert torch.equal(rank.long(), slot + 1), 'rank - 1 is the position in the screen'
    assert torch.equal(logit.view(torch.int32), s[ok].view(torch.int32)), 'the two kernels give one logit per pair'


@pytest.mark.parametrize('cid', cases.ids('a'))
def test_a_tile_and_size_edges(cid):
    _, u, _ = _check(cid, repeat=True)
    if cases.case(cid).z.shape[0] == 1:
        assert bool((u == -1).all())                                         # no candidate at all: everything is padding


@pytest.mark.parametrize('cid', cases.ids('b'))
def test_b_width_edges(cid):
    _check(cid)


@pytest.mark.parametrize('cid', cases.ids('c'))
def test_c_drug_block_edges(cid):
    _check(cid, repeat=True)


@pytest.mark.parametrize('cid', cases.ids('d'))
def test_d_ties_straddle_the_cut(cid):
    _check(cid)


@pytest.mark.parametrize('cid', cases.ids('e'))
def test_e_buffer_pressure(cid):
    _check(cid)


@pytest.mark.parametrize('cid', cases.ids('f'))
def test_f_split_and_merge_levels(cid):
    _check_rank(cid, _check(cid))


@pytest.mark.parametrize('cid', cases.ids('g'))
def test_g_filter_routes(cid):
    n = cases.case(cid).z.shape[0]
    route = _lib.lib().tipk_distmult_screen_bitmap_route
    if not cid.endswith('-search'):
        assert route(n) == (1 if n <= 724 else 0)
        _check_rank(cid, _check(cid))
        return
    bitmap = _screen(cid)
    _lib.set_option('screen_search', 1)
    try:
        assert route(n) == 0
        got = _check(cid)
        _check_rank(cid, got)
    finally:
        _lib.set_option('screen_search', 0)
    assert route(n) == 1
    for x, y, name in zip(got, bitmap, ('score', 'u', 'v')):
        assert torch.equal(x, y), 'bitmap vs search route: ' + name


def test_h_top_of_the_key_range():
    s, u, v = _check('h')
    n = cases.H_N
    assert int((u[0].long() * n + v[0].long()).max()) == n * n - 2           # the key next to the last one was returned


def test_i_nan_and_infinities():
    s, u, v = _check('i', repeat=True)
    assert not bool((u == cases.I_NAN).any()) and not bool((v == cases.I_NAN).any())
    low = s[0].isneginf() & (u[0] >= 0)
    assert int(low.sum()) > 0 and bool((v[0][low] >= 0).all()) and bool((u[0] == -1).any())    # -inf entries, then padding
