"""CPU tests of the case table of the exact screen tests (tests/screen_cases.py): for every case the kernel's fp32 arithmetic
equals fp64 exactly, so tests/test_gpu_screen_edges.py may compare with `torch.equal`, and every case reaches the edge it is
named after -- ties that straddle the cut, the split counts and merge levels, parts without a drug block, the buffer filled
to CAP and cut at CAP - ROUND + 1, both filter routes, keys next to 2^31, NaN and infinite logits.  The kernel's deal, round
structure and workspace layout are restated here and held to `tipk_distmult_screen_workspace_bytes`; the vectorised
reference `exact_screen` is held to the Python-loop spec `spec_screen` on the small cases."""
import pytest
import torch

import screen_cases as cases
from screen_rank_spec import emulated_fp32_logits, on_exact_grid
from screen_spec import exact_screen, known_mask, spec_screen
from tip_amd import _lib

INF = float('inf')


def _relations(c):
    """{relation: None (a relation query asks for it: the whole matrix) or the sorted drugs of its drug queries}"""
    out = {}
    for r, du in c.queries:
        if du < 0:
            out[r] = None
        elif out.get(r, []) is not None:
            out[r] = sorted(set(out.get(r, []) + [du]))
    return out


@pytest.mark.parametrize('cid', [c for c in cases.ids() if not c.endswith('-search')])
def test_fp32_logits_equal_fp64(cid):
    """x_k = fl32(z[u,k] * w[r,k]), acc = fl32(x_k * z[v,k] + acc), k ascending, against the fp64 product: equal, so the
    reference needs no tolerance.  Case i (NaN, 3e38) is compared after rounding fp64 to fp32."""
    c = cases.case(cid)
    if cid[0] in 'abcdfgh':
        assert on_exact_grid(c.z, c.w), 'the grid that is exact up to dim 256'
    z64, w64 = c.z.double(), c.w.double()
    for r, drugs in _relations(c).items():
        rows = None if drugs is None else torch.tensor(drugs)
        emu = emulated_fp32_logits(c.z, c.w, r, rows)
        ref = ((z64 if rows is None else z64[rows]) * w64[r]) @ z64.t()
        if cid == 'i':
            assert torch.equal(emu.isnan(), ref.isnan()) and torch.equal(emu.nan_to_num(nan=0.0), ref.float().nan_to_num(nan=0.0))
            assert bool(emu.isinf().any()) and bool(emu.isnan().any())
        else:
            assert torch.equal(emu.double(), ref), (cid, r)


# ------------------------------------------------------------------ exact_screen against the Python-loop spec
@pytest.mark.parametrize('cid', [c for c in cases.ids('a') + cases.ids('d') if cases.case(c).z.shape[0] <= 65])
def test_exact_screen_equals_spec(cid):
    c = cases.case(cid)
    s, u, v = exact_screen(c.z, c.w, c.queries, c.k, c.known)
    ws, wu, wv = spec_screen(c.z, c.w, c.queries, c.k, c.known)
    assert s.dtype == torch.float32 and u.dtype == torch.int32 and v.dtype == torch.int32
    assert torch.equal(s.double(), ws) and torch.equal(u.long(), wu) and torch.equal(v.long(), wv)


# ------------------------------------------------------------------ the kernel's structure, restated
def workspace_bytes(n, n_q, k):
    """screen_layout: the query list, the part lists (score, key) and, above 8 parts, the lists of the first merge level"""
    def align(b):
        return (b + 255) & ~255
    s = cases.splits(n, n_q)
    s2 = (s + cases.MERGE_G - 1) // cases.MERGE_G if s > cases.MERGE_G else 0
    return align(n_q * 8) + 2 * align(n_q * s * k * 4) + 2 * align(n_q * s2 * k * 4)


def part_tiles(n, part, s):
    """WgDeal: the tiles (bu, bv), bu <= bv, row-major, of part `part` of `s`"""
    nb = (n + cases.TILE - 1) // cases.TILE
    every = [(bu, bv) for bu in range(nb) for bv in range(bu, nb)]
    return every[len(every) * part // s:len(every) * (part + 1) // s]


def part_blocks(n, part, s):
    """the blocks of 256 partners of a drug query that part `part` of `s` owns"""
    nvb = (n + cases.DBLK - 1) // cases.DBLK
    return range(nvb * part // s, nvb * (part + 1) // s)


def emulate_rounds(c, qi, part, s):
    """WgSel over the rounds of one part of relation query qi: a round is the rows u % 4 == i of a tile; a candidate is
    appended when it is not below the threshold and not listed; the buffer is cut to the k best when c > CAP - ROUND.
    -> [(c after the round's appends, appends of the round)]"""
    n, k = c.z.shape[0], c.k
    r = c.queries[qi][0]
    L = emulated_fp32_logits(c.z, c.w, r)
    km = known_mask(c.known[0], c.known[1], r, n, 'cpu') if c.known is not None else torch.zeros(n, n, dtype=torch.bool)
    keep_s, keep_key, thr, log = torch.empty(0), torch.empty(0, dtype=torch.int64), -INF, []
    for bu, bv in part_tiles(n, part, s):
        for i in range(4):
            uu, vv = torch.meshgrid(bu * 64 + 4 * torch.arange(16) + i, bv * 64 + torch.arange(64), indexing='ij')
            ok = (uu < vv) & (vv < n)
            uu, vv = uu[ok], vv[ok]
            sc = L[uu, vv]
            p = (sc >= thr) & ~km[uu, vv]
            keep_s, keep_key = torch.cat([keep_s, sc[p]]), torch.cat([keep_key, (uu * n + vv)[p]])
            log.append((keep_s.numel(), int(p.sum())))
            if keep_s.numel() > cases.CAP - cases.ROUND:
                by_key = torch.argsort(keep_key)
                order = by_key[torch.sort(keep_s[by_key], descending=True, stable=True).indices][:k]
                keep_s, keep_key = keep_s[order], keep_key[order]
                thr = float(keep_s[k - 1]) if keep_s.numel() == k else -INF
    return log


def test_restated_layout_is_the_library_s():
    L = _lib.lib()
    for n in (1, 64, 65, 129, 200, 255, 513, 700, 724, 46340):
        for n_q in (0, 1, 2, 8, 63, 64, 65, 455, 456, 511, 512, 513, 2048, 2049, 4096, 4097):
            for k in (1, 8, 37, 300, 1024):
                assert L.tipk_distmult_screen_workspace_bytes(n, 16, n_q, k) == workspace_bytes(n, n_q, k), (n, n_q, k)


def _straddles(c):
    """the queries whose slot k (1-based) and slot k + 1 hold the same logit: a tie runs through the cut"""
    s, u, _ = exact_screen(c.z, c.w, c.queries, c.k + 1, c.known)
    return [i for i in range(len(c.queries)) if int(u[i, c.k]) >= 0 and float(s[i, c.k - 1]) == float(s[i, c.k])]


@pytest.mark.parametrize('cid', cases.ids('d') + cases.ids('e') + cases.ids('f'))
def test_ties_straddle_the_cut(cid):
    assert _straddles(cases.case(cid)), 'no query of %s has equal logits on both sides of slot k' % cid


# ------------------------------------------------------------------ a
@pytest.mark.parametrize('cid', cases.ids('a'))
def test_a_candidate_counts_on_both_sides_of_k(cid):
    c = cases.case(cid)
    n = c.z.shape[0]
    _, u, _ = exact_screen(c.z, c.w, c.queries, n * n + 1, c.known)
    counts = (u >= 0).sum(1).tolist()
    assert counts[2] == n * (n - 1) // 2 and counts[3] == 0                  # relation 2: no list; relation 3: every pair
    if n <= 2:
        assert max(counts) <= 1                                              # k = 1 is met at most; all else is padding
    else:
        assert min(counts) < c.k < max(counts)
    if n > 7:
        assert c.queries[-1] == (4, n - 1) and (4, 7) in c.queries and counts[c.queries.index((4, 7))] == 0


# ------------------------------------------------------------------ c
@pytest.mark.parametrize('cid', cases.ids('c'))
def test_c_parts_without_a_block(cid):
    c = cases.case(cid)
    n = c.z.shape[0]
    s = cases.splits(n, len(c.queries))
    owned = [len(part_blocks(n, p, s)) for p in range(s)]
    assert sum(owned) == (n + 255) // 256 and owned.count(0) >= 1 and max(owned) == 1
    assert all(du >= 0 for _, du in c.queries) and len(c.queries) in (1, 8)
    if cid.endswith('-0'):                                                   # every partner of drug 0 is listed
        assert int((exact_screen(c.z, c.w, c.queries, c.k, c.known)[1] >= 0).sum()) == 0


def test_c_covers_the_block_edges():
    alone = {(cases.case(c).z.shape[0], cases.case(c).queries[0][1]) for c in cases.ids('c') if not c.endswith('eight')}
    for n in cases.C_N:
        for du in (0, 255, 256, n - 1):
            assert du >= n or (n, du) in alone


# ------------------------------------------------------------------ d
@pytest.mark.parametrize('cid', [c for c in cases.ids('d') if c.endswith('zero')])
def test_d_all_zero_answers_in_closed_form(cid):
    c = cases.case(cid)
    n, k = c.z.shape[0], c.k
    s, u, v = exact_screen(c.z, c.w, c.queries, k, c.known)
    for i, (r, du) in enumerate(c.queries):
        km = known_mask(c.known[0], c.known[1], r, n, 'cpu')
        pairs = [(a, b) for a in (range(n) if du < 0 else [du]) for b in (range(a + 1, n) if du < 0 else range(n))
                 if a != b and not km[a, b]][:k]                              # ascending key
        assert u[i, :len(pairs)].tolist() == [p[0] for p in pairs] and v[i, :len(pairs)].tolist() == [p[1] for p in pairs]
        assert bool((s[i, :len(pairs)] == 0).all()) and bool((u[i, len(pairs):] == -1).all())


# ------------------------------------------------------------------ e
def test_e_buffer_reaches_cap_and_the_cut_bound():
    c = cases.case('e-1024')
    n = cases.E_N
    assert cases.splits(n, len(c.queries)) == 6 and part_tiles(n, 1, 6) == [(0, 1)]
    log = emulate_rounds(c, 4, 1, 6)                                         # the all-zero relation on the full tile (0, 1)
    assert [x[0] for x in log] == [cases.CAP - cases.ROUND] + [cases.CAP] * 3 and all(x[1] == cases.ROUND for x in log)
    for qi in range(4):                                                      # rising and falling logits: cut mid-tile, and
        log = emulate_rounds(c, qi, 1, 6)                                    # the threshold then turns candidates away
        assert max(x[0] for x in log) > cases.CAP - cases.ROUND and min(x[1] for x in log) < cases.ROUND

    c = cases.case('e-walk')
    assert cases.splits(n, len(c.queries)) == 1 and len(part_tiles(n, 0, 1)) == 6
    for qi in range(5):
        log = emulate_rounds(c, qi, 0, 1)
        top = max(x[0] for x in log)
        assert len(log) == 24 and top > cases.CAP - cases.ROUND and (qi != 4 or top == cases.CAP)

    c = cases.case('e-edge')
    assert cases.splits(n, 1) == 6
    log = emulate_rounds(c, 0, 1, 6)
    assert log == [(1024, 1024), (1025, 1), (2048, 1024), (1024, 0)]         # cut at CAP - ROUND + 1, then a full round


# ------------------------------------------------------------------ f
@pytest.mark.parametrize('cid', cases.ids('f'))
def test_f_split_counts_and_merge_levels(cid):
    c = cases.case(cid)
    n, n_q, k, s = cases.F_CASES[cid]
    assert (c.z.shape[0], len(c.queries), c.k) == (n, n_q, k) and cases.splits(n, n_q) == s
    assert all(du < 0 for _, du in c.queries)
    groups = [min(8, s - g) for g in range(0, s, 8)]
    assert groups == {10: [8, 2], 9: [8, 1], 8: [8], 1: [1], 64: [8] * 8}[s]
    assert _lib.lib().tipk_distmult_screen_workspace_bytes(n, 4, n_q, k) == workspace_bytes(n, n_q, k)
    if s > 1:                                                                # the ties cross part boundaries
        want = exact_screen(c.z, c.w, c.queries[:1], k, c.known)
        key = want[1][0].long() * n + want[2][0].long()
        tile_of = {t: p for p in range(s) for t in part_tiles(n, p, s)}
        cut = float(want[0][0, k - 1])
        parts = {tile_of[(int(a) // 64, int(b) // 64)] for a, b, x in zip(key // n, key % n, want[0][0]) if float(x) == cut}
        assert len(parts) > 1, 'the logit at the cut comes from one part only'


# ------------------------------------------------------------------ g
def test_g_routes_and_list():
    L = _lib.lib()
    assert L.tipk_distmult_screen_bitmap_route(724) == 1 and L.tipk_distmult_screen_bitmap_route(725) == 0
    for n in (724, 725):
        c = cases.case('g-%d' % n)
        keys, ptr = c.known
        ptr = ptr.tolist()
        r0 = set(keys[ptr[0]:ptr[1]].tolist())
        assert 1 * n + 0 in r0 and 0 * n + 1 not in r0                       # reversed orientation only
        assert (n - 1) * n + n - 2 in r0 and (n - 2) * n + n - 1 not in r0
        assert 5 * n + 5 in r0                                               # a self key
        assert ptr[1] == ptr[2] and ptr[1] - ptr[0] > 1000 and ptr[3] - ptr[2] > 1000    # an empty block between two full ones
        _, u, v = exact_screen(c.z, c.w, c.queries, c.k, c.known)
        assert 1 not in v[c.queries.index((0, 0))].tolist() and n - 2 not in v[c.queries.index((0, n - 1))].tolist()
    a, b = cases.case('g-724-search'), cases.case('g-724')
    assert torch.equal(a.z, b.z) and torch.equal(a.known[0], b.known[0]) and a.queries == b.queries


# ------------------------------------------------------------------ h
def test_h_keys_next_to_the_int32_limit():
    c = cases.case('h')
    n = cases.H_N
    assert n * n - 1 < 2 ** 31 <= (n + 1) ** 2 and c.z.shape[0] == n and all(du >= 0 for _, du in c.queries)
    assert _lib.lib().tipk_distmult_screen_supported(n, 4, c.k) == 1 and _lib.lib().tipk_distmult_screen_bitmap_route(n) == 0
    s, u, v = exact_screen(c.z, c.w, c.queries, c.k, c.known)
    top = v[0][s[0] == s[0, 0]].tolist()
    assert len(top) < c.k and n - 2 in top and int(u[0, 0]) == n - 1         # key n^2 - 2 is among the best of the first query
    assert n - 1 in v[1][s[1] == s[1, 0]].tolist()
    assert n - 3 not in v[0].tolist() and 3 not in v[0].tolist() and 1 not in v[1].tolist() and n - 2 not in v[1].tolist()
    assert float(s[0, c.k - 1]) > 0 and int(u[1, c.k - 1]) == 0


# ------------------------------------------------------------------ i
def test_i_nan_and_infinities_in_the_reference():
    c = cases.case('i')
    s, u, v = exact_screen(c.z, c.w, c.queries, c.k, c.known)
    assert not bool(s.isnan().any())
    assert not bool((u == cases.I_NAN).any()) and not bool((v == cases.I_NAN).any())       # NaN candidates never appear
    for qi in (0, 2):                                                        # relation 0: the list leaves fewer than k candidates
        nv = int((u[qi] >= 0).sum())
        pos, neg = int((s[qi] == INF).sum()), int((s[qi, :nv] == -INF).sum())
        assert 0 < pos and 0 < neg and nv < c.k
        assert bool((s[qi, :pos] == INF).all()) and bool((s[qi, nv - neg:nv] == -INF).all())
        assert bool((v[qi, nv - neg:nv] >= 0).all()) and bool((u[qi, nv:] == -1).all())    # -inf entries, then the padding
        key = u[qi, :pos].long() * cases.I_N + v[qi, :pos].long()
        assert bool((key[1:] > key[:-1]).all())                              # +inf entries by ascending key
    assert c.queries[4] == (0, cases.I_NAN) and bool((u[4] == -1).all())     # every partner of the NaN drug is NaN
    assert int((u[1] >= 0).sum()) == c.k and float(s[1, 0]) == INF
