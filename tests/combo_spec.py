"""fp64 specification of the combination burden (include/tipk.h section 4n) and the acceptance rule its results are held to.

A `model` is ('distmult', z [n, dim], w [R, dim]) or ('table', s1 [n, R], s2 [n, R]) as in tests/pair_topk_spec.py.  A QUERY
is the pair (fixed, slots): a list of drug ids and a list of slots, each a list of alternatives (a drug id, or -1 for "leave
the slot empty").  `limits` is `ops.combo_limits()`: (max_fixed, max_slots, max_alternatives, max_combinations).

The spec works from the DEFINITION -- it enumerates the combinations (itertools.product order: the last slot runs fastest)
and, per combination, the unordered pairs of its regimen (the fixed drugs plus the chosen ids that are not -1); it knows
nothing of tables, levels or prefixes.
  A query is ILLEGAL -- every entry NaN -- with a fixed id outside [0, n), a repeated fixed drug, an alternative outside
  [-1, n), an empty slot, or a limit exceeded.  It owns prod A_s entries, or ONE entry when its structure is what is illegal
  (an empty slot, too many slots, alternatives or combinations): `combination_count`, the convention of `ops.combo_plan`.
  A combination is NOT APPLICABLE -- NaN, never selected -- when two chosen drugs coincide, a chosen drug is a fixed drug,
  or a triple of its pairs that is not known has a NaN logit.
  Otherwise, over the pairs (min id, max id) of the regimen, a triple CONTRIBUTES unless it is known for the pair's key, and
    noisy_or  A_r = sum of softplus(logit) over the contributing triples, P_r = 1 - exp(-A_r)
    max       P_r = sigma(largest contributing logit)
  P_r = 0 without a contributing triple; B = sum_r weights[r] * P_r.

`check_combo_burden` holds a result to the rule, in the form of tests/addon_spec.py:
  (a) NaN sits exactly where the query is illegal or the combination not applicable;
  (b) every other burden is within T_B = sum_r w_r * T_P,r + (R + C_COMBO) * U * B64 of B64, where, tau being the per-logit
      bound of tests/pair_topk_spec.py,
        noisy_or  T_A = sum of the contributing taus + (n_contributing + S + 1 + C_NOISY) * U * A64 -- the S + 1 covers the
                  adds that join the base, single and cross partial sums of the level order -- and
                  T_P = exp(-max(A64 - T_A, 0)) * T_A;
        max       T_P = (largest contributing tau) / 4;
      an infinite logit has an exact P and adds nothing to T_P.  With TIPK_ERRLOG set every check prints and logs the
      largest (|B - B64| - sum_r w_r T_P,r) / (U * B64) - R it saw (profiles/combination_risk.md);
  (c) the selection, EXACTLY, against the returned fp32 burdens (`addon_spec.check_selection`): the k lowest non-NaN entries
      of the query's range by (value ascending, combination index ascending), values bit-equal, padding (+inf, -1).
"""
import itertools
import json
import os

import torch

from addon_spec import check_selection
from pair_topk_spec import U, known_mask, logits64
from regimen_spec import C_NOISY, softplus64

C_COMBO = 4.0      # observed on MI355X: 0.51 (profiles/combination_risk.md); "at most 30 x that and not below 4"


def _sizes(model):
    return model[1].shape[0], (model[2].shape[0] if model[0] == 'distmult' else model[1].shape[1])


def query_legal(fixed, slots, n, limits):
    """(legal, structural): structural = the slot structure itself is within the limits (the query owns prod A_s entries)."""
    sizes = [len(s) for s in slots]
    count = 1
    for a in sizes:
        count *= a
    structural = len(slots) <= limits.max_slots and all(a >= 1 for a in sizes) and sum(sizes) <= limits.max_alternatives \
        and count <= limits.max_combinations
    legal = structural and len(fixed) <= limits.max_fixed and all(0 <= d < n for d in fixed) and len(set(fixed)) == len(fixed) \
        and all(-1 <= d < n for s in slots for d in s)
    return legal, structural


def combination_count(fixed, slots, n, limits):
    count = 1
    for s in slots:
        count *= len(s)
    return count if query_legal(fixed, slots, n, limits)[1] else 1


def combo_ptr(queries, n, limits):
    ptr = [0]
    for fixed, slots in queries:
        ptr.append(ptr[-1] + combination_count(fixed, slots, n, limits))
    return torch.tensor(ptr, dtype=torch.int64)


def query_lists(queries):
    """The five flat lists of section 4n (host tensors) of `queries`, as given -- illegal ones included."""
    fix, fptr, alt, aptr, sptr = [], [0], [], [0], [0]
    for fixed, slots in queries:
        fix += list(fixed)
        fptr.append(len(fix))
        for s in slots:
            alt += list(s)
            aptr.append(len(alt))
        sptr.append(len(aptr) - 1)
    return (torch.tensor(fix, dtype=torch.int32), torch.tensor(fptr, dtype=torch.int64), torch.tensor(alt, dtype=torch.int32),
            torch.tensor(aptr, dtype=torch.int64), torch.tensor(sptr, dtype=torch.int64))


def _spec_query(model, fixed, slots, aggregate, w, known, c_noisy, budget=1 << 22):
    """fp64 (B64, TP_w, P64 [C, R], applicable) of the combinations of one LEGAL query."""
    n, R = _sizes(model)
    dev = model[1].device
    S, m = len(slots), len(fixed)
    combos = torch.tensor(list(itertools.product(*slots)), dtype=torch.int64, device=dev).reshape(-1, S) if S \
        else torch.zeros((1, 0), dtype=torch.int64, device=dev)
    C = combos.shape[0]
    ids = torch.cat([torch.tensor(fixed, dtype=torch.int64, device=dev)[None, :].expand(C, m), combos], 1)   # the regimen, -1: absent
    pos_i, pos_j = torch.triu_indices(m + S, m + S, offset=1, device=dev)
    B64 = torch.zeros(C, dtype=torch.float64, device=dev)
    TP_w = torch.zeros(C, dtype=torch.float64, device=dev)
    P_all = torch.zeros((C, R), dtype=torch.float64, device=dev)
    ok = torch.ones(C, dtype=torch.bool, device=dev)
    n_pairs = max(int(pos_i.numel()), 1)
    step = max(1, budget // (n_pairs * R))
    for c0 in range(0, C, step):
        part = ids[c0:c0 + step]
        c = part.shape[0]
        a, b = part[:, pos_i], part[:, pos_j]                              # [c, P]
        there = (a >= 0) & (b >= 0)
        ok[c0:c0 + c] &= ~(there & (a == b)).any(1)
        use = there & (a != b)
        row, col = torch.nonzero(use, as_tuple=True)
        u, v = torch.minimum(a[row, col], b[row, col]), torch.maximum(a[row, col], b[row, col])
        L, tau = logits64(model, u, v)                                     # [pairs of the chunk, R]
        free = ~known_mask(known, u, v, n, R)
        nan_rows = (free & torch.isnan(L)).any(1)
        ok[c0:c0 + c] &= torch.zeros(c, dtype=torch.int64, device=dev).index_add_(0, row, nan_rows.long()) == 0
        contrib = free & ~torch.isnan(L)
        tau_c = torch.where(contrib & ~torch.isinf(L), tau, torch.zeros_like(tau))
        zero = torch.zeros((c, R), dtype=torch.float64, device=dev)
        if aggregate == 'noisy_or':
            A64 = zero.clone().index_add_(0, row, torch.where(contrib, softplus64(L), torch.zeros_like(L)))
            n_con = zero.clone().index_add_(0, row, contrib.double())
            fin = torch.isfinite(A64)
            Af = torch.where(fin, A64, torch.zeros_like(A64))
            T_A = zero.clone().index_add_(0, row, tau_c) + (n_con + S + 1 + c_noisy) * U * Af
            P64 = -torch.expm1(-A64)
            T_P = torch.where(fin, torch.exp(-(Af - T_A).clamp(min=0)) * T_A, torch.zeros_like(A64))
        else:
            assert aggregate == 'max'
            idx = row[:, None].expand(-1, R)
            Lmax = torch.full((c, R), float('-inf'), dtype=torch.float64, device=dev).scatter_reduce_(
                0, idx, torch.where(contrib, L, torch.full_like(L, float('-inf'))), 'amax', include_self=True)
            P64 = torch.sigmoid(Lmax)
            T_P = zero.clone().scatter_reduce_(0, idx, tau_c, 'amax', include_self=True) / 4
        P64 = torch.where(torch.isnan(P64), torch.zeros_like(P64), P64)    # (rows that are not applicable anyway)
        B64[c0:c0 + c] = (P64 * w).sum(1)
        TP_w[c0:c0 + c] = (T_P * w).sum(1)
        P_all[c0:c0 + c] = P64
    return B64, TP_w, P_all, ok


def spec_combo_burden(model, queries, aggregate, limits, weights=None, known=None, c_combo=C_COMBO, c_noisy=C_NOISY):
    """fp64 tables of the rule on the model's device: dict with B64 [T] (NaN where illegal or not applicable), T_B [T], TP_w
    [T], P64 [T, R], applicable [T], ptr [G + 1], R."""
    n, R = _sizes(model)
    dev = model[1].device
    w = torch.ones(R, dtype=torch.float64, device=dev) if weights is None else torch.as_tensor(weights).to(dev).double()
    ptr = combo_ptr(queries, n, limits)
    T = int(ptr[-1])
    B64 = torch.zeros(T, dtype=torch.float64, device=dev)
    TP_w = torch.zeros(T, dtype=torch.float64, device=dev)
    P64 = torch.zeros((T, R), dtype=torch.float64, device=dev)
    ok = torch.zeros(T, dtype=torch.bool, device=dev)
    for g, (fixed, slots) in enumerate(queries):
        if not query_legal(fixed, slots, n, limits)[0]:
            continue
        a, b = int(ptr[g]), int(ptr[g + 1])
        B64[a:b], TP_w[a:b], P64[a:b], ok[a:b] = _spec_query(model, list(fixed), [list(s) for s in slots], aggregate, w, known,
                                                             c_noisy)
    T_B = TP_w + (R + c_combo) * U * B64
    nan = torch.full_like(B64, float('nan'))
    return dict(B64=torch.where(ok, B64, nan), T_B=torch.where(ok, T_B, nan), TP_w=TP_w, P64=P64, applicable=ok,
                ptr=ptr.to(dev), R=R, dev=dev)


def check_combo_burden(model, queries, k, aggregate, got, limits, weights=None, known=None, c_combo=C_COMBO, what=''):
    """Assert the acceptance rule for got = (burden [T], best_burden [G, k] or None, best_comb [G, k] or None)."""
    t = spec_combo_burden(model, queries, aggregate, limits, weights, known, c_combo)
    dev = t['dev']
    B = got[0].to(dev).reshape(-1)
    assert B.dtype == torch.float32 and B.numel() == t['B64'].numel(), (B.dtype, B.numel(), t['B64'].numel())
    ok = t['applicable']
    # (a) NaN placement
    assert torch.equal(torch.isnan(B), ~ok), ('NaN placement', int((torch.isnan(B) != ~ok).sum()))
    # (b) tolerance
    off = (B.double() - t['B64']).abs()
    if os.environ.get('TIPK_ERRLOG') and bool(ok.any()):
        pos = ok & (t['B64'] > 0) & torch.isfinite(t['B64'])
        if bool(pos.any()):
            seen = ((off - t['TP_w']) / (U * t['B64']) - t['R'])[pos]
            line = {'what': 'combo burden c', 'case': what, 'aggregate': aggregate, 'n': int(pos.sum()),
                    'observed_c': float(seen.max()), 'max_rel_err_in_u': float((off / (U * t['B64']))[pos].max()),
                    'c_combo': c_combo}
            print('ERR %s' % json.dumps(line))
            with open(os.environ['TIPK_ERRLOG'], 'a') as f:
                f.write(json.dumps(line) + '\n')
    good = (B.double() == t['B64']) | (off <= t['T_B'])
    assert bool(good[ok].all()), ('burden off fp64', float((off - t['T_B'])[ok & ~good].max()), int((ok & ~good).sum()))
    # (c) selection
    if k == 0:
        assert got[1] is None and got[2] is None
    else:
        check_selection(B, t['ptr'], k, got[1].to(dev), got[2].to(dev))
    return t
