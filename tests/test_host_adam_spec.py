"""The acceptance rule of tests/adam_spec.py, checked on the CPU against an fp32 emulation of the kernel's operation order:
it admits the arithmetic it was derived for on EVERY element, and it sees the defect it was written for (complements formed
in fp32 from the rounded betas)."""
import numpy as np
import pytest

import adam_spec as A

N = 100_000


@pytest.mark.parametrize('contract', [False, True], ids=['plain', 'fma'])
@pytest.mark.parametrize('name', list(A.HYPER))
def test_emulation_with_double_rounded_complements_is_inside_the_bounds(name, contract):
    hyper = A.HYPER[name]
    worst = {'dP': 0.0, 'dM': 0.0, 'dV': 0.0}
    for k, done in enumerate(A.STEPS_DONE):
        before = A.rule_state(N, done, seed=100 + k, zero_g=name != 'eps_0')
        got = A.emulate_fp32(*before, done + 1, **hyper, contract=contract)
        used = A.check(got, before, done + 1, hyper, what=(name, done, contract))      # all N elements, none left out
        worst = {key: max(worst[key], used[key]) for key in worst}
        p, g, m, v = before
        if hyper['weight_decay'] == 0.0 and name != 'eps_0':                       # (with decay g' = wd p moves such an element)
            still = (g == 0) & (m == 0) & (v == 0)
            assert still.any() and np.array_equal(got[0][still].view(np.int32), p[still].view(np.int32))
        if hyper['lr'] == 0.0:
            assert np.array_equal(got[0].view(np.int32), p.view(np.int32))
    print('adam_spec shares %s %s: dP %.3f dM %.3f dV %.3f' % (name, 'fma' if contract else 'plain', worst['dP'],
                                                                 worst['dM'], worst['dV']))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('beta2', [0.999, 0.9999])
def test_float_complements_fall_outside_the_bound_on_exp_avg_sq(beta2):
    """1.0f - (float)beta2 is 216 u (beta2 = 0.999) or 2784 u (0.9999) off 1 - beta2; dV allows 3 u of V.  On a first step
    (v = 0) V = (1 - beta2) g^2, so every element with g != 0 must be outside."""
    hyper = dict(A.HYPER['default'], beta2=beta2)
    before = A.rule_state(N, 0, seed=7)
    g = before[1]
    for contract in (False, True):
        _, _, V = A.emulate_fp32(*before, 1, **hyper, float_complements=True, contract=contract)
        want = A.adam_step64(*before, 1, **hyper)[2]
        dV = A.adam_bounds(*before, 1, **hyper)[2]
        outside = np.abs(V.astype(np.float64) - want) > dV
        assert outside[g != 0].mean() > 0.5, outside[g != 0].mean()
        assert not outside[g == 0].any()
        with pytest.raises(AssertionError, match='dV'):
            A.check(A.emulate_fp32(*before, 1, **hyper, float_complements=True, contract=contract), before, 1, hyper)
    # the same complement, a later step (v over 1e-9 ... 100 beside g^2 over 1e-8 ... 100): still seen
    before = A.rule_state(N, 6, seed=8)
    with pytest.raises(AssertionError, match='dV'):
        A.check(A.emulate_fp32(*before, 7, **hyper, float_complements=True), before, 7, hyper)


def test_complement_constants():
    """The figures the bound's assumption rests on: (float)(1 - beta) is within one rounding of 1 - beta, 1.0f - (float)beta
    is not."""
    f = np.float32
    for beta, far in ((0.999, 200), (0.9999, 2500), (0.9, 3)):
        exact = 1.0 - beta
        assert abs(float(f(exact)) - exact) <= A.U * exact
        assert abs(float(f(1.0) - f(beta)) - exact) > far * A.U * exact
