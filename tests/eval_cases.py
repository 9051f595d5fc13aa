"""Score lists of the evaluation tests (tests/test_gpu_eval_paths.py, tests/test_host_logic.py): every builder returns
fp32 (pos, neg) arrays of n scores each, from a fixed seed.  The reference of all of them is sklearn on float64 copies
(`oracle.tip_oracle.auprc_auroc_ap`)."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def sklearn_metrics(pos, neg):
    """(AUPRC, AUROC, AP) of one relation by sklearn, as the reference calls it, on float64 copies of the scores;
    +-inf enter as +-FLT_MAX (same order: sklearn subtracts neighbouring scores, inf - inf would be NaN)."""
    from oracle import tip_oracle as O
    pos, neg = np.asarray(pos), np.asarray(neg)
    s = np.r_[pos, neg].astype(np.float64)
    assert not (np.abs(s[np.isfinite(s)]) >= FLT_MAX).any()          # no other score may meet the stand-in
    s = np.where(np.isinf(s), np.sign(s) * float(FLT_MAX), s)
    return np.array(O.auprc_auroc_ap(np.r_[np.ones(pos.size), np.zeros(neg.size)], s))


def continuous(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(n) * 0.6 + 0.3).astype(np.float32), (rng.rand(n) * 0.7).astype(np.float32)


def one_decimal(n, seed):
    """11 distinct values: at n >= 512 a tie group spans many threads' chunks of ranks."""
    p, q = continuous(n, seed)
    return np.round(p, 1), np.round(q, 1)


def _sigmoid32(x):
    with np.errstate(over='ignore'):
        return (np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))).astype(np.float32)


def sigmoid_logits(n, seed, scale=1.0):
    """sigmoid of N(+2, 3) / N(-2, 3) logits (times `scale`) evaluated in fp32: the top of the positives crowds against
    1.0 and the bottom of the negatives runs toward 0."""
    rng = np.random.RandomState(seed)
    return _sigmoid32(scale * (2 + 3 * rng.randn(n))), _sigmoid32(scale * (-2 + 3 * rng.randn(n)))


def saturated_sigmoid(n, seed):
    """The same logits times 8: fp32 sigma is exactly 1.0 above ~17 (about half of the positives, a tenth of the
    negatives), and the low end runs through the denormals to exact 0."""
    return sigmoid_logits(n, seed, scale=8.0)


def all_equal(n, value=0.25):
    return np.full(n, value, np.float32), np.full(n, value, np.float32)


def separated(n, seed, inverted=False):
    """Distinct scores, every positive above every negative (or below, inverted)."""
    rng = np.random.RandomState(seed)
    hi = (0.5 + (1 + rng.permutation(n)) / (4.0 * n)).astype(np.float32)
    lo = (0.25 * (1 + rng.permutation(n)) / n).astype(np.float32)
    assert np.unique(hi).size == n and np.unique(lo).size == n and lo.max() < hi.min()
    return (lo, hi) if inverted else (hi, lo)


def logits(n, seed):
    """Raw decoder outputs (sigmoid=0): both signs, large magnitudes, and fp32 denormals of both signs."""
    rng = np.random.RandomState(seed)
    p, q = (3 + 40 * rng.randn(n)).astype(np.float32), (-3 + 40 * rng.randn(n)).astype(np.float32)
    tiny = np.float32(1e-45)                                          # the smallest denormal
    for a in (p, q):
        k = max(1, n // 5)
        a[rng.choice(n, k, replace=False)] = (rng.randint(-40, 41, k) * tiny).astype(np.float32)   # some are +-0.0
    return p, q


def signed_zeros(n, seed):
    """About half exact zeros of either sign in both classes -- the positives mostly -0.0, the negatives mostly +0.0, so
    an order that ranks +0.0 above -0.0 is far from the tie -- next to small positive and negative values (denormals
    included)."""
    rng = np.random.RandomState(seed)
    out = []
    for minus_share in (0.8, 0.2):
        a = (rng.randn(n) * 1e-3).astype(np.float32)
        a[rng.rand(n) < 0.1] = np.float32(1e-45) * rng.choice([-1, 1])
        zero = rng.rand(n) < 0.5
        a[zero] = np.where(rng.rand(int(zero.sum())) < minus_share, np.float32(-0.0), np.float32(0.0))
        out.append(a)
    if n >= 4:                                                        # both signs in both classes, whatever the draw
        for a in out:
            a[0], a[1] = np.float32(0.0), np.float32(-0.0)
    return out[0], out[1]


def infinities(n, seed):
    """Logits with +inf and -inf in both classes (several of each, so equal infinities have to tie)."""
    rng = np.random.RandomState(seed)
    p, q = (1 + 5 * rng.randn(n)).astype(np.float32), (-1 + 5 * rng.randn(n)).astype(np.float32)
    for a in (p, q):
        k = max(1, n // 16)
        a[rng.choice(n, 2 * k, replace=False)] = np.r_[np.full(k, np.inf), np.full(k, -np.inf)].astype(np.float32)
    return p, q
