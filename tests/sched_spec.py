"""The scheduler's arithmetic restated in plain numpy float64 (no oracle or
device code), for tests/test_scheduler.py: scheduler weights, the deterministic
total (256-cell stride trees, then the heap tree over the blocks), and the
CONSTANT and INTEGRATED budgets.  PROBABILISTIC budgets are draws; the spec
holds their distribution only (multinomial_p, chi2_sf).

Every function takes one entry per cell; a cell without a living organism has
weight 0 (the caller masks it)."""
import math

import numpy as np

AVE_TIME_SLICE = 30
DBL_MAX = float(np.finfo(np.float64).max)
WEIGHT_CAP = math.ldexp(1.0, 990)
LAM_CLAMP = 1.0e8
BLOCK = 256


def weights(merit, head_start=None):
    """A merit's scheduler weight: 0 unless 0 <= m <= DBL_MAX (NaN, inf and
    negative merits are never scheduled); m (1 + hs / 65536) while a head start
    hs is set, 0 if that product overflows; at most 2^990."""
    m = np.asarray(merit, dtype=np.float64)
    hs = np.zeros(m.shape) if head_start is None else np.asarray(head_start, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (m >= 0.0) & (m <= DBL_MAX)
        w = np.where(hs != 0.0, m * (1.0 + hs / 65536.0), m)
        ok &= w <= DBL_MAX
        return np.where(ok, np.minimum(w, WEIGHT_CAP), 0.0)


def block_partials(w):
    """per 256-cell block (the last one zero-padded) the stride tree
    s[t] += s[t + stride], strides 128, 64, ..., 1"""
    w = np.asarray(w, dtype=np.float64)
    nb = (len(w) + BLOCK - 1) // BLOCK
    s = np.zeros(nb * BLOCK)
    s[:len(w)] = w
    s = s.reshape(nb, BLOCK)
    stride = BLOCK // 2
    while stride >= 1:
        s = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0]


def tree_total(w):
    """the deterministic total: the block partials, zero-padded to a power of
    two, summed as a heap tree (pairs t[0::2] + t[1::2] up to the root)"""
    part = block_partials(w)
    P = 1
    while P < len(part):
        P *= 2
    t = np.zeros(P)
    t[:len(part)] = part
    while len(t) > 1:
        t = t[0::2] + t[1::2]
    return float(t[0])


def constant_budgets(alive, ave=AVE_TIME_SLICE):
    """CONSTANT (and the fallback when the total weight is not positive):
    AVE_TIME_SLICE for every living organism"""
    return np.where(np.asarray(alive, dtype=bool), ave, 0).astype(np.int64)


def integrated_budgets(w, credit, ud):
    """INTEGRATED: lam = (ud w) / total, at most 1e8; cr = credit + lam;
    budget floor(cr), new credit cr - floor(cr) -- in this order of
    operations.  Returns (budgets, credits)."""
    w = np.asarray(w, dtype=np.float64)
    total = tree_total(w)
    assert total > 0.0
    lam = np.minimum((float(ud) * w) / total, LAM_CLAMP)
    cr = np.asarray(credit, dtype=np.float64) + lam
    fl = np.floor(cr)
    return fl.astype(np.int64), cr - fl


def multinomial_p(w):
    """PROBABILISTIC: an update's budgets are Multinomial(UD, w / sum w)"""
    w = np.asarray(w, dtype=np.float64)
    return w / math.fsum(w.tolist())


def chi2_sf(x, dof):
    """upper-tail probability of a chi-square variate: the regularised
    incomplete gamma function Q(dof / 2, x / 2), by its series below
    a + 1 and by its continued fraction (modified Lentz) above"""
    a, x = 0.5 * dof, 0.5 * x
    if x <= 0.0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        k = a
        for _ in range(10000):
            k += 1.0
            term *= x / k
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * lead
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * lead
