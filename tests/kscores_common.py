"""The fp64 yardstick of the ensemble scores (CFNERF_F_KSCORES, cfnerf_kscores.hip) and the inputs its tests share: numpy only, no GPU.

For a row x_0 .. x_K-1 with order statistics x_(0) <= .. <= x_(K-1) and a target y:
  rank_code = 2 #{x_k < y} + #{x_k == y}                     (integers: exact)          pit = float32(rank_code) / float32(2K)
  quantile at q: numpy.quantile(method="linear")             = x_(lo) + frac (x_(hi) - x_(lo)), lo = floor(q (K-1)), hi = min(lo + 1, K - 1)
  crps = A - B,   A = (1/K) sum_k |x_k - y|,   B = (1/K^2) sum_{g<K-1} (g+1)(K-1-g) (x_(g+1) - x_(g))
B is the ensemble's 1/(2K^2) sum_kl |x_k - x_l| written over the sorted gaps (``crps_brute`` is that double sum as it stands).
Calibration: with truth and samples exchangeable #below is uniform on 0..K; ``ideal_coverage`` counts the rule of evaluate.calibration."""
import numpy as np

LEVELS = (0, 0.05, 0.25, 0.5, 0.75, 0.95, 1)
U24 = 2.0 ** -24


def make_rows(M, K, seed, special=True):
    """samples [M,K] and targets [M] in fp32.  Row i draws uniform values at scale i % 4 of ([0,1), 0.5 + 1e-3 u, 2 + 6 u, 1 + 1e-6 u); one
    quarter of the rows (i % 16 in 0..3: each scale once) is rounded to multiples of 1/4, which forces ties; one row in seven has its target
    equal to one of its samples.  With ``special`` and M >= 64 rows 20, 21, 22 hold +-0, +-inf and denormals."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (M, K))
    uy = rng.uniform(0, 1, M)
    scale = np.arange(M) % 4
    lo = np.array([0.0, 0.5, 2.0, 1.0])[scale]
    w = np.array([1.0, 1e-3, 6.0, 1e-6])[scale]
    x = (lo[:, None] + w[:, None] * u).astype(np.float32)
    y = (lo + w * uy).astype(np.float32)
    tie = (np.arange(M) % 16) < 4
    x[tie] = np.round(x[tie] * 4) / 4
    y[tie] = np.round(y[tie] * 4) / 4
    hit = np.arange(M) % 7 == 3
    y[hit] = x[hit, rng.integers(0, K, M)[hit]]
    if special and M >= 64:
        z = np.array([0.0, -0.0], np.float32)
        x[20] = z[rng.integers(0, 2, K)]
        y[20] = 0.0
        x[21, 0] = np.inf
        if K > 1:
            x[21, K - 1] = -np.inf
        den = np.float32(1e-45) * rng.integers(1, 1000, K).astype(np.float32)
        x[22] = den * np.where(rng.integers(0, 2, K) > 0, 1, -1).astype(np.float32)
        y[22] = np.float32(3e-43)
    return x, y


def rank_code(x, y):
    return (2 * (x < y[:, None]).sum(1) + (x == y[:, None]).sum(1)).astype(np.int32)


def pit_of(code, K):
    return (code.astype(np.float32) / np.float32(2 * K)).astype(np.float32)


def crps_terms(x, y):
    """(A, B) in fp64 from fp32 (or fp64) rows: the gap form"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    K = x.shape[1]
    A = np.abs(x - y[:, None]).sum(1) / K
    xs = np.sort(x, 1)
    g = np.arange(K - 1)
    B = (((g + 1) * (K - 1 - g))[None] * (xs[:, 1:] - xs[:, :-1])).sum(1) / (K * K) if K > 1 else np.zeros(x.shape[0])
    return A, B


def crps_brute(x, y):
    """the definition: mean |x_k - y| - 1/(2 K^2) sum_k sum_l |x_k - x_l|, fp64"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    K = x.shape[1]
    return np.abs(x - y[:, None]).mean(1) - np.abs(x[:, :, None] - x[:, None, :]).sum((1, 2)) / (2.0 * K * K)


def quantiles64(x, levels=LEVELS):
    """numpy.quantile(method="linear") of the rows in fp64 -> [M,Q], with the brackets (lo, hi) per level and whether frac == 0"""
    x = np.asarray(x, np.float64)
    K = x.shape[1]
    with np.errstate(invalid="ignore"):
        q = np.quantile(x, np.asarray(levels, np.float64), axis=1, method="linear").T
    pos = np.asarray(levels, np.float64) * (K - 1)
    lo = np.floor(pos).astype(int)
    hi = np.minimum(lo + 1, K - 1)
    return q, lo, hi, (pos - lo).astype(np.float32) == 0


def ideal_coverage(K, tenths=range(1, 10)):
    """#{b in 0..K : 10 |2b - K| <= j K} / (K + 1) for j in ``tenths``"""
    b = np.arange(K + 1)
    return np.array([np.count_nonzero(10 * np.abs(2 * b - K) <= j * K) / (K + 1) for j in tenths])


def coverage_of(code, K, tenths=range(1, 10)):
    """the share of rows with 10 |code - K| <= j K, for j in ``tenths`` (code >= 0)"""
    d = 10 * np.abs(code.astype(np.int64) - K)
    return np.array([np.mean(d <= j * K) for j in tenths])
