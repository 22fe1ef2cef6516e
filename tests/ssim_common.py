"""The yardstick and the shared cases of the SSIM tests (numpy only).

``yardstick``: an fp64 restatement of the documented algorithm of ``skimage.metrics.structural_similarity`` (Wang et al. 2004) on the VALID
region - skimage filters the whole image and crops ``(win - 1) / 2`` pixels from every side before it takes the mean, which leaves exactly
the windows that lie inside the image.  Both window kinds: the uniform ``win x win`` box with the sample covariance ``n / (n - 1)``
(skimage's default, ``win = 7``) and the Gaussian of ``gaussian_weights=True`` (``sigma = 1.5``, radius ``int(3.5 sigma + 0.5)``, population
covariance), its taps normalised in double and NOT rounded to fp32.  Per channel, then the mean over the channels.

``naive32``: the same closed form, ``E[x^2] - mu^2``, in numpy fp32 - what a torch user would write.

``CASES``: the image pairs of the tests, all from seed 0."""
import functools

import numpy as np

CASES = ("uniform", "render", "bright_flat", "identical", "constant", "far", "one_nan")
# H, W, C, win (the tile of ssim_kernel is 32 x 32 output pixels)
SHAPES = [(7, 7, 1, 7),          # one output pixel
          (8, 9, 3, 7),          # the smallest image with more than one output pixel
          (38, 39, 3, 7),        # interior 32 x 33: exactly one tile in one axis, one past it in the other
          (45, 70, 3, 7),        # ragged, multi-tile, uniform window
          (45, 70, 3, 11),       # ragged, multi-tile, Gaussian window
          (20, 20, 4, 15),       # the widest window, four channels
          (12, 12, 2, 3)]        # the narrowest window
SIGMA = 1.5


def window_kind(win):
    """the shape table's rule: the 11-tap window is the Gaussian one (sigma = 1.5), every other one is uniform"""
    return "gaussian" if win == 11 else "uniform"


def gaussian_taps(win, sigma=SIGMA):
    r = (win - 1) // 2
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * i ** 2)
    return w / w.sum()


def _separable(a, taps):
    """valid-region correlation of a [H,W,C] with taps (x) taps, accumulated in a's dtype, tap by tap"""
    H, W = a.shape[:2]
    n = len(taps)
    h = np.zeros((H, W - n + 1) + a.shape[2:], a.dtype)
    for j in range(n):
        h += taps[j] * a[:, j:j + W - n + 1]
    v = np.zeros((H - n + 1, W - n + 1) + a.shape[2:], a.dtype)
    for i in range(n):
        v += taps[i] * h[i:i + H - n + 1]
    return v


def _box(a, n):
    """valid-region n x n box mean in a's dtype: the running sums, then one division by n^2"""
    one = np.ones(n, a.dtype)
    return _separable(a, one) / a.dtype.type(n * n)


def _closed_form(x, y, kind, win, data_range, dt, sigma=SIGMA):
    x, y = x.astype(dt), y.astype(dt)
    c1, c2 = dt((0.01 * data_range) ** 2), dt((0.03 * data_range) ** 2)
    if kind == "uniform":
        n = win * win
        cov = dt(n / (n - 1.0))
        f = lambda a: _box(a, win)
    else:
        cov = dt(1.0)
        taps = gaussian_taps(win, sigma).astype(dt)
        f = lambda a: _separable(a, taps)
    with np.errstate(invalid="ignore"):
        mx, my = f(x), f(y)
        vx, vy, vxy = cov * (f(x * x) - mx * mx), cov * (f(y * y) - my * my), cov * (f(x * y) - mx * my)
        return ((dt(2) * mx * my + c1) * (dt(2) * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def yardstick(x, y, kind="uniform", win=7, data_range=1.0, sigma=SIGMA):
    """(map [H-win+1, W-win+1, C] in fp64, the mean over the interior per channel and then over the channels) of x, y [H,W,C]"""
    S = _closed_form(x, y, kind, win, data_range, np.float64, sigma)
    return S, float(S.mean(axis=(0, 1)).mean())


def naive32(x, y, kind="uniform", win=7, data_range=1.0, sigma=SIGMA):
    """the same closed form in fp32, no pivot; the mean taken in fp64 of the fp32 map"""
    S = _closed_form(x, y, kind, win, data_range, np.float32, sigma)
    return S, float(S.astype(np.float64).mean(axis=(0, 1)).mean())


NAN_AT = lambda H, W, C: (H // 2, (2 * W) // 3, C - 1)          # the NaN pixel of `one_nan` (row, column, channel)


@functools.lru_cache(maxsize=None)
def make_case(name, H, W, C):
    """(x, y) [H,W,C] fp32, seed 0.  Read-only: shared among the tests."""
    rng = np.random.default_rng(0)
    noisy = lambda a: np.clip(a + 0.02 * rng.standard_normal(a.shape), 0.0, 1.0)
    if name == "uniform":
        x, y = rng.random((H, W, C)), rng.random((H, W, C))
    elif name in ("render", "one_nan"):
        yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        x = np.clip(0.5 + 0.4 * np.sin((xx + 3 * cc) / 9.0) * np.cos(yy / 7.0), 0.0, 1.0)
        y = noisy(x)
        if name == "one_nan":
            x[NAN_AT(H, W, C)] = np.nan
    elif name == "bright_flat":
        x = 0.97 + 0.002 * rng.standard_normal((H, W, C))
        y = noisy(x)
    elif name == "identical":
        x = rng.random((H, W, C))
        y = x.copy()
    elif name == "constant":
        x, y = np.full((H, W, C), 0.3), np.full((H, W, C), 0.7)
    elif name == "far":
        x, y = np.zeros((H, W, C)), np.ones((H, W, C))
    else:
        raise KeyError(name)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(name, H, W, C, win):
    """((yardstick map, mean), (naive32 map, mean)) of a case: computed once, shared, read-only"""
    x, y = make_case(name, H, W, C)
    kind = window_kind(win)
    out = yardstick(x, y, kind, win), naive32(x, y, kind, win)
    for S, _ in out:
        S.setflags(write=False)
    return out


def max_err(got, ref):
    """max |got - ref| over the entries where ref is finite; the NaN patterns must be the same"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "the NaN entries differ"
    ok = ~np.isnan(ref)
    return float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
