"""Host models of the device quality metrics (idn.mse / idn.psnr / idn.ssim) and the inputs the
metric tests share.

Two statements of skimage 0.14.2's measure.compare_mse / compare_psnr / compare_ssim
(multichannel=True, uniform window, sample covariance, uint8 images, data_range 255):

  *_int    the exact-integer form the kernel implements: box sums of x, y, x^2, y^2, xy in int64
           (cumsum), cx = NP sxx - sx^2 ..., S = (A1 A2) / (B1 B2) in float64 with the constants
           multiplied through by NP^2 and NP (NP - 1).  This is the definition the GPU tests hold
           the kernels to.
  compare_*  a line-by-line restatement of skimage's float code on scipy.ndimage.uniform_filter
           (float64, reflecting borders, crop (win - 1) // 2, mean), kept to pin the integer form
           to what skimage computes (tests/test_metrics.py: the two agree within 1e-12).
"""
import numpy as np

K1, K2, DATA_RANGE = 0.01, 0.03, 255


# ---- the exact-integer form ---------------------------------------------------------------------

def mse_int(x, y):
    """compare_mse of two uint8 arrays: integer sum of squares, one float64 division"""
    d = x.astype(np.int64) - y.astype(np.int64)
    return np.float64(int((d * d).sum())) / np.float64(d.size)


def psnr_of_mse(m):
    """compare_psnr from compare_mse's value (float64 scalar or array); +inf for 0"""
    with np.errstate(divide="ignore"):
        return 10 * np.log10((DATA_RANGE ** 2) / np.asarray(m, np.float64))


def _box(a, win):
    """sums of a (int64, H x W) over every win x win window that lies inside it"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]


def ssim_int_plane(x, y, win):
    """one channel (H x W uint8): the mean of S over the windows inside the image"""
    x = x.astype(np.int64)
    y = y.astype(np.int64)
    NP = win * win
    sx, sy = _box(x, win), _box(y, win)
    sxx, syy, sxy = _box(x * x, win), _box(y * y, win), _box(x * y, win)
    cx = NP * sxx - sx * sx
    cy = NP * syy - sy * sy
    cxy = NP * sxy - sx * sy
    C1 = (K1 * DATA_RANGE) ** 2
    C2 = (K2 * DATA_RANGE) ** 2
    c1s = C1 * float(NP * NP)
    c2s = C2 * float(NP * (NP - 1))
    A1 = (2 * sx * sy).astype(np.float64) + c1s
    B1 = (sx * sx + sy * sy).astype(np.float64) + c1s
    A2 = (2 * cxy).astype(np.float64) + c2s
    B2 = (cx + cy).astype(np.float64) + c2s
    S = (A1 * A2) / (B1 * B2)
    return S.mean(dtype=np.float64)


def ssim_int(x, y, win=7):
    """(H, W, C) uint8 pair -> (mean over channels, per-channel values)"""
    if win % 2 == 0 or min(x.shape[0], x.shape[1]) < win:
        raise ValueError("win_size must be odd and fit the image")
    ch = np.array([ssim_int_plane(x[..., k], y[..., k], win) for k in range(x.shape[-1])])
    return ch.mean(), ch


# ---- skimage 0.14.2's float code on scipy ---------------------------------------------------------

def compare_mse(im1, im2):
    im1 = im1.astype(np.float64)
    im2 = im2.astype(np.float64)
    return np.mean(np.square(im1 - im2), dtype=np.float64)


def compare_psnr(im_true, im_test):
    err = compare_mse(im_true, im_test)
    with np.errstate(divide="ignore"):
        return 10 * np.log10((DATA_RANGE ** 2) / err)


def _compare_ssim_plane(X, Y, win_size):
    from scipy.ndimage import uniform_filter
    if np.any((np.asarray(X.shape) - win_size) < 0):
        raise ValueError("win_size exceeds image extent")
    if not (win_size % 2 == 1):
        raise ValueError("Window size must be odd.")
    ndim = X.ndim
    X = X.astype(np.float64)
    Y = Y.astype(np.float64)
    NP = win_size ** ndim
    cov_norm = NP / (NP - 1)  # sample covariance
    ux = uniform_filter(X, size=win_size)
    uy = uniform_filter(Y, size=win_size)
    uxx = uniform_filter(X * X, size=win_size)
    uyy = uniform_filter(Y * Y, size=win_size)
    uxy = uniform_filter(X * Y, size=win_size)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = DATA_RANGE
    C1 = (K1 * R) ** 2
    C2 = (K2 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    D = B1 * B2
    S = (A1 * A2) / D
    pad = (win_size - 1) // 2
    return S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean()


def compare_ssim(X, Y, win_size=7):
    """multichannel=True: (mean over channels, per-channel values)"""
    nch = X.shape[-1]
    mssim = np.empty(nch)
    for ch in range(nch):
        mssim[ch] = _compare_ssim_plane(X[..., ch], Y[..., ch], win_size)
    return mssim.mean(), mssim


# ---- shared inputs ----------------------------------------------------------------------------------

# (N, H, W) at win 7, C = 3
SHAPES_WIN7 = [(1, 7, 7), (1, 8, 7), (2, 7, 40), (3, 64, 96), (2, 37, 53), (1, 33, 336),
               (2, 17, 344), (1, 130, 70), (1, 600, 1000)]
SHAPES_WIN_OTHER = [(1, 11, 11), (3, 64, 96), (2, 37, 53), (1, 130, 70)]  # win 3 and 11, C = 3
SHAPES_C1 = [(2, 37, 53), (1, 64, 96)]                                    # win 7, C = 1
# (shape, C, win)
CASES = ([(s, 3, 7) for s in SHAPES_WIN7]
         + [(s, 3, win) for win in (3, 11) for s in SHAPES_WIN_OTHER]
         + [(s, 1, 7) for s in SHAPES_C1])
FAMILIES = ["noisy", "inverted", "same", "black_white", "random"]


def make_pair(family, shape, c):
    """(X, Y) uint8 (N, H, W, C) of one input family; every image of a batch has its own seed"""
    from conftest import textured
    n, h, w = shape
    base = 1000 * FAMILIES.index(family) + h + 3 * w + c
    if family == "black_white":
        return np.zeros((n, h, w, c), np.uint8), np.full((n, h, w, c), 255, np.uint8)
    if family == "random":
        xs = [np.random.RandomState(base + 7 * i).randint(0, 256, (h, w, c)) for i in range(n)]
        ys = [np.random.RandomState(base + 7 * i + 3).randint(0, 256, (h, w, c)) for i in range(n)]
        return np.stack(xs).astype(np.uint8), np.stack(ys).astype(np.uint8)
    X = np.stack([textured(1, h, w, c, seed=base + 7 * i)[0] for i in range(n)])
    if family == "same":
        return X, X.copy()
    if family == "inverted":
        return X, (255 - X).astype(np.uint8)
    noise = np.stack([np.random.RandomState(base + 7 * i + 5).normal(0, 25, (h, w, c))
                      for i in range(n)])
    return X, np.clip(np.rint(X + noise), 0, 255).astype(np.uint8)
