"""float64 restatement of the full-reference metric definitions (INTEGRATION.md 'Metrics') and of eval_metrics.py's per-clip steps,
in numpy: the yardstick of tests/test_metrics_cpu.py and tests/test_metrics_gpu.py."""
import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def window_1d():
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-((i - 5) ** 2) / 4.5)
    return g / g.sum()


def fspecial(size=11, sigma=1.5):
    """pyiqa's fspecial('gaussian') construction: 2-D np.ogrid Gaussian, tiny values zeroed, normalised."""
    m = n = (size - 1.0) / 2.0
    y, x = np.ogrid[-m:m + 1, -n:n + 1]
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h / h.sum()


def to01(img):
    """uint8 -> u/255 in float64; float arrays -> float64 as they are."""
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def rgb_to_y(img):
    """eval_metrics.py rgb_to_y on [N,3,H,W] float64 -> [N,1,H,W]."""
    r, g, b = img[:, 0:1], img[:, 1:2], img[:, 2:3]
    return 0.257 * r + 0.504 * g + 0.098 * b + 0.0625


def luma(img):
    """[N,C,H,W] float64 in [0,1] -> [N,H,W] luma on 0..255, rounded half-to-even."""
    if img.shape[1] == 3:
        return np.rint(255.0 * (0.299 * img[:, 0] + 0.587 * img[:, 1] + 0.114 * img[:, 2]))
    return np.rint(255.0 * img[:, 0])


def _filter_valid(x, g):
    """separable 'valid' filtering of [N,H,W] with the 11-tap g along H then W."""
    v = np.lib.stride_tricks.sliding_window_view(x, 11, axis=1) @ g
    return np.lib.stride_tricks.sliding_window_view(v, 11, axis=2) @ g


def ssim(x, y):
    """[N,C,H,W] float64 in [0,1] -> [N] SSIM (pyiqa 'ssim': Y channel, no downsampling)."""
    X, Y = luma(x), luma(y)
    g = window_1d()
    mx, my = _filter_valid(X, g), _filter_valid(Y, g)
    sxx = _filter_valid(X * X, g) - mx * mx
    syy = _filter_valid(Y * Y, g) - my * my
    sxy = _filter_valid(X * Y, g) - mx * my
    cs = np.maximum((2 * sxy + C2) / (sxx + syy + C2), 0.0)
    lum = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    return (lum * cs).reshape(len(x), -1).mean(1)


def psnr(x, y):
    """[N,C,H,W] float64 in [0,1] -> [N] PSNR in dB (pyiqa 'psnr', data range 1)."""
    mse = ((x - y) ** 2).reshape(len(x), -1).mean(1)
    return 10 * np.log10(1.0 / (mse + 1e-8))


def metrics(pred, ref, rgb_y=False):
    """[N,C,H,W] (uint8 or float) -> (psnr[N], ssim[N]) with eval_metrics.py's optional rgb_to_y first."""
    p, r = to01(pred), to01(ref)
    if rgb_y:
        p, r = rgb_to_y(p), rgb_to_y(r)
    return psnr(p, r), (ssim(p, r) if min(p.shape[2:]) >= 11 else None)


def clip_values(pred_fhwc, gt_fhwc, crop=0, test_y_channel=False, is_center=False):
    """eval_metrics.py per clip on [F,H,W,3] uint8: match_resolution, crop_border, rgb_to_y, mean over frames."""
    gt, pred = np.asarray(gt_fhwc).transpose(0, 3, 1, 2), np.asarray(pred_fhwc).transpose(0, 3, 1, 2)
    t = min(len(gt), len(pred))
    gt, pred = gt[:t], pred[:t]
    th, tw = min(gt.shape[2], pred.shape[2]), min(gt.shape[3], pred.shape[3])

    def cut(a):
        top, left = ((max((a.shape[2] - th) // 2, 0), max((a.shape[3] - tw) // 2, 0)) if is_center else (0, 0))
        return a[:, :, top:top + th, left:left + tw]

    gt, pred = cut(gt), cut(pred)
    if crop > 0:
        gt, pred = gt[:, :, crop:-crop, crop:-crop], pred[:, :, crop:-crop, crop:-crop]
    p, s = metrics(pred, gt, test_y_channel)
    return {"psnr": float(p.mean()), "ssim": float(s.mean())}


def structured_pair(rng, n, h, w, noise=20):
    """a smooth colour gradient and a noisy copy of it: SSIM well inside (0, 1)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 127 // max(h + w - 2, 1))], -1)
    base = np.broadcast_to(base, (n, h, w, 3)).astype(np.int64)
    noisy = np.clip(base + rng.normal(0, noise, base.shape).round(), 0, 255)
    return base.astype(np.uint8), noisy.astype(np.uint8)
