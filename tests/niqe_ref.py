"""fp64 numpy restatement of NIQE (pyiqa's 'niqe' with its defaults, a port of the MATLAB release) as INTEGRATION.md 1i defines it, written
from the definition and independently of csrc/niqe.hip: the half-scaling is the GENERAL MATLAB imresize weight computation (not the eight
taps the kernel uses), Gamma is math.gamma (the library builds its tables from lgamma), alpha is a literal first-index argmin over the grid,
and the pseudo-inverse is numpy's.  No run against pyiqa itself has been made: it is not available where this was written."""
import math

import numpy as np

BLOCK = 96
GAM = np.arange(0.2, 10.001, 0.001)                               # 9801 entries
assert GAM.shape == (9801,)
_G1 = np.array([math.gamma(1.0 / g) for g in GAM])
_G2 = np.array([math.gamma(2.0 / g) for g in GAM])
_G3 = np.array([math.gamma(3.0 / g) for g in GAM])
R_GAM = _G2 ** 2 / (_G1 * _G3)
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
EIGHT_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0


def to_unit_chw(img) -> np.ndarray:
    """[C,H,W] float in [0,1] or uint8 (u/255), or uint8 [H,W,3] -> float64 [C,H,W]."""
    a = np.asarray(img)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] in (1, 3) and a.shape[0] not in (1, 3):
        a = a.transpose(2, 0, 1)
    return a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)


def luma(img) -> np.ndarray:
    v = to_unit_chw(img)
    if v.shape[0] == 3:
        return np.round(255.0 * (0.299 * v[0] + 0.587 * v[1] + 0.114 * v[2]))     # numpy rounds half to even, as rint does
    return np.round(255.0 * v[0])


def gaussian_window() -> np.ndarray:
    x = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def gaussian_filter_replicate(a: np.ndarray) -> np.ndarray:
    g = gaussian_window()
    p = np.pad(a, 3, mode="edge")
    h = sum(g[k] * p[:, k:k + a.shape[1]] for k in range(7))
    return sum(g[k] * h[k:k + a.shape[0], :] for k in range(7))


def mscn(img: np.ndarray):
    mu = gaussian_filter_replicate(img)
    sigma = np.sqrt(np.abs(gaussian_filter_replicate(img * img) - mu * mu))
    return (img - mu) / (sigma + 1.0), sigma


def _cubic(x):
    ax = np.abs(x)
    return np.where(ax <= 1, 1.5 * ax ** 3 - 2.5 * ax ** 2 + 1, np.where(ax < 2, -0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2, 0.0))


def imresize_weights(in_len: int, scale: float):
    """MATLAB imresize's contributions for one dimension (bicubic, antialiasing on) -> (weights [out,P], 0-based source indices [out,P])."""
    out_len = int(math.ceil(in_len * scale))
    width = 4.0 / scale if scale < 1 else 4.0
    x = np.arange(1, out_len + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - width / 2)
    P = int(math.ceil(width)) + 2
    ind = left[:, None] + np.arange(P)[None]                      # 1-based
    d = u[:, None] - ind
    w = scale * _cubic(d * scale) if scale < 1 else _cubic(d)
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(in_len), np.arange(in_len - 1, -1, -1)])       # symmetric reflection
    return w, aux[np.mod(ind.astype(np.int64) - 1, 2 * in_len)]


def imresize(a: np.ndarray, scale: float) -> np.ndarray:
    w, idx = imresize_weights(a.shape[0], scale)
    a = np.einsum("op,opw->ow", w, a[idx])                        # along dim 0
    w, idx = imresize_weights(a.shape[1], scale)
    return np.einsum("op,hop->ho", w, a[:, idx])                  # along dim 1


def half_eight_taps(a: np.ndarray) -> np.ndarray:
    """The fixed 8-tap filter at source 2i-3 .. 2i+4 with symmetric reflection: what the general weights reduce to at exactly 0.5."""
    def along0(m):
        n = m.shape[0]
        aux = np.concatenate([np.arange(n), np.arange(n - 1, -1, -1)])
        out = np.zeros((n // 2,) + m.shape[1:])
        for i in range(n // 2):
            for k in range(8):
                out[i] += EIGHT_TAPS[k] * m[aux[(2 * i - 3 + k) % (2 * n)]]
        return out
    return along0(along0(a).T).T


def aggd(b: np.ndarray):
    """-> (grid index of alpha or -1, alpha, beta_l, beta_r); an empty sign set makes everything NaN."""
    b = b.ravel()
    with np.errstate(all="ignore"):
        neg, pos = b[b < 0], b[b > 0]
        left = np.sqrt(np.mean(neg ** 2)) if neg.size else np.nan
        right = np.sqrt(np.mean(pos ** 2)) if pos.size else np.nan
        gh = left / right
        rhat = np.mean(np.abs(b)) ** 2 / np.mean(b ** 2)
        R = (rhat * (gh ** 3 + 1) * (gh + 1)) / ((gh ** 2 + 1) ** 2)
    if np.isnan(R):
        return -1, np.nan, np.nan, np.nan
    k = int(np.argmin((R_GAM - R) ** 2))
    alpha = GAM[k]
    c = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return k, alpha, left * c, right * c


def block_features(m: np.ndarray):
    """18 features of one MSCN block and the 5 grid indices."""
    k, alpha, bl, br = aggd(m)
    feat, idx = [alpha, (bl + br) / 2], [k]
    for s in SHIFTS:
        k, alpha, bl, br = aggd(m * np.roll(m, s, axis=(0, 1)))
        mean = (br - bl) * (math.gamma(2 / alpha) / math.gamma(1 / alpha)) if k >= 0 else np.nan
        feat += [alpha, mean, bl, br]
        idx.append(k)
    return feat, idx


def features(img, perturb=None):
    """One image -> (features [B,36], sharpness [B], alpha grid indices [B,10]).  ``perturb`` = (numpy Generator, eps) multiplies the MSCN
    fields by 1 + eps * N(0,1): the probe for how close the alphas of an input sit to a grid midpoint."""
    y = luma(img)
    H, W = (y.shape[0] // BLOCK) * BLOCK, (y.shape[1] // BLOCK) * BLOCK
    if H == 0 or W == 0:
        raise ValueError("NIQE needs H and W >= 96")
    y = y[:H, :W]                                                 # crop BEFORE filtering
    feats, idxs, sharp = [], [], None
    for scale in (1, 2):
        m, sigma = mscn(y)
        if perturb is not None:
            m = m * (1.0 + perturb[1] * perturb[0].standard_normal(m.shape))
        bs = BLOCK // scale
        nby, nbx = y.shape[0] // bs, y.shape[1] // bs
        f, ix = [], []
        for by in range(nby):
            for bx in range(nbx):
                ff, ii = block_features(m[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs])
                f.append(ff)
                ix.append(ii)
        feats.append(np.array(f))
        idxs.append(np.array(ix))
        if scale == 1:
            sharp = sigma.reshape(nby, bs, nbx, bs).mean(axis=(1, 3)).ravel()
            y = 255.0 * imresize(y / 255.0, 0.5)
    return np.concatenate(feats, axis=1), sharp, np.concatenate(idxs, axis=1)


def stats(F: np.ndarray):
    """-> (nanmean [36], covariance over the NaN-free rows [36,36] (NaN for fewer than two), (NaN-free rows, rows with any value))."""
    with np.errstate(all="ignore"):
        ok = ~np.isnan(F)
        mu = np.where(ok.sum(0) > 0, np.where(ok, F, 0.0).sum(0) / ok.sum(0), np.nan)
    clean = F[ok.all(axis=1)]
    cov = np.cov(clean, rowvar=False) if clean.shape[0] >= 2 else np.full((36, 36), np.nan)
    return mu, cov, (int(clean.shape[0]), int(ok.any(axis=1).sum()))


def distance(mu_a, cov_a, mu_b, cov_b) -> float:
    pooled = (np.asarray(cov_a) + np.asarray(cov_b)) / 2
    d = np.asarray(mu_a) - np.asarray(mu_b)
    if not (np.isfinite(pooled).all() and np.isfinite(d).all()):
        return float("nan")
    return float(np.sqrt(d @ np.linalg.pinv(pooled, rcond=36 * np.finfo(np.float64).eps) @ d))


def score(mu_p, cov_p, F) -> float:
    mu, cov, _ = stats(F)
    return distance(mu_p, cov_p, mu, cov)


def fit(images, sharpness=0.75):
    """-> (mu [36], cov [36,36], the kept block indices per image)."""
    rows, kept = [], []
    for img in images:
        F, s, _ = features(img)
        keep = (s > sharpness * s.max()) & ~np.isnan(F).any(axis=1)
        rows.append(F[keep])
        kept.append(np.nonzero(keep)[0])
    rows = np.concatenate(rows)
    return rows.mean(axis=0), np.cov(rows, rowvar=False), kept


def make_image(seed: int, h: int, w: int, channels: int = 3) -> np.ndarray:
    """Seeded uint8 [h,w,channels]: a smooth ramp plus noise whose law and strength change from region to region (Gaussian, uniform,
    Laplacian; a few grey levels to tens), so that the blocks' alphas spread over the grid."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = 60.0 + 120.0 * (0.6 * xx / w + 0.4 * yy / h)
    out = np.zeros((h, w, channels))
    for c in range(channels):
        strength = 4.0 + 30.0 * (0.5 + 0.5 * np.sin(xx / 37.0 + c) * np.cos(yy / 29.0))
        kind = (np.floor(xx / 48) + np.floor(yy / 48)) % 3
        noise = np.where(kind == 0, rng.standard_normal((h, w)),
                         np.where(kind == 1, rng.uniform(-1.7, 1.7, (h, w)), rng.laplace(0.0, 0.7, (h, w))))
        out[..., c] = ramp + 10.0 * c + strength * noise
    return np.clip(np.round(out), 0, 255).astype(np.uint8)
