"""float64 definitions of the normalisation and affine layout operators (csrc/norm.hip, csrc/elementwise.hip), and the error budget
the GPU kernels are held to.  Plain torch on the CPU; nothing here comes from emu_ops.

Every operator returns ``(ref, mag)``: the float64 result and, per element, the sum of the absolute values of the terms the definition adds
to form it.  A kernel (or an fp32 restatement) output ``got`` is accepted when, for EVERY element,

    |got - ref| <= 0.5 * ulp_out(ref) + k * 2^-24 * mag

``ulp_out`` being the spacing of the output dtype at ``ref``: the correctly rounded result, plus k fp32 roundings of the magnitudes that went
into it.  Where the output cancels to nearly nothing the second term is what keeps a rounding-level bound usable.

Scalar parameters (eps, scale, shift, clamp limits, a, b) cross the C interface as fp32: the definitions use their fp32 values."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
U24 = 2.0 ** -24
_PREC = {torch.bfloat16: 8, torch.float32: 24, torch.float64: 53}


def f32(v):
    """The value a Python float has once it went through a C ``float`` argument."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def ulp(ref, dtype):
    """Spacing of ``dtype`` at |ref| (the subnormal spacing below the smallest normal)."""
    _, e = torch.frexp(ref.abs().to(F64))                       # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, -126), e - 1).clamp_min(-126)
    return torch.ldexp(torch.ones_like(ref, dtype=F64), e - (_PREC[dtype] - 1))


def need_k(got, ref, mag, dtype=None):
    """Smallest k at which every element of ``got`` meets the budget (inf: an element misses it where mag is 0)."""
    dtype = dtype or got.dtype
    excess = (got.to(F64).cpu() - ref).abs() - 0.5 * ulp(ref, dtype)
    bad = ~torch.isfinite(excess)
    k = torch.where(excess > 0, excess / (U24 * mag), torch.zeros_like(excess))          # x / 0 = inf
    k = torch.where(bad, torch.full_like(k, math.inf), k)
    return float(k.max()) if k.numel() else 0.0


def within(got, ref, mag, k, dtype=None):
    return need_k(got, ref, mag, dtype) <= k


def ulps_off(got, ref, dtype=None):
    """max |got - ref| in units of the output spacing at ref (entry points that start from given sums: both sides are fp64)."""
    dtype = dtype or got.dtype
    return float(((got.to(F64).cpu() - ref).abs() / ulp(ref, dtype)).max())


# ---- GroupNorm(32) statistics --------------------------------------------------------------------------------------------------

def _groups(x, nb):
    Cc = x.shape[-1]
    return x.to(F64).reshape(nb, -1, 32, Cc // 32)


def gn_stats(x, eps, nb=1):
    """(mean, rstd) per instance and group of x [nb*T,H,W,C] or [N,C]: ([nb,32,2] | [32,2], mag).  Two passes.  mag is the absolute
    condition of each output against fp32 roundings of the summed terms: E|x| for the mean, kappa_rstd * rstd for rstd with
    kappa_rstd = (E[x^2] + 2 |mean| E|x|) / (2 (var + eps))."""
    eps = f32(eps)
    xg = _groups(x, nb)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    ea, e2 = xg.abs().mean(dim=(1, 3)), (xg * xg).mean(dim=(1, 3))
    kap = (e2 + 2 * mean.abs() * ea) / (2 * (var + eps))
    st, mag = torch.stack([mean, rstd], dim=-1), torch.stack([ea, kap * rstd], dim=-1)
    return (st[0], mag[0]) if nb == 1 else (st, mag)


def gn_sums(x):
    """Raw (sum, sum of squares) per group, [32,2]; mag = (sum |x|, sum x^2)."""
    xg = _groups(x, 1)[0]
    return (torch.stack([xg.sum(dim=(0, 2)), (xg * xg).sum(dim=(0, 2))], dim=1),
            torch.stack([xg.abs().sum(dim=(0, 2)), (xg * xg).sum(dim=(0, 2))], dim=1))


def gn_from_sums(sums, count, eps):
    """(mean, rstd) [..,32,2] from fp64 (sum, sumsq) [..,32,2] over ``count`` elements; ``count=None``: the 65-double message whose last
    entry is the count.  Starts from given sums, so there is nothing to condition on: mag is 0 and the bound is output rounding."""
    sums = sums.to(F64)
    if count is None:
        count, sums = float(sums.reshape(-1)[64]), sums.reshape(-1)[:64].reshape(32, 2)
    mean = sums[..., 0] / count
    var = (sums[..., 1] / count - mean * mean).clamp_min(0)
    st = torch.stack([mean, 1.0 / torch.sqrt(var + f32(eps))], dim=-1)
    return st, torch.zeros_like(st)


def gn_from_partials(rows, nb, count, eps):
    """Statistics [nb,32,2] (nb = 1: [32,2]) from fp32 partial rows [nb*rows, 64] = (sum, sumsq) x 32 groups, summed in fp64."""
    s = rows.to(F64).reshape(nb, -1, 32, 2).sum(dim=1)
    st, mag = gn_from_sums(s, count, eps)
    return (st[0], mag[0]) if nb == 1 else (st, mag)


def sums_from_partials(rows):
    s = rows.to(F64).reshape(-1, 32, 2).sum(dim=0)
    return s, torch.zeros_like(s)


# ---- GroupNorm / SpatialNorm apply ---------------------------------------------------------------------------------------------

def silu_with_mag(p, mag_p):
    """silu(p) and its magnitude |silu'(p)| mag_p + (1 + |p|) |silu(p)|: the input's error through the slope, and the exponent's own
    rounding (an fp32 exponential of p is only good to about |p| roundings)."""
    sg = torch.sigmoid(p)
    y = p * sg
    return y, (sg * (1 + p * (1 - sg))).abs() * mag_p + (1 + p.abs()) * y.abs()


def gn_preact(x, stats, gamma, beta, yb=None, Tz=0, sshift=0, tmap=None, nb=1):
    """The value before the activation, and its mag: p = x sc - mean sc + beta with sc = rstd gamma, then p Y + B with
    Y, B = yb[b Tz + tmap[t]][h >> sshift][w >> sshift][c], [C + c]."""
    TT, H, W, Cc = x.shape
    T, cpg = TT // nb, Cc // 32
    st = stats.to(F64).reshape(nb, 32, 2)
    mean = st[:, :, 0].repeat_interleave(cpg, dim=1)[:, None, None, None, :]
    sc = (st[:, :, 1].repeat_interleave(cpg, dim=1) * gamma.to(F64))[:, None, None, None, :]
    xs = x.to(F64).reshape(nb, T, H, W, Cc) * sc
    ms = mean * sc
    p = xs - ms + beta.to(F64)
    mag = xs.abs() + ms.abs() + beta.to(F64).abs()
    if yb is not None:
        assert len(tmap) == T and yb.shape[0] == nb * Tz
        tz = (torch.arange(nb)[:, None] * Tz + torch.tensor(list(tmap), dtype=torch.long)[None, :]).reshape(-1)
        hi, wi = torch.arange(H) >> sshift, torch.arange(W) >> sshift
        g = yb[tz][:, hi][:, :, wi].to(F64).reshape(nb, T, H, W, 2 * Cc)
        Y, B = g[..., :Cc], g[..., Cc:]
        p = p * Y + B
        mag = mag * Y.abs() + B.abs()
    return p.reshape(TT, H, W, Cc), mag.reshape(TT, H, W, Cc)


def gn_apply(x, stats, gamma, beta, silu=True, yb=None, Tz=0, sshift=0, tmap=None, nb=1):
    p, mag = gn_preact(x, stats, gamma, beta, yb, Tz, sshift, tmap, nb)
    return silu_with_mag(p, mag) if silu else (p, mag)


# ---- LayerNorm + AdaLN modulation ----------------------------------------------------------------------------------------------

def ln_affine(N, gamma, beta, mod=None, split=0):
    """Per row: A = gamma (1 + scale), B = beta (1 + scale) + shift with (shift, scale) = mod[row >= split], and B's own mag
    |beta (1 + scale)| + |shift| (the two terms that are added to form it)."""
    D = gamma.shape[0]
    A, B = gamma.to(F64).expand(N, D), beta.to(F64).expand(N, D)
    magB = B.abs()
    if mod is not None:
        m = mod.to(F64)[(torch.arange(N) >= split).long()]          # [N, 2 (shift, scale), D]
        A, B, magB = A * (1 + m[:, 1]), B * (1 + m[:, 1]) + m[:, 0], (B * (1 + m[:, 1])).abs() + m[:, 0].abs()
    return A, B, magB


def ln_mod(x, gamma, beta, eps, mod=None, split=0):
    """y = (x - mean) rstd A + B per row (ln_affine); mag = (|x| + |mean|) rstd |A| + |beta (1 + scale)| + |shift|: every term that is
    added, B's two included (they cancel where scale is near -1 or shift opposes beta)."""
    xd = x.to(F64)
    N, D = xd.shape
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    A, B, magB = ln_affine(N, gamma, beta, mod, split)
    return (xd - mean) * rstd * A + B, (xd.abs() + mean.abs()) * rstd * A.abs() + magB


def ln_constant_rows(x, gamma, beta, mod=None, split=0):
    """Rows whose elements are all equal: var = 0 and x - mean = 0 whatever eps is, so the output is B and nothing but B's own two terms
    may round: (B, |beta (1 + scale)| + |shift|).  An fp32 mean of D equal bf16 values is exact (D <= 4096 times 8 significant bits),
    so a kernel has no (x - mean) rstd residue to hide behind; rstd = eps^-1/2 multiplies an exact zero."""
    xd = x.to(F64)
    assert bool((xd == xd[:, :1]).all())
    _, B, magB = ln_affine(xd.shape[0], gamma, beta, mod, split)
    return B, magB


# ---- affine layout kernels: y = x scale + shift, mag = |x scale| + |shift| (0 where the definition puts an exact zero) ----------

def _affine(x, scale, shift):
    xs = x.to(F64) * f32(scale)
    return xs + f32(shift), xs.abs() + abs(f32(shift))


def cl_from_ncthw(x, cp, scale=1.0, shift=0.0):
    Cc, T, H, W = x.shape
    v, m = _affine(x, scale, shift)
    y, mag = torch.zeros(T, H, W, cp, dtype=F64), torch.zeros(T, H, W, cp, dtype=F64)
    y[..., :Cc], mag[..., :Cc] = v.permute(1, 2, 3, 0), m.permute(1, 2, 3, 0)
    return y, mag


def cl_im2col3x3_from_ncthw(x, cp, scale=1.0, shift=0.0):
    """y[t][h][w][(dy*3+dx)*C + c] = (x scale + shift)[c][t][h+dy-1][w+dx-1], zero outside the frame and beyond 9C."""
    Cc, T, H, W = x.shape
    v, m = _affine(x, scale, shift)
    y, mag = torch.zeros(T, H, W, cp, dtype=F64), torch.zeros(T, H, W, cp, dtype=F64)
    vp, mp = F.pad(v, (1, 1, 1, 1)), F.pad(m, (1, 1, 1, 1))     # the zero border is part of the definition (after the affine map)
    for dy in range(3):
        for dx in range(3):
            k = (dy * 3 + dx) * Cc
            y[..., k:k + Cc] = vp[:, :, dy:dy + H, dx:dx + W].permute(1, 2, 3, 0)
            mag[..., k:k + Cc] = mp[:, :, dy:dy + H, dx:dx + W].permute(1, 2, 3, 0)
    return y, mag


def ncthw_from_cl(x, Cc, scale=1.0, shift=0.0, lo=-math.inf, hi=math.inf):
    v, m = _affine(x[..., :Cc], scale, shift)
    return v.clamp(f32(lo), f32(hi)).permute(3, 0, 1, 2).contiguous(), m.permute(3, 0, 1, 2).contiguous()


def avgpool_time(x, nb=1):
    """Per instance: odd T keeps frame 0 and averages (1,2), (3,4), ..; even T averages (0,1), (2,3), .."""
    xs = x.to(F64).reshape(nb, x.shape[0] // nb, *x.shape[1:])
    T = xs.shape[1]
    a, b = (xs[:, 1::2], xs[:, 2::2]) if T % 2 else (xs[:, 0::2], xs[:, 1::2])
    y, mag = 0.5 * a + 0.5 * b, 0.5 * a.abs() + 0.5 * b.abs()
    if T % 2:
        y, mag = torch.cat([xs[:, :1], y], dim=1), torch.cat([torch.zeros_like(xs[:, :1]), mag], dim=1)   # a copy: exact
    return y.reshape(-1, *x.shape[1:]), mag.reshape(-1, *x.shape[1:])


def axpby(x, y, a, b):
    ax, by = f32(a) * x.to(F64), f32(b) * y.to(F64)
    return ax + by, ax.abs() + by.abs()


def posterior_sample(moments_cl, latent_channels, noise):
    """mean + exp(0.5 clamp(logvar, -30, 20)) noise, [L,T,h,w].  mag = |mean| + (1 + |p|) |exp(p) noise|, p = 0.5 logvar: the exponential's
    term carries the same (1 + |p|) as SiLU's."""
    L = latent_channels
    m = moments_cl.to(F64)
    mean, p = m[..., :L].permute(3, 0, 1, 2), 0.5 * m[..., L:2 * L].permute(3, 0, 1, 2).clamp(-30.0, 20.0)
    t = torch.exp(p) * noise.to(F64)
    return mean + t, mean.abs() + (1 + p.abs()) * t.abs()


# ---- what the CPU check compares the definitions with -------------------------------------------------------------------------

def torch_group_norm(x, eps, gamma, beta):
    """F.group_norm in float64 on x [T,H,W,C] (one instance), channels-last in and out."""
    Cc = x.shape[-1]
    xn = x.to(F64).reshape(-1, Cc).T.reshape(1, Cc, -1)
    return F.group_norm(xn, 32, gamma.to(F64), beta.to(F64), f32(eps)).reshape(Cc, -1).T.reshape(x.shape)
