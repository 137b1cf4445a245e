"""float64 definitions of the T5 operators (csrc/t5.hip) and of the token and tile glue kernels of csrc/elementwise.hip, with the
magnitude `mag` the budget of tests/norm_ref.py scales with:

    |got - ref| <= 0.5 * ulp_out(ref) + k * 2^-24 * mag   (+ slack: the half ulp of an inner bf16 rounding the kernel documents)

Plain torch on the CPU; nothing here comes from emu_ops.  Where a kernel DOCUMENTS an inner rounding to bf16 (gelu before the gate,
the scores and the probabilities of the T5 attention) the definition rounds there too, from float64 and to nearest even, and says which
elements sit so close to a rounding boundary that k fp32 roundings of the operand could push them across: there either neighbour is right."""
import math

import torch

from norm_ref import F64, U24, ulp

BF = torch.bfloat16


# ---- bf16 rounding of float64 values, without a detour through fp32 (which would round twice) ---------------------------------------

def rne(x, dtype=BF):
    """x rounded to nearest even on the grid of `dtype`, as float64."""
    u = ulp(x, dtype)
    return torch.round(x / u) * u                                 # x / u is exact (u is a power of two); torch.round is half-to-even


def neighbours(x, dtype=BF):
    """(lo, hi, dist): the grid points around x (lo == hi where x is one) and |x - the rounding boundary between them| (inf on the grid)."""
    u = ulp(x, dtype)
    lo, hi = torch.floor(x / u) * u, torch.ceil(x / u) * u
    dist = torch.where(lo == hi, torch.full_like(x, math.inf), (x - 0.5 * (lo + hi)).abs())
    return lo, hi, dist


def need_k(got, ref, mag, dtype=None, slack=None):
    """norm_ref.need_k with an additive slack per element (the half ulp of a documented inner rounding)."""
    dtype = dtype or got.dtype
    excess = (got.to(F64).cpu() - ref).abs() - 0.5 * ulp(ref, dtype) - (0.0 if slack is None else slack)
    bad = ~torch.isfinite(excess)
    k = torch.where(excess > 0, excess / (U24 * mag), torch.zeros_like(excess))
    k = torch.where(bad, torch.full_like(k, math.inf), k)
    return float(k.max()) if k.numel() else 0.0


# ---- T5LayerNorm -------------------------------------------------------------------------------------------------------------------

def rmsnorm(x, w, eps):
    """y = w x / sqrt(mean(x^2) + eps), no mean subtraction, no bias; mag = |y| (a product: nothing is added to form it)."""
    from norm_ref import f32
    xd = x.to(F64)
    y = w.to(F64) * xd / torch.sqrt((xd * xd).mean(dim=1, keepdim=True) + f32(eps))
    return y, y.abs()


# ---- T5DenseGatedActDense ----------------------------------------------------------------------------------------------------------

def gelu_tanh(a):
    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))


class GatedGelu:
    """out = rne_bf16(rne_bf16(gelu_tanh(a)) b) for x = (a || b): the product of two bf16 values is exact in fp32, so the output's bits
    are a function of the ONE rounding of gelu.  An element is undecided at k when gelu64(a) lies within k 2^-24 |a| of a bf16 rounding
    boundary; there the product with either neighbour is right, elsewhere only `out`."""

    def __init__(self, x):
        Fh = x.shape[1] // 2
        xd = x.to(F64)
        self.a, self.b = xd[:, :Fh], xd[:, Fh:]
        self.g = gelu_tanh(self.a)
        lo, hi, self.dist = neighbours(self.g)
        self.out = rne(rne(self.g) * self.b)
        self.out_lo, self.out_hi = rne(lo * self.b), rne(hi * self.b)

    def need_k(self, got):
        """Smallest band half-width k (in 2^-24 |a|) at which `got` is accepted everywhere; inf: an element is neither neighbour's product."""
        gd = got.to(F64).cpu()
        k = torch.where(gd == self.out, torch.zeros_like(self.dist), self.dist / (U24 * self.a.abs()))
        k = torch.where((gd == self.out) | (gd == self.out_lo) | (gd == self.out_hi), k, torch.full_like(k, math.inf))
        return float(torch.nan_to_num(k, nan=math.inf, posinf=math.inf).max())

    def band_share(self, k):
        return float((self.dist <= k * U24 * self.a.abs()).double().mean())

    def tail(self):
        """(ref, mag, slack) where 1 + tanh cancels: gelu(a) is tiny next to a, an fp32 gelu is good to k 2^-24 |a| only, which is many
        bf16 spacings of gelu(a), so no neighbour can be named: ref = gelu64(a) b with mag = |a b|, and the documented rounding of gelu to
        bf16 is allowed its half ulp times |b|."""
        return self.g * self.b, (self.a * self.b).abs(), 0.5 * ulp(self.g, BF) * self.b.abs()


# ---- T5Attention -------------------------------------------------------------------------------------------------------------------

class AttentionBias:
    """softmax(q k^T + bias) v per head, NO 1/sqrt(d), with the roundings the kernel documents: S = rne(rne(q k^T) + rne(bias)) and
    P = rne(softmax(S)), all to bf16, everything else float64.  ref = sum_j P_j v_j, mag = sum_j P_j |v_j|.  Key j of a row is undecided
    at k when its exact probability p_j lies within k 2^-24 p_j of a bf16 rounding boundary."""

    def __init__(self, qkv, bias, heads):
        N, D = qkv.shape[0], heads * 64
        q, k, v = (qkv.to(F64)[:, i * D:(i + 1) * D].reshape(N, heads, 64).permute(1, 0, 2) for i in range(3))
        qk = torch.einsum("hqd,hkd->hqk", q, k)
        self.scores_exact = bool((rne(qk) == qk).all())
        bb = rne(bias.to(F64))
        s = rne(rne(qk) + bb)
        self.scores_exact = self.scores_exact and bool((bb == bias.to(F64)).all()) and bool((s == qk + bias.to(F64)).all())
        self.p = torch.softmax(s, dim=-1)
        self.v = v
        pb = rne(self.p)
        _, _, self.dist = neighbours(self.p)
        self.N, self.heads = N, heads
        self.ref = self._rows(torch.einsum("hqk,hkd->hqd", pb, v))
        self.mag = self._rows(torch.einsum("hqk,hkd->hqd", pb, v.abs()))

    def _rows(self, t):
        return t.permute(1, 0, 2).reshape(self.N, self.heads * 64)

    def undecided(self, k):
        return self.dist <= k * U24 * self.p

    def slack(self, k):
        """sum over the undecided keys of ulp_bf16(p_j) |v_j|."""
        w = torch.where(self.undecided(k), ulp(self.p, BF), torch.zeros_like(self.p))
        return self._rows(torch.einsum("hqk,hkd->hqd", w, self.v.abs()))

    def share(self, k):
        return float(self.undecided(k).double().mean())


def selected_rows(qkv, pi):
    """The `selection` family's answer: row i of head h is v[pi[h, i]] of that head, bit for bit."""
    heads, N = pi.shape
    v = qkv[:, 2 * heads * 64:].reshape(N, heads, 64)
    return torch.stack([v[pi[h], h] for h in range(heads)], dim=1).reshape(N, heads * 64).contiguous()


# ---- M = 1 linear ------------------------------------------------------------------------------------------------------------------

def gemv(W, bias, x, act=0):
    """y = W act(x) + b, act 1 = SiLU; mag = sum_k |W act(x)| + |b|."""
    xd = x.to(F64)
    if act == 1:
        xd = xd * torch.sigmoid(xd)
    t = W.to(F64) * xd[None, :]
    y, mag = t.sum(dim=1), t.abs().sum(dim=1)
    if bias is not None:
        y, mag = y + bias.to(F64), mag + bias.to(F64).abs()
    return y, mag


# ---- CogVideoXPatchEmbed gather ----------------------------------------------------------------------------------------------------

def patch_index(T, Cc, H, W, pt, p):
    """[tokens, features] -> flat index into [T, C, H, W]: token (it, ih, iw), feature (c, tt, ph, pw)."""
    idx = torch.arange(T * Cc * H * W).reshape(T // pt, pt, Cc, H // p, p, W // p, p)
    return idx.permute(0, 3, 5, 2, 1, 4, 6).reshape(-1, Cc * pt * p * p)


def patch_index_loops(T, Cc, H, W, pt, p):
    """The same map spelled out element by element (small shapes: the check of patch_index)."""
    rows = []
    for it in range(T // pt):
        for ih in range(H // p):
            for iw in range(W // p):
                rows.append([(((it * pt + tt) * Cc + c) * H + ih * p + ph) * W + iw * p + pw
                             for c in range(Cc) for tt in range(pt) for ph in range(p) for pw in range(p)])
    return torch.tensor(rows)


def rne_bits_bf16(x32):
    """fp32 -> bf16 bits by integer arithmetic (finite inputs): the upper half after adding 0x7fff + the kept part's last bit."""
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 32768, r - 65536, r).to(torch.int16)


# ---- diffusers blend_v / blend_h ---------------------------------------------------------------------------------------------------

def blend_edge(a, b, extent, axis):
    """b's strip [.., e, ..] = a[.., La - extent + e, ..] (1 - e / extent) + b[.., e, ..] (e / extent), e < extent, along H (axis 0) or W
    (axis 1) of [T,H,W,ld]; the rest of b unchanged.  -> (ref, mag, strip mask), mag = |a| wa + |b| wb (0 outside the strip: a copy)."""
    ax = axis + 1
    ad, bd = a.to(F64), b.to(F64)
    wb = (torch.arange(extent, dtype=F64) / extent).reshape([-1 if d == ax else 1 for d in range(4)])
    sa = ad.narrow(ax, a.shape[ax] - extent, extent)
    sb = bd.narrow(ax, 0, extent)
    ref, mag, strip = bd.clone(), torch.zeros_like(bd), torch.zeros_like(bd, dtype=torch.bool)
    ref.narrow(ax, 0, extent).copy_(sa * (1 - wb) + sb * wb)
    mag.narrow(ax, 0, extent).copy_(sa.abs() * (1 - wb) + sb.abs() * wb)
    strip.narrow(ax, 0, extent).fill_(True)
    return ref, mag, strip


# ---- tap-split conv_out, second half -----------------------------------------------------------------------------------------------

def conv_out_gather(p, Cc, bias):
    """s[t][y][x][c] = sum over the 9 taps of p[t][y+dy-1][x+dx-1][(dy*3+dx) Cc + c] (zero outside the frame) + bias[c]; channels-last
    float64 [T,H,W,Cc] BEFORE the conv's bf16 output rounding, and mag = sum |taps| + |bias|."""
    T, H, W, _ = p.shape
    pd = torch.zeros(T, H + 2, W + 2, 9 * Cc, dtype=F64)
    pd[:, 1:H + 1, 1:W + 1] = p[..., :9 * Cc].to(F64)
    s, mag = torch.zeros(T, H, W, Cc, dtype=F64), torch.zeros(T, H, W, Cc, dtype=F64)
    for dy in range(3):
        for dx in range(3):
            k = (dy * 3 + dx) * Cc
            tap = pd[:, dy:dy + H, dx:dx + W, k:k + Cc]
            s, mag = s + tap, mag + tap.abs()
    if bias is not None:
        s, mag = s + bias.to(F64), mag + bias.to(F64).abs()
    return s, mag
