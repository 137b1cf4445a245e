"""The case table of the T5 operators (csrc/t5.hip: rmsnorm, gated_gelu, attention_bias) and of the token and tile glue kernels of
csrc/elementwise.hip that the norm / layout net did not reach (gemv, patchify / unpatchify, blend_edge, conv_out_gather[_cl], tile_gather),
shared by tests/test_glue_ref_cpu.py (which measures what the fp32 restatements of tests/emu_ops.py need against tests/glue_ref.py and
proves that the table reaches every branch of the kernels) and tests/test_glue_fp64_gpu.py (which holds the kernels to the same budget).
Shapes are the smallest at which each branch is live; every input is seeded, so both files see the same values.  Imports no GPU."""
import math

import torch

from norm_cases import _gen

BF = torch.bfloat16


def _rand(shape, g):
    return torch.rand(*shape, generator=g)


# ---- rmsnorm: one wave a row, lane l owns the 8 columns (i * 64 + l) * 8 of iteration i < NIT = ceil(D / 512) -------------------------
# 8 .. 4096 as the operator's brief lists them, plus 1536, 2040, 2552, 3064, 3584 so that EVERY NIT has a full and a ragged last iteration
RMS_D = (8, 504, 512, 520, 1024, 1528, 1536, 2040, 2048, 2552, 2560, 3064, 3072, 3576, 3584, 4088, 4096)
RMS_ROWS = (1, 3, 4, 5, 226)                                     # 4 rows a block: one partial block, exactly one, one + 1, 57 blocks
RMS_FAMILIES = ("gaussian3", "spike", "constant", "tiny")
RMS_EPS = 1e-6
RMS_SINGLE_ROWS = (0, 3, 4, 225)                                 # rows of the 226-row call that are recomputed in a 1-row call


def rms_nit(D):
    """(NIT, lanes live in the last iteration): 64 = a full last iteration."""
    nit = (D // 8 + 63) // 64
    return nit, D // 8 - (nit - 1) * 64


def rms_input(family, rows, D):
    g = _gen("rms", family, rows, D)
    r = torch.randn(rows, D, generator=g)
    if family == "gaussian3":
        x = 3.0 * r
    elif family == "spike":                                      # one 1e3 among 1e-2: the spike is the whole mean square; row 0's is the
        x = 1e-2 * r                                             # LAST column (the ragged iteration's last live lane)
        pos = (torch.arange(rows) * 37 + D - 1) % D
        x[torch.arange(rows), pos] = 1e3 * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)
    elif family == "constant":                                   # every element equal: y = w sign(x) up to eps
        c = 1.7 * torch.randn(rows, 1, generator=g) + 0.9
        x = torch.where(c.abs() < 0.05, torch.full_like(c, 0.3), c).to(BF).float().expand(rows, D)
    elif family == "tiny":                                       # mean square ~ 1e-8 against eps = 1e-6: a wrong eps is a first-order error
        x = 1e-4 * r
    else:
        raise KeyError(family)
    return x.to(BF).contiguous()


def rms_weight(D):
    return 1 + 0.5 * torch.randn(D, generator=_gen("rmsw", D))


# ---- gated_gelu: one thread per 8 outputs, row = t / (F / 8) -----------------------------------------------------------------------
GG_F = (8, 16, 1024, 10240)
GG_M = (1, 3, 226)
GG_FAMILIES = ("main", "tail")
GG_BAND_CAP = 0.01                                                # the share of `main` elements whose bf16 rounding of gelu is undecided
TINY = 1e-30


def gg_input(family, M, F):
    """x [M, 2F] bf16 = (a || b).  main: a in [-3, 12] with 0, +-tiny and both ends; tail: a in [-12, -3] (1 + tanh cancels)."""
    g = _gen("gg", family, M, F)
    u = _rand((M, F), g)
    if family == "main":
        a = -3.0 + 15.0 * u
        a.view(-1)[:5] = torch.tensor([0.0, TINY, -TINY, -3.0, 12.0])
    elif family == "tail":
        a = -12.0 + 9.0 * u
        a.view(-1)[:2] = torch.tensor([-12.0, -3.0])
    else:
        raise KeyError(family)
    b = 1.5 * torch.randn(M, F, generator=g)
    return torch.cat([a, b], dim=1).to(BF).contiguous()


# ---- attention_bias: one wave per (query, head), lanes own keys lane, lane + 64, ..; 4 queries a block ---------------------------------
ATT_CASES = [(N, h) for N in (1, 2, 63, 64, 65, 128, 226, 1024) for h in (1, 3)] + [(226, 64)]
ATT_FAMILIES = ("selection", "uniform", "exact")
ATT_B_CAP = 0.01                                                  # the share of keys whose bf16 rounding of P is undecided (`exact`)
SELECT_BIAS = 40.0                                                # exp(-40) = 4e-18: the other keys' weights vanish below fp32


def att_perm(N, heads):
    """pi [heads, N]: per head its own permutation of the keys, so every key (0, N - 1, lanes 63 / 64 / 65) is selected once a head."""
    g = _gen("attperm", N, heads)
    return torch.stack([torch.randperm(N, generator=g) for _ in range(heads)])


def att_input(family, N, heads):
    """(qkv [N, 3 heads 64] bf16, bias [heads, N, N] fp32)."""
    g = _gen("att", family, N, heads)
    D = heads * 64
    if family in ("selection", "uniform"):
        q = torch.zeros(N, D)
        k = torch.randn(N, D, generator=g)                        # q = 0: whatever k holds, every score is 0
        sign = torch.where(_rand((N, D), g) < 0.5, -1.0, 1.0)
        v = sign * (0.25 + 3.75 * _rand((N, D), g))               # no v near 0: v[pi(i)] dwarfs the 4e-18 weights of the others
        bias = torch.zeros(heads, N, N)
        if family == "selection":
            bias.scatter_(2, att_perm(N, heads)[:, :, None], SELECT_BIAS)
    elif family == "exact":                                       # q k^T = m / 8, |m| <= 64; bias = m' / 8, |m'| <= 32: exact in bf16, and the sum too
        q = torch.randint(-1, 2, (N, D), generator=g).float()
        k = torch.randint(-1, 2, (N, D), generator=g).float() / 8
        v = 1.5 * torch.randn(N, D, generator=g)
        bias = torch.randint(-32, 33, (heads, N, N), generator=g).float() / 8
    else:
        raise KeyError(family)
    return torch.cat([q, k, v], dim=1).to(BF).contiguous(), bias.contiguous()


# ---- gemv: one wave per output row, 4 rows a block; a lane takes 8 inputs of every 512 --------------------------------------------------
GEMV_IN = (8, 504, 512, 520, 3072)                                # 1 lane; 63 lanes; one full trip; one full + 1 lane; 6 full trips
GEMV_OUT = (1, 3, 4, 5, 701)                                      # out % 4 = 1, 3, 0, 1 (two blocks), 1 (176 blocks)


def gemv_input(in_f, out_f):
    g = _gen("gemv", in_f, out_f)
    return (torch.randn(out_f, in_f, generator=g).to(BF), torch.randn(out_f, generator=g), 1.5 * torch.randn(in_f, generator=g))


# ---- patchify / unpatchify: (pt, p, C, T, H, W, ld - features) ---------------------------------------------------------------------
PATCH_CASES = [
    (1, 1, 1, 1, 1, 3, 0),                                        # 3 elements, 1 feature
    (1, 1, 16, 2, 3, 5, 0),
    (1, 2, 1, 3, 4, 6, 8),
    (1, 2, 16, 1, 6, 10, 0),
    (2, 2, 1, 2, 2, 6, 1),                                        # an odd ld
    (2, 2, 16, 2, 6, 10, 0),                                      # the product's 16 * 2 * 2 * 2 = 128 features; 1920 elements = 7.5 blocks
    (2, 2, 16, 4, 10, 6, 8),                                      # 3840 elements = exactly 15 blocks, ld 136
]


def finite_bf16_patterns(n, *key):
    """n DISTINCT finite bf16 bit patterns (subnormals and both zeros included) as a bf16 tensor: a misplaced element shows."""
    v = torch.arange(65536)
    v = v[((v >> 7) & 0xFF) != 0xFF]
    assert n <= v.numel()
    v = v[torch.randperm(v.numel(), generator=_gen("bits", n, *key))[:n]]
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(BF)


def widen_with_low_bits(x):
    """fp32 whose upper half is x's bits and whose lower half runs through the rounding classes: 0, below / at / above the tie."""
    lows = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x8000, 0x1234])
    hi = x.contiguous().view(torch.int16).to(torch.int32) << 16
    low = lows[torch.arange(x.numel()) % lows.numel()].reshape(x.shape).to(torch.int32)
    return (hi | low).view(torch.float32)


# ---- blend_edge: (axis, T, (Ha, Wa), (Hb, Wb), ld); the blended axis differs between a and b, in both orders --------------------------
BLEND_CASES = [
    (0, 1, (5, 5), (3, 5), 4),                                    # extent 1: 5 granules in all
    (0, 3, (3, 7), (6, 7), 8),
    (0, 1, (4, 33), (9, 33), 32),                                 # 1056 granules at extent 4: five blocks, the last partial
    (1, 1, (5, 6), (5, 3), 4),
    (1, 3, (4, 3), (4, 7), 8),
    (1, 1, (9, 4), (9, 11), 32),
]


def blend_extents(case):
    axis, T, sa, sb, ld = case
    return sorted({1, 2, min(sa[axis], sb[axis])})


def blend_input(case):
    axis, T, sa, sb, ld = case
    g = _gen("blend", *case)
    return (1.7 * torch.randn(T, *sa, ld, generator=g) + 0.2).to(BF), (1.7 * torch.randn(T, *sb, ld, generator=g) - 0.4).to(BF)


# ---- conv_out_gather / conv_out_gather_cl: 8 x 64 pixels a block, records of ldp floats (+1 pad) in LDS ---------------------------------
COG_CLDP = [(1, 12), (1, 36), (2, 20), (3, 28), (3, 32), (4, 36)]  # ldp = 36 alone needs the raised dynamic-LDS limit (97 680 bytes)
COG_HW = [(1, 1), (7, 63), (8, 64), (9, 65), (17, 130)]            # below / at / above one block in both directions; 3 x 3 blocks
COG_T = (1, 2)
COG_LDY = (4, 8, 32)
COG_FAMILIES = ("grid", "gaussian")


def cog_input(family, Cc, ldp, T, H, W):
    """(p [T,H,W,ldp] fp32 partial planes, bias [Cc] fp32).  grid: multiples of 2^-6 in [-2, 2], so the 9 taps + bias sum exactly in
    fp32.  The planes beyond 9 Cc are NaN: the kernel stages them but must never add them."""
    g = _gen("cog", family, Cc, ldp, T, H, W)
    if family == "grid":
        p = torch.randint(-128, 129, (T, H, W, ldp), generator=g).float() / 64
        bias = torch.randint(-128, 129, (Cc,), generator=g).float() / 64
    else:
        p = torch.randn(T, H, W, ldp, generator=g)
        bias = torch.randn(Cc, generator=g)
    p[..., 9 * Cc:] = float("nan")
    return p.contiguous(), bias


# ---- tile_gather: the grid is capped at 8192 blocks of 256 chunks; above that a thread walks more than one chunk ------------------------
TG_GRID_CAP = 256 * 8192
TG_BIG = dict(T=3, H=136, W=200, C=32, t0=1, nt=2, th=136, tw=128, nb=16)     # th == H; 16 * 2 * 136 * 128 * 4 chunks
TG_SMALL = dict(T=2, H=9, W=70, C=32, t0=0, nt=2, th=9, tw=6)                  # nb = 64 passes, 65 is refused


def tg_chunks(c):
    return c["nb"] * c["nt"] * c["th"] * c["tw"] * (c["C"] // 8)


def tg_origins(c, nb):
    """nb tile origins, left edge, right edge and in between (repeats allowed); th == H leaves oy = 0."""
    g = _gen("tg", nb, c["th"], c["tw"])
    oy = torch.randint(0, c["H"] - c["th"] + 1, (nb,), generator=g)
    ox = torch.randint(0, c["W"] - c["tw"] + 1, (nb,), generator=g)
    ox[0], ox[-1] = 0, c["W"] - c["tw"]
    return [(int(a), int(b)) for a, b in zip(oy, ox)]


def tg_source(c, cin):
    """The clip [cin, T, H, W] bf16 whose im2col (Cp = C) the tiles are cut from."""
    return (1.7 * torch.randn(cin, c["T"], c["H"], c["W"], generator=_gen("tgsrc", c["H"], c["W"])) + 0.2).to(BF)


# ---- the budget: k fixed from what an fp32 restatement of the same operator needs ------------------------------------------------------
# K_EMU is measured by tests/test_glue_ref_cpu.py (asserted there as an upper bound on every case of this table, so that it cannot rot);
# a kernel is allowed max(4, 8 K_EMU): it sums in another order, uses the 1-ulp hardware rsqrt / rcp / exp2 and may contract a*b+c.
K_EMU = {
    "rmsnorm": 2.94,
    "gated_gelu": 0.06,        # the half-width of the band around a bf16 boundary of gelu(a), in 2^-24 |a|
    "gated_gelu_tail": 0.5,
    "attention_uniform": 0.0,  # P = rne(1 / N) for every key: the restatement is correctly rounded
    "attention_exact": 1.67,
    "gemv": 1.66,
    "gemv_silu": 1.89,
    "blend_edge": 0.01,        # two products and one sum under a bf16 rounding: all but correctly rounded
    "conv_out_gather": 0.96,
}


def allowed_k(op):
    return max(4.0, 8.0 * K_EMU[op])


assert all(math.isfinite(v) for v in K_EMU.values())
