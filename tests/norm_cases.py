"""The case table of the normalisation family (csrc/norm.hip) and the affine layout kernels (csrc/elementwise.hip), shared by
tests/test_norm_ref_cpu.py (which measures what an fp32 restatement needs against tests/norm_ref.py, and proves that wrong restatements
fail) and tests/test_norm_fp64_gpu.py (which holds the kernels to the same budget).  Shapes are the smallest at which each branch of the
kernels is live; every input is seeded, so both files see the same values."""
import math

import torch

BF = torch.bfloat16
FAMILIES = ("plain", "offset", "tiny", "group-scaled")
LN_FAMILIES = FAMILIES + ("constant-rows",)


def _gen(*key):
    return torch.Generator().manual_seed(hash_key(*key))


def hash_key(*key):
    """A seed from a tuple of ints / strings that does not depend on PYTHONHASHSEED."""
    h = 1469598103934665603
    for part in key:
        for ch in str(part) + "|":
            h = ((h ^ ord(ch)) * 1099511628211) % (1 << 63)
    return h


def family_input(family, shape, *key):
    """bf16 input of `shape` ([..., C], groups = 32 runs of C/32 channels; for C < 32 every channel is its own "group")."""
    g = _gen(family, *key)
    Cc = shape[-1]
    r = torch.randn(*shape, generator=g)
    if family == "plain":
        x = 1.7 * r + 0.9
    elif family == "offset":                                    # kappa ~ 1600: a one-pass or fp32 combine shows
        x = r + 40.0
    elif family == "tiny":                                      # var ~ eps: a wrong eps is a first-order error
        x = 2.0 ** -9 * r
    elif family == "group-scaled":                              # an index slip moves the answer by far more than a rounding
        grp = torch.arange(Cc) * 32 // max(Cc, 32) if Cc >= 32 else torch.arange(Cc)
        x = r * torch.exp2((grp % 8 - 4).float()) + grp.float() / 8
    elif family == "constant-rows":                             # LayerNorm only: var = 0, the output is exactly B rounded
        x = (1.7 * torch.randn(*shape[:-1], 1, generator=g) + 0.9).to(BF).float().expand(*shape)
    else:
        raise KeyError(family)
    return x.to(BF).contiguous()


def channel_params(Cc, *key):
    """gamma, beta fp32, distinct per channel (not smooth)."""
    g = _gen("params", Cc, *key)
    return 1 + 0.5 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)


def yb_table(shape, *key):
    """SpatialNorm table [nb*Tz, hz, wz, 2C] bf16: scale around 1, shift around 0."""
    g = _gen("yb", *key)
    Cc = shape[-1] // 2
    t = torch.randn(*shape, generator=g) * 0.5
    t[..., :Cc] += 1.0
    return t.to(BF)


def mod_table(D, *key):
    """AdaLN (shift, scale) for the two row classes, [2, 2, D] fp32; the classes differ by far more than a rounding."""
    g = _gen("mod", D, *key)
    return 0.3 * torch.randn(2, 2, D, generator=g) + torch.tensor([0.0, 0.7])[:, None, None]


# ---- GroupNorm statistics: (name, C, shape of x, nb) ------------------------------------------------------------------------------
STATS_CASES = [
    ("c32_15pix", 32, (2, 3, 5, 32), 1),            # 15 pixels a frame < 64 pixel lanes; cpg = 1
    ("c64_2blocks", 64, (1, 40, 40, 64), 1),        # 2 blocks a frame, the second ragged
    ("c128", 128, (3, 20, 24, 128), 1),
    ("c512_cpg16", 512, (3, 6, 5, 512), 1),
    ("c1024_cap256", 1024, (1, 129, 128, 1024), 1),  # nsub = 2; 258 wanted blocks capped at 256: uneven trip counts
    ("c2048", 2048, (2, 7, 9, 2048), 1),            # nsub = 1, chan[] full
    ("c256_2d", 256, (1000, 256), 1),               # frame_pix = 0
    ("c128_nb3", 128, (6, 9, 13, 128), 3),          # every instance from another family
]


def stats_input(case, family):
    name, Cc, shape, nb = case
    if nb == 1:
        return family_input(family, shape, name)
    per = (shape[0] // nb,) + tuple(shape[1:])
    first = FAMILIES.index(family)
    return torch.cat([family_input(FAMILIES[(first + i) % len(FAMILIES)], per, name, i) for i in range(nb)], dim=0)


def blocks_per_frame(frame_pix, Cc):
    """gn_partial_launch's grid: (pixel lanes, blocks per frame)."""
    nsub = 256 // (Cc // 8)
    return nsub, min(256, -(-frame_pix // (nsub * 32)))


# ---- finalize_partials[_nb] / sums_from_partials on synthetic fp32 rows ------------------------------------------------------------
PARTIAL_ROWS = (1, 2, 5, 1023, 1024, 1025, 4099)
PARTIAL_NB = (1, 3)


def partial_rows(rows, nb):
    """([nb*rows, 64] fp32 (sum, sumsq) x 32 groups, count): row r of an instance stands for 64 * 2^(7 r mod 21) elements of mean m and
    variance v, so magnitudes span 2^0 .. 2^20 (an fp32 combine loses them) and var / mean^2 is about 1 (an fp64 reordering stays at
    1e-16).  Every instance has the same count and its own values."""
    g = _gen("rows", rows, nb)
    n = 64.0 * torch.exp2(((torch.arange(rows) * 7) % 21).double()).repeat(nb)[:, None]
    m = 0.5 + 0.3 * torch.randn(nb * rows, 32, generator=g, dtype=torch.float64) + torch.arange(32) / 16
    v = 1.0 + torch.rand(nb * rows, 32, generator=g, dtype=torch.float64)
    out = torch.stack([n * m, n * (m * m + v)], dim=2).reshape(nb * rows, 64).float()
    return out, float(n[:rows].sum())


# ---- GroupNorm / SpatialNorm apply: (name, C, nb, (T, H, W), yb (Tz, hz, wz) | None, sshift, tmap | None) --------------------------
def nearest_tmap(T, Tz):
    return [t * Tz // T for t in range(T)]


def _wild_tmap(T, Tz):
    g = _gen("tmap", T, Tz)
    return [4, 0, 0, 3] + [int(v) for v in torch.randint(0, Tz, (T - 4,), generator=g)]


APPLY_CASES = [
    ("h4100", 32, 1, (1, 4100, 1), None, 0, None),                                 # H > 4096: rows grid-stride
    ("w257_nsub64", 32, 1, (2, 3, 257), None, 0, None),                            # second W trip with one live slot
    ("c2048_tail", 2048, 1, (1, 2, 5), (1, 1, 2), 2, [0]),                         # nsub = 1, 4-unroll tail, H and W ragged
    ("c128_ragged4", 128, 1, (5, 13, 21), (3, 4, 6), 2, nearest_tmap(5, 3)),
    ("c256_ragged2", 256, 1, (4, 5, 9), (2, 3, 5), 1, nearest_tmap(4, 2)),
    ("c128_sshift8", 128, 1, (2, 200, 300), (2, 1, 2), 8, [0, 1]),
    ("c64_t32_wild", 64, 1, (32, 3, 3), (5, 3, 3), 0, _wild_tmap(32, 5)),           # the tmap[32] limit, non-monotone repeats
    ("c128_nb3", 128, 3, (3, 6, 10), (2, 2, 3), 2, [1, 0, 1]),                      # per-instance statistics and yb block
]


def apply_input(case, family):
    name, Cc, nb, (T, H, W), ybs, sshift, tmap = case
    x = stats_input((name, Cc, (nb * T, H, W, Cc), nb), family)
    gamma, beta = channel_params(Cc, name)
    yb = None if ybs is None else yb_table((nb * ybs[0], ybs[1], ybs[2], 2 * Cc), name)
    return x, gamma, beta, yb


# ---- LayerNorm + modulation --------------------------------------------------------------------------------------------------------
LN_CASES = [(3, 8), (33, 520), (41, 1544), (70, 3072), (9, 3080), (5, 4096), (64, 512)]
LN_EPS = (1e-5, 1e-6)


def ln_splits(N):
    return sorted({0, 1, N // 4, N - 1, N, N + 5})


def ln_input(N, D, family):
    x = family_input(family, (N, D), "ln", N, D)
    gamma, beta = channel_params(D, "ln", N)
    return x, gamma, beta, mod_table(D, N)


# ---- layout kernels ----------------------------------------------------------------------------------------------------------------
# cl_from_ncthw: (C, Cp, (T, H, W)); npix = 1, 255, 257; Cp with and without padding
CL_CASES = [(1, 8, (1, 1, 1)), (3, 8, (1, 15, 17)), (5, 16, (1, 1, 257)), (16, 16, (3, 5, 17)), (16, 32, (1, 1, 257)), (8, 8, (1, 1, 1))]
# ncthw_from_cl: (C, ld, (T, H, W))
NCTHW_CASES = [(1, 4, (1, 1, 1)), (3, 4, (1, 15, 17)), (5, 8, (1, 1, 257)), (16, 16, (3, 5, 17)), (16, 32, (1, 1, 257)), (3, 32, (1, 1, 1))]
AFFINE = [(1.0, 0.0), (0.5, 0.5), (1.7, -0.3), (127.5, 127.5)]
CLAMP = (-0.75, 1.25)                                             # bites on both sides of 1.7 randn
# cl_im2col3x3_from_ncthw: (C, Cp, (T, H, W)); H or W of 1 and 2: every tap crosses a border; Cp > 9C
IM2COL_CASES = [(3, 32, (2, 1, 7)), (3, 32, (1, 6, 1)), (3, 32, (1, 2, 2)), (1, 16, (1, 2, 5)), (5, 48, (1, 3, 4)), (3, 40, (2, 17, 16))]
# avgpool_time: (T, nb, frame elements)
POOL_CASES = [(T, nb, fe) for T in (2, 3, 8, 9) for nb in (1, 3) for fe in (8, 8 * 257)]
AXPBY_CASES = [(n, dt) for n in (1, 257) for dt in (torch.float32, BF)]
AXPBY_COEF = [(1.0, 0.0), (0.6, -0.8), (1.0, 1.0)]


def layout_input(shape, dtype, *key):
    return (1.7 * torch.randn(*shape, generator=_gen("layout", *key)) + 0.2).to(dtype)


def posterior_input(L=16, T=2, h=3, w=43, ld=32):
    """moments [T,h,w,ld] bf16 whose log-variance runs past both clamps (-30, 20), noise [L,T,h,w] fp32."""
    g = _gen("posterior")
    m = torch.randn(T, h, w, ld, generator=g)
    m[..., L:2 * L] = m[..., L:2 * L] * 14.0 - 3.0
    m[0, 0, 0, L:2 * L] = torch.linspace(-45.0, 33.0, L)
    return m.to(BF), torch.randn(L, T, h, w, generator=g)


# ---- the budget: k (outputs) and c (statistics), fixed from what an fp32 restatement of the same operator needs --------------------
# K_EMU / C_EMU are measured by tests/test_norm_ref_cpu.py (asserted there as upper bounds on every case of this table, so that they
# cannot rot); a kernel is allowed max(4, 8 K_EMU) and 4 C_EMU: it sums in another order, uses the 1-ulp hardware rsqrt / rcp / exp2 and
# may contract a*b+c, each a few fp32 roundings.
K_EMU = {
    "ln_mod": 2.02,
    "ln_constant_rows": 0.0,   # rows of equal elements against B alone (norm_ref.ln_constant_rows): emu_ops is correctly rounded there
    "gn_apply": 1.5,
    "gn_apply_silu": 0.95,
    "sn_apply": 1.71,
    "sn_apply_silu": 0.87,
    "cl_from_ncthw": 0.96,
    "cl_im2col3x3": 0.61,
    "ncthw_from_cl": 0.72,
    "avgpool_time": 0.0,       # exact arithmetic: correctly rounded
    "axpby": 0.63,
    "posterior_sample": 0.59,
}
C_EMU = {"gn_stats": 1.52, "gn_sums": 3.34}


def allowed_k(op):
    return max(4.0, 8.0 * K_EMU[op])


def allowed_c(op):
    return 4.0 * C_EMU[op]


assert all(math.isfinite(v) for v in list(K_EMU.values()) + list(C_EMU.values()))
