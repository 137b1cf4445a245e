"""The case table of the MXFP8 family (csrc/mxfp8.hip: dove_mx_quant_bf16, dove_linear_mxfp8; csrc/attention_mx.hip: dove_qkv_post_mxfp8),
shared by tests/test_mx_cases_cpu.py (which checks the table's class keys, measures what an fp32 restatement of the GEMM's K order needs
against the float64 reference, and proves that wrong restatements fail) and tests/test_mx_fp64_gpu.py (which holds the kernels to the same
budget, inside poisoned operand slabs and guarded outputs).  The idiom is tests/igemm_cases.py's.

THE QUANTISER'S RULE (`quant_exact`), in float64 and integers: per 32-element block s = the smallest power of two in [2^-127, 2^127] with
amax / s <= 448 (amax = 0: 2^-127), q = e4m3fn(x / s) rounded to nearest even.  Both steps are exact: amax = m 2^ex with m in [0.5, 1)
gives ceil(log2(amax / 448)) = ex - 9 where m <= 0.875 and ex - 8 above (448 = 0.875 2^9); x / s is a bf16 value times a power of two.

WALK CLASSES of dove_linear_mxfp8.  `class_key(case, cus)` restates, from csrc/mxfp8.hip:
  the entry point's grid rule ("const unsigned grid = nt > cus ? (unsigned)cus : (unsigned)nt", nt = ceil(M / 256) N / 256)
  mx_decode     "GM = k.tiles_n > 16 ? 8u : 1u", "gm = left < GM ? left : GM", m0 = (group GM + within % gm) 256, n0 = (within / gm) 256,
                after xcd_remap(id, ntiles) (common.h: remainder branch where ntiles % 8 != 0); id >= ntiles is clamped to the last tile
  mx_open_tile  "s.n_on = id < k.ntiles", zero-length descriptors for an off-stream successor, "rows = left < BM ? left : BM"
  mx_advance    "if (++s.n_k4 == k.nk4) mx_open_tile(s, a, k, s.n_tile + k.G)": the successor opens during the tile's last 256-wide chunk
  the epilogue  "rows = vl >= 32 ? 32 : (vl > 0 ? (int)vl : 0)" per 32-row block of a wave's 128 rows (wm = wave >> 1 halves the tile)
The fields of a key:
  nk4     K / 256: 2 | 4 | 6+   (2: the hand-over falls in the K loop's only trip, right behind the prologue)
  tpw     most tiles one workgroup walks: 1 | 2 | 3+
  succ    the first successors id + G: off (ntiles <= cus: every one is off-stream) | mixed (cus < ntiles < 2 cus) | live
  round   lt (ntiles < cus) | eq (ntiles a multiple of cus) | ragged
  gm      1 | 8full | 8ragged
  xcdrem  ntiles % 8 != 0: 0 | 1
  mrem    M % 256: 0 | 1 | 31 | 32 | 33 | 127 | 128 | 129 | 255 | other ;  "mlt256" where M < 256
  inst    plain | plain_resid | gelu | gelu_resid (<true,false> taking its kRes branch) | gate
  bias    0 | 1
  ld      ldo== | ldo>  and, with a residual, ldr==ldo | ldr!=ldo
  xzero   the activation operand is all zero (the epilogue alone)
  gsplit  (gate) 0 | mid (inside a 32-row block) | t256 (a multiple of 256 inside M) | M | beyond

THE REFERENCE is float64 of the dequantised operand bytes (an e4m3 value times 2^e is exact), fp32 bias, tanh-GELU in float64,
resid + gate * v, no intermediate rounding.  `mag` = sum |x w| + |bias|, carried through the epilogue as in tests/igemm_cases.py.

THE BUDGET, per element:   |got - ref| <= 0.5 ulp_bf16(ref) + k 2^-24 mag  (+ 32 2^-24 max(|v|, |gelu v|) where act = 1)
k is not fitted to the kernel: `chain32` walks K in 64-element blocks (one v_mfma_scale_f32_32x32x64_f8f6f4 each) in the kernel's order with
one fp32 accumulator, one rounding per block.  A block is NOT summed exactly: the instruction, measured alone on operands built for the
purpose (docs/kernels.md section 4.2), aligns the products of every 8 consecutive K elements to the group's largest exponent sum E and
truncates each toward zero at 2^(E - 13) - `mfma_sum` restates that, and agrees with the instruction bit for bit on random operands of one
scale and to two fp32 roundings of mag with random scales and a C input.  With exactly summed blocks k_chain is 0.09 .. 3.4 and the
MI355X needs 40 .. 190; the truncation is first order in 2^-14 of a group's largest product, i.e. hundreds of 2^-24 mag where a block's
elements spread over binades.  A row stores k = max(1, 16 k_chain) as a literal, rounded up to three digits;
tests/test_mx_cases_cpu.py keeps it inside [16, 16.2] k_chain.  The margin of 16 is the igemm net's (2x the matrix core's unspecified
order across groups and rounding mode, 2x one CPU sample against up to 1e7 GPU elements, 2x2 slack).

OPERAND FAMILIES: "blocks": per-32-block log-normal magnitudes on BOTH operands (sigma two binades), so that a scale byte, an h half or
a row taken from a neighbouring block is first order; "offset": the same plus 3 before quantisation, so that a dropped K-step is.

dove_qkv_post_mxfp8: `qkv_ref64` is LayerNorm(64) + RoPE + scale in float64 with the magnitudes of tests/norm_ref.py; Q8 / K8 are held to
0.5 ulp_e4m3(ref) + k 2^-24 mag with k = max(4, 8 K_EMU_QKV) (the norm net's rule; K_EMU_QKV is what emu_ops' fp32 restatement needs,
asserted as an upper bound on the CPU); V8t / Vs are `quant_exact` along the keys in the stored quad order [0,2,4,6,1,3,5,7]."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

import torch

from igemm_cases import EPS24, GELU_LIP, _gelu64, k_of, ulp_out   # noqa: F401  (re-exported: the budget's pieces are the igemm net's)
from norm_cases import hash_key

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
F64 = torch.float64
FAMILIES = ("blocks", "offset")
BM = BN = 256
GUARD = -1232.0                                     # exact in bf16, nothing a case computes
GUARD_ROWS = 2


# ---- the exact quantiser ----------------------------------------------------------------------------------------------------------------
def _p2(k):
    """2^k in float64 for an integer tensor k (exp2 of an integer is exact; torch.ldexp would form the power in fp32)."""
    return torch.exp2(k.to(F64))


def e4m3_rne_bytes(y):
    """float64 |y| <= 448 -> e4m3fn bytes, round to nearest even, in float64 / integer arithmetic (the sign bit survives a zero result)."""
    y = y.to(F64)
    v = y.abs()
    assert bool((v <= 448.0).all()), "a value above 448 would be converted"
    ex = torch.frexp(v)[1].to(torch.int64) - 1                      # v = 1.m 2^ex
    ex = torch.where(v == 0, torch.full_like(ex, -6), ex).clamp_min(-6)   # below 2^-6: the subnormal step 2^-9
    k = torch.round(v * _p2(3 - ex)).to(torch.int64)         # v / 2^(ex-3), exact; torch.round is half-to-even; k in [0, 16]
    up = k == 16
    ex = torch.where(up, ex + 1, ex)
    k = torch.where(up, torch.full_like(k, 8), k)
    byte = torch.where(k < 8, k, ((ex + 7) << 3) | (k - 8))         # k < 8 only at ex = -6: exponent field 0
    assert bool((byte <= 0x7E).all())
    sign = torch.signbit(y).to(torch.int64) << 7
    return (byte | sign).to(torch.uint8)


def e8m0_exact(amax):
    """float64 amax >= 0 -> biased E8M0 exponent (int64) of the smallest power of two s in [2^-127, 2^127] with amax / s <= 448."""
    m, ex = torch.frexp(amax.to(F64))
    t = torch.where(m <= 0.875, ex - 9, ex - 8).to(torch.int64).clamp(-127, 127)
    return torch.where(amax > 0, t, torch.full_like(t, -127)) + 127


def quant_exact(x):
    """x [rows, K] (bf16 or any float holding bf16 values) -> (q uint8 [rows, K], e uint8 [rows, K/32])."""
    rows, K = x.shape
    xb = x.to(F64).reshape(rows, K // 32, 32)
    e = e8m0_exact(xb.abs().amax(dim=2))
    q = e4m3_rne_bytes(xb * _p2(127 - e)[..., None])
    return q.reshape(rows, K), e.to(torch.uint8)


def dequant64(q, e):
    rows, K = q.shape
    v = q.contiguous().view(F8).to(torch.float32).to(F64).reshape(rows, K // 32, 32)
    return (v * _p2(e.to(torch.int64) - 127)[..., None]).reshape(rows, K)


def scale_words(e):
    """[rows, K/32] exponents -> the kernel's layout int32 [K/256][rows][2]: word (c, r, h), byte u = block 8c + 2u + h."""
    rows, nb = e.shape
    w = e.reshape(rows, nb // 8, 4, 2).permute(1, 0, 3, 2).contiguous().to(torch.int64)       # [c][r][h][u]
    v = w[..., 0] | (w[..., 1] << 8) | (w[..., 2] << 16) | (w[..., 3] << 24)
    return torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)


def scale_bytes(words):
    """The inverse of scale_words: int32 [K/256][rows][2] -> uint8 [rows, K/32]."""
    nc, rows, _ = words.shape
    w = words.to(torch.int64) & 0xFFFFFFFF
    b = torch.stack([(w >> (8 * u)) & 0xFF for u in range(4)], dim=-1)                        # [c][r][h][u]
    return b.permute(1, 0, 3, 2).reshape(rows, nc * 8).to(torch.uint8)


# ---- the quantiser's sweep ------------------------------------------------------------------------------------------------------------------
def quant_sweep(K):
    """bf16 [rows, K]: one 32-element block per finite positive bf16 value (bit patterns 1 .. 0x7F7F, 32 639 of them) as the block's maximum,
    alternately positive and negative, then blocks of the edges (all zero, all -0, the maximum alone).  The other 31 elements of a block of
    maximum a, with s its exact scale: the seven e4m3 rounding ties of every binade of s that lie below a (s (8 + j + 1/2) 2^b / 8 is a bf16
    value: five significant bits), the ties inside e4m3's subnormals and around its underflow to zero (s 2^-9 (j + 1/2), s 2^-10, the bf16
    value just above and below it), +-0, the smallest bf16 subnormals, a / 2 and the bf16 value just below a, signs alternating - each kept
    only where it is a bf16 value of magnitude <= a, zero otherwise.  The blocks fill whole rows of K; the ragged last row is padded with
    zero blocks."""
    pat = torch.arange(1, 0x7F80, dtype=torch.int32)
    a = (pat << 16).view(torch.float32).to(F64)                     # every finite positive bf16 value
    e = e8m0_exact(a) - 127
    s = _p2(e)
    n = a.numel()
    cols = [a]
    cand = []
    for i in range(18):                                             # ties s (8 + j + 1/2) 2^(b-3): binade b and step j rotate with the
        b = 8 - (pat + i) % 15                                      # maximum's bit pattern, so the 128 maxima that share a scale cover them all
        j = (pat // 15 + i) % 7
        cand.append(s * (8 + j + 0.5).to(F64) * _p2(b - 3))
    for j in range(0, 8):                                           # subnormal ties s 2^-9 (j + 1/2); j = 0: the underflow tie s 2^-10
        cand.append(s * 2.0 ** -9 * (j + 0.5))
    below = ((pat - 1) << 16).view(torch.float32).to(F64)
    cand += [below, a / 2, s * 2.0 ** -10 * (1 + 2.0 ** -7), s * 2.0 ** -10 * (1 - 2.0 ** -8)]
    tiny = torch.tensor([2.0 ** -133, 3 * 2.0 ** -133], dtype=F64)
    cand += [tiny[0].expand(n), tiny[1].expand(n), torch.zeros(n, dtype=F64)]
    cand = cand[:31]
    assert len(cand) == 31
    for i, cnd in enumerate(cand):
        ok = (cnd.to(BF).to(F64) == cnd) & (cnd.abs() <= a)
        v = torch.where(ok, cnd, torch.zeros_like(cnd))
        cols.append(-v if i & 1 else v)                             # odd columns negative: -0 where the candidate was dropped
    blk = torch.stack(cols, dim=1)                                  # [n, 32], the maximum first
    blk[1::2, 0] = -blk[1::2, 0]                                    # both signs of the maximum
    rot = torch.arange(n) % 32                                      # the maximum visits every position of a block
    idx = (torch.arange(32)[None, :] - rot[:, None]) % 32
    blk = torch.gather(blk, 1, idx)
    edge = torch.zeros(3, 32, dtype=F64)
    edge[1] = -0.0
    edge[2, 17] = 448.0
    blk = torch.cat([blk, edge])
    per = K // 32
    pad = (-blk.shape[0]) % per
    blk = torch.cat([blk, torch.zeros(pad, 32, dtype=F64)])
    x = blk.reshape(-1, K).to(BF)
    assert bool((x.to(F64) == blk.reshape(-1, K)).all())
    return x


# ---- the GEMM's case table ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    act: int = 0
    resid: bool = False
    gate: bool = False
    gate_split: int = 0
    bias: bool = True
    ldo_x: int = 0                # output columns beyond N
    ldr_x: int = 0                # resid columns beyond N
    sampled: bool = False
    x_zero: bool = False          # the activation operand is all zero: the accumulators are exact zeros, the epilogue alone is checked
    kk: float = 1.0               # the budget's k (literal; see the module docstring)
    key: str = ""                 # expected class_key at 256 CUs, "/"-joined

    @property
    def ldo(self):
        return self.N + self.ldo_x

    @property
    def ldr(self):
        return self.N + self.ldr_x


def xcd_remap(bid, nwg):
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def decode(tid, ntiles, tiles_n, gm8_always=False):
    """mx_decode: tile id -> (row tile, column tile)."""
    rest = xcd_remap(min(tid, ntiles - 1), ntiles)
    GM = 8 if tiles_n > 16 else 1
    tiles_m = ntiles // tiles_n
    per_group = GM * tiles_n
    group, within = divmod(rest, per_group)
    left = tiles_m - group * GM
    gm = GM if gm8_always else min(left, GM)
    return group * GM + within % gm, within // gm


def geometry(c: Case, cus: int = 256):
    tiles_n, tiles_m = c.N // BN, (c.M + BM - 1) // BM
    ntiles = tiles_n * tiles_m
    return dict(tiles_n=tiles_n, tiles_m=tiles_m, ntiles=ntiles, G=min(ntiles, cus), nk4=c.K // 256)


_MREM = (0, 1, 31, 32, 33, 127, 128, 129, 255)


def class_key(c: Case, cus: int = 256) -> tuple:
    g = geometry(c, cus)
    nt, G, nk4 = g["ntiles"], g["G"], g["nk4"]
    assert c.K % 512 == 0 and c.N % 256 == 0 and not (c.gate and c.act) and (c.resid or not c.gate)
    tpw = (nt + G - 1) // G
    key = ["nk4=" + ("6+" if nk4 >= 6 else str(nk4)), "tpw=" + ("3+" if tpw >= 3 else str(tpw)),
           "succ=" + ("off" if nt <= cus else "mixed" if nt < 2 * cus else "live"),
           "round=" + ("lt" if nt < cus else "eq" if nt % cus == 0 else "ragged"),
           "gm=" + ("1" if g["tiles_n"] <= 16 else "8full" if g["tiles_m"] % 8 == 0 else "8ragged"),
           f"xcdrem={int(nt % 8 != 0)}", "mrem=" + (str(c.M % 256) if c.M % 256 in _MREM else "other")]
    if c.M < 256:
        key.append("mlt256")
    key.append("inst=" + ("gate" if c.gate else ("gelu" if c.act else "plain") + ("_resid" if c.resid else "")))
    key.append(f"bias={int(c.bias)}")
    key.append("ldo" + (">" if c.ldo_x else "=="))
    if c.resid:
        key.append("ldr" + ("==ldo" if c.ldr_x == c.ldo_x else "!=ldo"))
    if c.x_zero:
        key.append("xzero")
    if c.gate:
        gs = c.gate_split
        key.append("gsplit=" + ("0" if gs == 0 else "beyond" if gs > c.M else "M" if gs == c.M else "t256" if gs % 256 == 0 else
                                "mid" if gs % 32 else "other"))
    return tuple(key)


REQUIRED = (
    [[f] for f in ("nk4=2", "nk4=4", "nk4=6+", "tpw=1", "tpw=2", "tpw=3+", "succ=mixed", "gm=1", "gm=8full", "gm=8ragged", "xcdrem=0",
                   "xcdrem=1", "mlt256", "inst=plain", "inst=plain_resid", "inst=gelu", "inst=gelu_resid", "inst=gate", "bias=0", "bias=1",
                   "ldo==", "ldo>", "ldr==ldo", "ldr!=ldo", "gsplit=0", "gsplit=mid", "gsplit=t256", "gsplit=M", "gsplit=beyond")]
    + [[f"mrem={r}"] for r in _MREM]
    + [["succ=off", "round=lt"], ["succ=off", "round=eq"], ["succ=live", "round=eq", "tpw=2"], ["nk4=2", "tpw=2"], ["ldo>", "ldr==ldo"],
       ["mrem=255", "tpw=1"], ["mrem=1", "mlt256"], ["xzero", "inst=gelu"]]
)


def missing_classes(cases, cus: int = 256):
    keys = [class_key(c, cus) for c in cases]
    return [f for f in REQUIRED if not any(all(x in key for x in f) for key in keys)]


_ROWS = [
    # ---- one tile (every successor off-stream, ntiles < G): the row tails, the instantiations, the strides, the gate splits
    Case("m1", 1, 256, 512),
    Case("m31_nobias", 31, 256, 512, bias=False),
    Case("m32_ldo", 32, 256, 512, ldo_x=8),
    Case("m33_resid_ldr", 33, 256, 512, resid=True, ldr_x=4),
    Case("m127_gelu", 127, 256, 512, act=1),
    Case("m128_gelu_resid", 128, 256, 512, act=1, resid=True),
    Case("m129_gate0", 129, 256, 512, resid=True, gate=True, gate_split=0),
    Case("m255_gate_mid", 255, 256, 512, resid=True, gate=True, gate_split=45),
    Case("m256_gate_M", 256, 256, 512, resid=True, gate=True, gate_split=256),
    Case("m257_gate_beyond", 257, 256, 512, resid=True, gate=True, gate_split=357),
    Case("m511_gate_t256", 511, 256, 512, resid=True, gate=True, gate_split=256, bias=False),
    Case("m300_k1024_ld", 300, 512, 1024, resid=True, ldo_x=8, ldr_x=8),
    Case("m64_k1536_gelu", 64, 256, 1536, act=1),
    # ---- x = 0: out = GELU(bias) with k = 1.  The one class on which the tanh form can be told from the erf form: they differ by at most
    # 4.7e-4 (near |v| = 2.2), and where products are summed the instruction's own truncation, times the margin of 16, is above that
    Case("m40_gelu_xzero", 40, 256, 512, act=1, x_zero=True),
    # ---- GM = 8 with a ragged last group, the smallest: 3 x 17 tiles
    Case("gm8_ragged", 513, 4352, 512),
    # ---- ntiles = G: one full round, every successor off-stream
    Case("one_round", 32768, 512, 512, sampled=True),
    # ---- G < ntiles < 2G: 9 x 30 tiles, workgroups 0 .. 13 hand over to a live tile behind the prologue, the others to an off-stream one
    Case("mixed_270", 2177, 7680, 512, act=1, sampled=True),
    # ---- ntiles = 2G: 16 x 32 tiles, every first successor live, every second off-stream; the gated residual rides the hand-over
    Case("two_rounds", 4096, 8192, 512, resid=True, gate=True, gate_split=226, sampled=True),
    # ---- three tiles on workgroup 0: 27 x 19 = 513 tiles
    Case("three_tiles", 6700, 4864, 512, sampled=True),
]
# name -> (k of the budget = 16 k_chain rounded up to three digits, expected class_key at 256 CUs); the comment is the measured k_chain
_S1 = "nk4=2/tpw=1/succ=off/round=lt/gm=1/xcdrem=1/"
EXPECT = {
    "m1": (2140.0, _S1 + "mrem=1/mlt256/inst=plain/bias=1/ldo=="),   # 133.1
    "m31_nobias": (5010.0, _S1 + "mrem=31/mlt256/inst=plain/bias=0/ldo=="),   # 313.0
    "m32_ldo": (8810.0, _S1 + "mrem=32/mlt256/inst=plain/bias=1/ldo>"),   # 550.4
    "m33_resid_ldr": (5830.0, _S1 + "mrem=33/mlt256/inst=plain_resid/bias=1/ldo==/ldr!=ldo"),   # 363.9
    "m127_gelu": (8300.0, _S1 + "mrem=127/mlt256/inst=gelu/bias=1/ldo=="),   # 518.6
    "m128_gelu_resid": (5280.0, _S1 + "mrem=128/mlt256/inst=gelu_resid/bias=1/ldo==/ldr==ldo"),   # 329.7
    "m129_gate0": (6540.0, _S1 + "mrem=129/mlt256/inst=gate/bias=1/ldo==/ldr==ldo/gsplit=0"),   # 408.4
    "m255_gate_mid": (8360.0, _S1 + "mrem=255/mlt256/inst=gate/bias=1/ldo==/ldr==ldo/gsplit=mid"),   # 522.3
    "m256_gate_M": (7370.0, _S1 + "mrem=0/inst=gate/bias=1/ldo==/ldr==ldo/gsplit=M"),   # 460.0
    "m257_gate_beyond": (8850.0, "nk4=2/tpw=1/succ=off/round=lt/gm=1/xcdrem=1/mrem=1/inst=gate/bias=1/ldo==/ldr==ldo/gsplit=beyond"),   # 552.8
    "m511_gate_t256": (11100.0, "nk4=2/tpw=1/succ=off/round=lt/gm=1/xcdrem=1/mrem=255/inst=gate/bias=0/ldo==/ldr==ldo/gsplit=t256"),   # 688.9
    "m300_k1024_ld": (8870.0, "nk4=4/tpw=1/succ=off/round=lt/gm=1/xcdrem=1/mrem=other/inst=plain_resid/bias=1/ldo>/ldr==ldo"),   # 554.0
    "m64_k1536_gelu": (4210.0, "nk4=6+/tpw=1/succ=off/round=lt/gm=1/xcdrem=1/mrem=other/mlt256/inst=gelu/bias=1/ldo=="),   # 263.0
    "m40_gelu_xzero": (1.0, _S1 + "mrem=other/mlt256/inst=gelu/bias=1/ldo==/xzero"),   # 0.0
    "gm8_ragged": (9680.0, "nk4=2/tpw=1/succ=off/round=lt/gm=8ragged/xcdrem=1/mrem=1/inst=plain/bias=1/ldo=="),   # 604.8
    "one_round": (10400.0, "nk4=2/tpw=1/succ=off/round=eq/gm=1/xcdrem=0/mrem=0/inst=plain/bias=1/ldo=="),   # 644.9
    "mixed_270": (15900.0, "nk4=2/tpw=2/succ=mixed/round=ragged/gm=8ragged/xcdrem=1/mrem=129/inst=gelu/bias=1/ldo=="),   # 992.3
    "two_rounds": (14500.0, "nk4=2/tpw=2/succ=live/round=eq/gm=8full/xcdrem=0/mrem=0/inst=gate/bias=1/ldo==/ldr==ldo/gsplit=mid"),   # 902.5
    "three_tiles": (13200.0, "nk4=2/tpw=3+/succ=live/round=ragged/gm=8ragged/xcdrem=1/mrem=other/inst=plain/bias=1/ldo=="),   # 819.7
}
CASES = [dataclasses.replace(c, kk=EXPECT[c.name][0], key=EXPECT[c.name][1]) for c in _ROWS]


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(hash_key("mx", *key))


def _blocks(rows, K, g, shift):
    v = torch.randn(rows, K // 32, 32, generator=g) * torch.exp2(2.0 * torch.randn(rows, K // 32, 1, generator=g))
    return (v + shift).reshape(rows, K)


def operands(c: Case, family: str) -> dict:
    """CPU operands: x [M, K], w [N, K] bf16, bias [N] fp32 | None, resid [M, ldr] bf16 | None, gate [2, N] fp32 | None."""
    assert family in FAMILIES
    g = _gen(c.name, family)
    shift = 3.0 if family == "offset" else 0.0
    x = _blocks(c.M, c.K, g, shift).to(BF)
    if c.x_zero:
        x = torch.zeros_like(x)
    w = (_blocks(c.N, c.K, g, shift) * c.K ** -0.5).to(BF)
    b = torch.randn(c.N, generator=g) if c.bias else None
    resid = (4.0 * torch.randn(c.M, c.ldr, generator=g)).to(BF) if c.resid else None
    gate = (0.3 * torch.randn(2, c.N, generator=g) + torch.tensor([0.6, -1.3])[:, None]) if c.gate else None
    return dict(x=x, w=w, bias=b, resid=resid, gate=gate)


def quantise_cpu(inp: dict) -> dict:
    """Adds the exact rule's bytes and exponents (xq, xe, wq, we): what the CPU tests multiply; the GPU test puts the kernel's own there."""
    out = dict(inp)
    out["xq"], out["xe"] = quant_exact(inp["x"])
    out["wq"], out["we"] = quant_exact(inp["w"])
    return out


def sample_rows(c: Case):
    """Rows a sampled case is checked at (all N columns each): 0 and M - 1, both sides of every 32 / 128 / 256-row boundary of the first and
    the last row tile, both sides of gate_split, one more row of every row tile.  None: the case is checked everywhere."""
    if not c.sampled:
        return None
    tiles_m = (c.M + BM - 1) // BM
    pick = [0, c.M - 1]
    for t0 in (0, (tiles_m - 1) * BM):
        for j in range(0, 9):
            pick += [t0 + 32 * j - 1, t0 + 32 * j]
    if c.gate:
        pick += [c.gate_split - 1, c.gate_split]
    g = _gen("rows", c.name)
    for t in range(tiles_m):
        pick.append(t * BM + int(torch.randint(0, min(BM, c.M - t * BM), (1,), generator=g)))
    return torch.unique(torch.tensor([p for p in pick if 0 <= p < c.M]))


# ---- the float64 reference and the fp32 chain -----------------------------------------------------------------------------------------------
POISON = 1.5                                       # finite poison behind the activation operand (mutant rows_past_m)


def _mut_scales(e, how):
    """e [rows, K/32] with block = 8c + 2u + h; one wrong way of picking a block's scale."""
    rows, nb = e.shape
    v = e.reshape(rows, nb // 8, 4, 2)                               # [r][c][u][h]
    if how == "u_plus":
        v = torch.roll(v, -1, dims=2)
    elif how == "u_minus":
        v = torch.roll(v, 1, dims=2)
    elif how == "h_swap":
        v = v.flip(3)
    elif how == "row_next":
        v = torch.roll(v, -1, dims=0)
    elif how == "chunk_next":
        v = torch.roll(v, -1, dims=1)
    return v.reshape(rows, nb)


MFMA_GROUP, MFMA_KEEP = 8, 13


def elem_exp(q, e):
    """The exponent the matrix core sees for each element: e4m3 field (0 reads as 1: subnormals and zero) - 7, plus the block scale's."""
    rows, K = q.shape
    f = ((q.to(torch.int64) >> 3) & 15).clamp_min(1) - 7
    return (f.reshape(rows, K // 32, 32) + (e.to(torch.int64) - 127)[..., None]).reshape(rows, K)


def mfma_sum(X, W, eX, eW):
    """The 64 scaled products of one v_mfma_scale_f32_32x32x64_f8f6f4 as the MI355X sums them (measured with one instruction and operands
    built for the purpose, docs/kernels.md section 4.2): inside each group of MFMA_GROUP consecutive K elements every product is aligned to
    the group's largest exponent sum E = max (e_x + e_w) (elem_exp; the product itself is below 2^(E + 2)) and truncated toward zero to a
    multiple of 2^(E - MFMA_KEEP); the eight group sums are then added without a visible loss.  X [n, 64], W [N, 64] float64, eX, eW their
    element exponents -> [n, N] float64."""
    n, N = X.shape[0], W.shape[0]
    out = torch.empty(n, N, dtype=F64)
    step = max(1, (1 << 22) // max(N, 1))
    G = 64 // MFMA_GROUP
    for r0 in range(0, n, step):
        P = (X[r0:r0 + step, None, :] * W[None, :, :]).reshape(-1, N, G, MFMA_GROUP)
        E = (eX[r0:r0 + step, None, :] + eW[None, :, :]).reshape(-1, N, G, MFMA_GROUP)
        E = torch.where(P == 0, torch.full_like(E, -1000), E)       # a zero product does not set the group's exponent
        grid = torch.exp2((E.amax(dim=3, keepdim=True) - MFMA_KEEP).to(F64))
        out[r0:r0 + step] = (torch.trunc(P / grid) * grid).sum(dim=(2, 3))
    return out


def reference64(c: Case, inp: dict, rows=None, mut: str | None = None, cus: int = 256):
    """(ref, mag, gterm) float64 [n, N] over the output rows `rows` (None: all).  `inp` holds the quantised operands (xq, xe, wq, we).
    `mut` names one deliberately wrong restatement (tests/test_mx_cases_cpu.py)."""
    M, N, K = c.M, c.N, c.K
    if rows is None:
        rows = torch.arange(M)
    xe, we = inp["xe"], inp["we"]
    if mut in ("u_minus", "h_swap", "chunk_next"):
        xe = _mut_scales(xe, mut)
    if mut in ("u_plus", "row_next"):
        we = _mut_scales(we, mut)
    X = dequant64(inp["xq"][rows], xe[rows])
    W = dequant64(inp["wq"], we)
    Xr = X                                                           # what the reference's magnitude is made of
    if mut == "drop_step":
        X = X.clone()
        X[:, K - 192:K - 128] = 0                                    # step u = 1 of the last chunk
    ref = X @ W.T
    mag = Xr.abs() @ W.abs().T
    g = geometry(c, cus)
    if mut == "next_tile_chunk":                                     # the last chunk's operands come from tile id + G (zeros off-stream)
        ids = {decode(t, g["ntiles"], g["tiles_n"]): t for t in range(g["ntiles"])}
        Xall_q, Xall_e = inp["xq"], inp["xe"]
        kl = slice(K - 256, K)
        for tm in torch.unique(rows // BM).tolist():
            sel = (rows // BM == tm).nonzero()[:, 0]
            for tn in range(g["tiles_n"]):
                cs = slice(tn * BN, (tn + 1) * BN)
                ref[sel, cs] -= X[sel][:, kl] @ W[cs, kl].T
                nid = ids[(tm, tn)] + g["G"]
                if nid < g["ntiles"]:
                    tm2, tn2 = decode(nid, g["ntiles"], g["tiles_n"])
                    r2 = rows[sel] - tm * BM + tm2 * BM
                    ok = r2 < M
                    r2 = r2.clamp_max(M - 1)
                    X2 = dequant64(Xall_q[r2], Xall_e[r2])[:, kl] * ok[:, None]
                    ref[sel, cs] += X2 @ W[tn2 * BN:(tn2 + 1) * BN, kl].T
    if mut == "gm8_always":                                          # tiles the wrong decode never reaches keep their prefill
        seen = {decode(t, g["ntiles"], g["tiles_n"], gm8_always=True) for t in range(g["ntiles"])}
        for tm in torch.unique(rows // BM).tolist():
            sel = (rows // BM == tm).nonzero()[:, 0]
            for tn in range(g["tiles_n"]):
                if (tm, tn) not in seen:
                    ref[sel, tn * BN:(tn + 1) * BN] = float("nan")
    # ---- epilogue ----
    gterm = torch.zeros_like(ref)
    if inp["bias"] is not None:
        bias = inp["bias"].double()
        if mut == "bias_neighbour":
            bias = torch.roll(bias, -8)                              # the next lane's eight columns
        ref = ref + bias
        mag = mag + inp["bias"].double().abs()
    if c.act == 1:
        pre = ref
        ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0))) if mut == "gelu_erf" else _gelu64(pre)
        mag = GELU_LIP * mag
        gterm = 32 * EPS24 * torch.maximum(pre.abs(), ref.abs())
    if c.resid:
        if mut == "ldr_as_ldo":                                      # the residual read with the output's pitch
            flat = inp["resid"].reshape(-1)
            idx = (rows[:, None] * c.ldo + torch.arange(N)[None, :]) % flat.numel()
            r = flat[idx]
        else:
            r = inp["resid"][rows][:, :N]
        if mut == "resid_after_round":
            ref = ref.to(BF).double()
        if c.gate:
            cls = rows >= c.gate_split + (1 if mut == "gate_off1" else 0)
            if mut == "gate_swap":
                cls = ~cls
            gg = inp["gate"].double()[cls.long()]
            ref = r.double() + gg * ref
            mag = r.double().abs() + gg.abs() * mag
            gterm = gg.abs() * gterm
        else:
            ref = r.double() + ref
            mag = r.double().abs() + mag
    return ref, mag, gterm


CHAIN_ELEMENTS = 1 << 18


def chain_rows(c: Case, rows):
    """Positions in `rows` the chain restatement is evaluated at: all where rows x N <= CHAIN_ELEMENTS, else that many, evenly spaced (the
    restatement forms every one of the rows x N x K products)."""
    n = len(rows)
    keep = max(1, CHAIN_ELEMENTS // c.N)
    return torch.arange(n) if n <= keep else torch.unique(torch.linspace(0, n - 1, keep).round().long())


def chain32(c: Case, inp: dict, rows, exact_blocks: bool = False):
    """The fp32 chain restatement of the kernel's K order at the output rows `rows`: one fp32 accumulator, one MFMA (64 K elements) per step
    summed as `mfma_sum` says and added with one rounding, then the epilogue in fp32 - the un-rounded value handed to the output rounding.
    `exact_blocks`: every 64-block summed exactly instead (what the restatement was before the instruction was measured)."""
    X, W = dequant64(inp["xq"][rows], inp["xe"][rows]), dequant64(inp["wq"], inp["we"])
    eX, eW = elem_exp(inp["xq"][rows], inp["xe"][rows]), elem_exp(inp["wq"], inp["we"])
    acc = torch.zeros(len(rows), c.N, dtype=torch.float32)
    for k0 in range(0, c.K, 64):
        ks = slice(k0, k0 + 64)
        blk = X[:, ks] @ W[:, ks].T if exact_blocks else mfma_sum(X[:, ks], W[:, ks], eX[:, ks], eW[:, ks])
        acc = (acc.double() + blk).float()
    if inp["bias"] is not None:
        acc = acc + inp["bias"].float()
    if c.act == 1:
        acc = torch.nn.functional.gelu(acc, approximate="tanh")
    if c.resid:
        r = inp["resid"][rows][:, :c.N].float()
        acc = r + inp["gate"].float()[(rows >= c.gate_split).long()] * acc if c.gate else r + acc
    return acc


def budget(c: Case, ref, mag, gterm, k=None):
    return 0.5 * ulp_out(ref) + (c.kk if k is None else k) * EPS24 * mag + gterm


def over_budget(got, tol_ref, tol):
    """Elements outside the budget; an element that is not a number is outside it."""
    return ~((got.double() - tol_ref).abs() <= tol)


def guarded_out(c: Case, device="cpu", prefill=None):
    """([M + 4, ldo] buffer, its [M, ldo] interior): the guard value in the two rows before and after and in the columns [N, ldo); the stored
    columns NaN, or `prefill` (the residual of an in-place launch)."""
    buf = torch.full((c.M + 2 * GUARD_ROWS, c.ldo), GUARD, dtype=BF, device=device)
    out = buf[GUARD_ROWS:GUARD_ROWS + c.M]
    out[:, :c.N] = float("nan")
    if prefill is not None:
        out[:, :c.N] = prefill[:, :c.N]
    return buf, out


def guards_intact(c: Case, buf):
    g = GUARD_ROWS
    return bool((buf[:g] == GUARD).all()) and bool((buf[-g:] == GUARD).all()) and bool((buf[g:-g, c.N:] == GUARD).all())


def rows_past_m_store(c: Case, inp: dict, buf):
    """The wrong restatement 'rows past M are neither zeroed nor dropped': the last row tile's rows M, M + 1, .. multiply the finite poison
    that lies behind the activation operand and are stored like any other row (those that fall inside the buffer)."""
    W = dequant64(inp["wq"], inp["we"])
    n = min(GUARD_ROWS, (-c.M) % BM)
    v = (torch.full((n, c.K), POISON, dtype=F64) @ W.T).to(BF)
    buf[GUARD_ROWS + c.M:GUARD_ROWS + c.M + n, :c.N] = v


# ---- dove_qkv_post_mxfp8 ------------------------------------------------------------------------------------------------------------------------
K_EMU_QKV = 24.0              # what emu_ops' fp32 restatement needs: 19.7 measured (tests/test_mx_cases_cpu.py asserts the bound); its mean of 64
                              # terms errs by roundings of E|x|, which the element's own |x| + |mean| can undercut several times


def qkv_allowed_k():
    return max(4.0, 8.0 * K_EMU_QKV)


def ulp_e4m3(ref):
    """Spacing of e4m3fn at |ref|: 2^(e - 3), the subnormal spacing 2^-9 below 2^-6."""
    e = torch.frexp(ref.abs().to(F64).clamp_min(2.0 ** -6))[1] - 1
    return _p2(e - 3)


def qkv_operands(N, heads, text_len, with_rope=True):
    """qkv [N, 3 heads 64] bf16, the four LayerNorm vectors, cos / sin [N - text_len, 64] fp32 whose pair entries DIFFER (cr[2i + 1] is not
    cr[2i]: a kernel that reads one entry for both elements of a pair is wrong by first order)."""
    g = _gen("qkv", N, heads, text_len)
    D = heads * 64
    qkv = (torch.randn(N, 3 * D, generator=g) * torch.exp2(torch.randn(N, 1, generator=g))).to(BF)
    aff = tuple(t.contiguous() for t in (1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g),
                                          1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)))
    cos = sin = None
    if with_rope:
        ang = torch.rand(max(N - text_len, 1), 64, generator=g) * 6.28
        cos, sin = ang.cos().contiguous(), (ang + 0.3 * torch.randn(ang.shape, generator=g)).sin().contiguous()
    return qkv, aff, cos, sin


def qkv_ref64(qkv, N, heads, text_len, aff, cos, sin, qscale, eps, mut=None):
    """(Q, magQ, K, magK) float64 [heads, N, 64]: LayerNorm(64) + RoPE on the rows >= text_len + (qscale 8 on Q), and the sum of the absolute
    terms (tests/norm_ref.py ln_mod; a rotated element adds its two products)."""
    from norm_ref import f32
    gq, bq, gk, bk = (t.to(F64) for t in aff)
    if mut == "gk_for_gq":
        gq = gk
    D = heads * 64
    eps = f32(eps) * (10.0 if mut == "eps10" else 1.0)
    out = []
    for i, (gam, bet) in enumerate(((gq, bq), (gk, bk))):
        x = qkv.to(F64)[:, i * D:(i + 1) * D].reshape(N, heads, 64)
        mean = x.mean(dim=2, keepdim=True)
        var = ((x - mean) ** 2).sum(dim=2, keepdim=True) / (63.0 if mut == "var_d1" else 64.0)
        rstd = 1.0 / torch.sqrt(var + eps)
        y = (x - mean) * rstd * gam + bet
        mag = (x.abs() + mean.abs()) * rstd * gam.abs() + bet.abs()
        if cos is not None:
            t0 = 0 if mut == "rope_on_text" else text_len
            n_rot = N - t0
            if n_rot > 0:
                rowi = torch.arange(n_rot) + (t0 - text_len)
                if mut == "table_row_off1":
                    rowi = rowi + 1
                rowi = rowi.clamp(0, cos.shape[0] - 1)
                cr, sr = cos.to(F64)[rowi][:, None, :], sin.to(F64)[rowi][:, None, :]
                if mut == "pair_swapped":
                    cr, sr = cr.reshape(n_rot, 1, 32, 2).flip(3).reshape(n_rot, 1, 64), sr.reshape(n_rot, 1, 32, 2).flip(3).reshape(n_rot, 1, 64)
                yv, mv = y[t0:], mag[t0:]
                a, b = yv[..., 0::2], yv[..., 1::2]
                ma, mb = mv[..., 0::2], mv[..., 1::2]
                rot = torch.stack([a * cr[..., 0::2] - b * sr[..., 0::2], b * cr[..., 1::2] + a * sr[..., 1::2]], dim=-1).flatten(2)
                mrot = torch.stack([ma * cr[..., 0::2].abs() + mb * sr[..., 0::2].abs(),
                                    mb * cr[..., 1::2].abs() + ma * sr[..., 1::2].abs()], dim=-1).flatten(2)
                y, mag = torch.cat([y[:t0], rot]), torch.cat([mag[:t0], mrot])
        sc = f32(f32(qscale) * 8.0) if i == 0 else 1.0
        if mut == "q_not_x8" and i == 0:
            sc = f32(qscale)
        out += [(y * sc).permute(1, 0, 2).contiguous(), (mag * abs(sc)).permute(1, 0, 2).contiguous()]
    return tuple(out)


def qkv_budget(ref, mag, k=None):
    return 0.5 * ulp_e4m3(ref) + (qkv_allowed_k() if k is None else k) * EPS24 * mag


def v8_store_index(npad):
    """position p of a V8t row holds key v8_store_index[p]: inside every 32-key block the quads are stored [0,2,4,6,1,3,5,7]."""
    idx = torch.arange(npad)
    qs = (idx >> 2) & 7
    return (idx & ~31) | (((qs & 3) * 2 + (qs >> 2)) << 2) | (idx & 3)


def v_exact(qkv, N, npad, heads):
    """(V8t uint8 [heads, 64, npad] in the stored order, Vs uint8 [heads, npad / 64, 64, 2]) by the exact rule along the keys; pad keys are
    zero bytes and blocks wholly in the pad carry scale byte 0."""
    D = heads * 64
    v = torch.zeros(heads, 64, npad, dtype=F64)
    v[:, :, :N] = qkv.to(F64)[:, 2 * D:].reshape(N, heads, 64).permute(1, 2, 0)
    q, e = quant_exact(v.reshape(heads * 64, npad))
    return (q.reshape(heads, 64, npad)[..., v8_store_index(npad)].contiguous(),
            e.reshape(heads, 64, npad // 64, 2).permute(0, 2, 1, 3).contiguous())
