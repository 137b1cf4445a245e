"""The case table of the implicit-GEMM family (csrc/igemm.hip, csrc/igemm_legacy.hip: everything behind dove_conv_igemm_bf16), shared by
tests/test_igemm_cases_cpu.py (which checks the table against the library's dispatch, measures what an fp32 restatement of each kernel's
K order needs against the float64 reference, and proves that wrong restatements fail) and tests/test_igemm_fp64_gpu.py (which holds the
kernels to the same budget, inside poisoned operand slabs and a guarded output).

WALK CLASSES.  `class_key(case, cus)` restates the dispatch and the walk parameters each kernel derives from its arguments; a key is the
kernel's name followed by "field=value" strings.  Where each field comes from:

  select_kernel (igemm.hip, "static ConvKernel select_kernel"): smallk | gemm8p | halo4x | halo4x_up | halo4x_sub | igemm_fast | igemm.
  smallk (smallk_kernel; grid in conv_dispatch "case K_SMALLK")
      last   rows of the last 128-row block: lt32 (waves 1-3 break at once: "if (m >= M) break"), ragged (ends inside a wave's 32 rows),
             wave (ends on a wave boundary), full
      cout   c128 | lt256 | ragged_y2 (grid.y > 1 and "live = n0 < cout_store" cuts the last block) | c256k
      bias   0 | 1
  gemm8p (gemm8p_kernel, g4_decode / g4_open_tile in igemm_args.h, gemm_tail_split, conv_dispatch "case K_GEMM8P")
      inst   plain | plain_resid | gelu | gate (the three instantiations; plain with a residual and no gate)
      nk4    2 | 3 | 4+ ("kc.nk4 = a.Cin / 128")
      last   rows of the launch's last row tile: 1 | le128 (waves 4-7 have no row) | 129 | mid | full ("rows = left < BM ? left : BM")
      tpw    tiles per workgroup: 1 (grid = ntiles <= cus) | multi (ntiles % cus == 0) | multi_off (some workgroups open tiles with
             "n_on = id < k.ntiles" false)
      gm     1 | 8full | 8ragged ("GM = k.tiles_n > 16 ? 8u : 1u", "gm = left < GM ? left : GM")
      split  taken, or the reason gemm_tail_split returns false: not_token_major | le_cus | even | tail_blocks.  (Its two other exits
             cannot be reached with buffers a test may allocate: main_rt < 1 needs Cout > 65536, main_rt >= row_tiles contradicts
             ntiles % cus != 0, 128 * Cin * 2 >= 2^31 needs Cin >= 2^23.)
      gsplit where gate_split falls: none | main (before rows_main) | edge (== rows_main: the tail's split clamps to 0) | tail | nosplit
      tail   the igemm_fast key of the tail launch (split taken)
      flags  cout<st (zero weight rows inside the stored columns), inplace, nt_out ("a.nt_out = M * ldo * 2 > 256 MB"), ldo>st
  halo4x (conv3x3_halo4x_kernel<false, false, kPart>, h4_split, h4_decode, halo4x_plan, dove_conv_gn_partial_rows)
      kt     1 | 3
      route  kt1 | cache | nocache_wfirst | nocache_plain | tdup1_cache | tdup1_nocache | tdup2 ; splits = the h4_split classes met
      nb     1 | n | n_strided
      kcn    Cin / 32 ; ctiles = Cout_pad / 128
      hrem   H % 16: 0 | 1..15 ; wrem  W % 32: 0 | 1..16 | 17..31 ; min16 (16 x 16, the smallest image the kernel takes)
      tpw    lt1 (grid = ntiles) | 1 | multi | multi_off, of the main launch ; xcdrem = ntiles % 8 != 0 (xcd_remap's remainder branch)
      part   0 | 1 | 1cut (the 32 x 16 launch's last tile ends inside the image: H % 32 != 0)
      resid  0 | ld= | ld> ; ldo  = | > ; gn  0 | 128 | 256 | 512
  halo4x_up (<kUp>): tmode 0 | 1 | 2 ; why  lowres_small | no_wsub ; hrem, wrem of the OUTPUT ; ctiles ; kcn
  halo4x_sub (<kSub>): tmode ; hrem, wrem of the LOW-RES grid (the four phases always run: tiles_n = 4 x Cout / 128) ; ctiles ; kcn
  igemm_fast (igemm_fast_kernel<BN, BK>, conv_dispatch's generic tail)
      inst   BNxBK ; nk  1 | 2 | odd | even ("nk = kt kh kw Cin / BK", the pair loop and its odd tail) ; tw  tw_log2 7 | 4 | 3 | 2
      stride 1 | 2even | 2odd ; front  kt1 | cache | frame0 (igemm_src_frame) ; nb ; epi  act / resid / gate / f32 / bias letters
      st<pad ("if (cb >= a.Cout_st) continue") ; st%8 (an 8-channel fragment half stored)
  igemm (igemm_legacy.hip: up == 1 shapes too small for the halo tile): tmode ; inst BNxBK

THE REFERENCE is what the launch is defined to compute, in float64 from the bf16 operands as packed: per output frame the temporal groups
of ops.temporal_split on the table each group uses (w, w_first, w_pair; w_sub per phase), fp32 bias, tanh-GELU in float64, resid + gate * v,
no intermediate rounding.  `mag` = sum |w x| + |bias|, carried through the epilogue as |resid| + |gate| mag_v (GELU: Lipschitz bound 1.13).

THE BUDGET, per element:   |got - ref| <= 0.5 ulp_out(ref) + k 2^-24 mag  (+ 32 2^-24 max(|v|, |gelu v|) where act = 1)
k is not fitted to the kernels: `chain32` walks K with one fp32 accumulator in the kernel's documented order (halo4x: temporal group -> 32
channel chunk -> spatial tap, blocks of 32; igemm_fast / igemm: tap -> chunk, blocks of 16; gemm8p: blocks of 32; smallk: pairs, starting
from the bias), every block summed exactly and rounded once.  k_chain = max |chain - ref| / (2^-24 mag) over both operand families; a row
stores k = max(1, 16 k_chain) as a literal, rounded UP to three digits (2x each for the matrix core's unspecified in-block order and rounding mode, 2x for one CPU
sample against up to 1e7 GPU elements, 2x slack).  tests/test_igemm_cases_cpu.py asserts 16 k_chain <= k <= 64 k_chain (or k = 1), and
that the literal is no more than the three-digit rounding above 16 k_chain.

THE FUSED GROUPNORM PARTIAL SUMS (gn_partial of halo4x, <kUp>, <kSub>) have their own reference, `gn_partials64`: per 4-row slot of a 16 x 32
tile the (sum, sum of squares) of the STORED values over the pixels inside the image, held to K_GN 2^-24 sum |v| (K_GN from the depth of
the kernel's reduction, see there).  Tile rows / columns past the image entering the sums miss it on every case with a ragged tile."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

import torch

from norm_cases import hash_key

BF = torch.bfloat16
FAMILIES = ("plain", "offset")
EPS24 = 2.0 ** -24
GELU_LIP = 1.13
N_RANDOM_SAMPLES = 4096


@dataclass(frozen=True)
class Case:
    name: str
    cin: int
    cout: int
    k: tuple                      # (kt, kh, kw)
    T: int                        # input frames per instance
    H: int
    W: int
    nb: int = 1
    stride: int = 1
    pad: tuple | None = None
    up: int = 0
    tmode: int = 0
    t_out: int | None = None
    cache: str = ""               # "" | "c" (contiguous) | "s" (nb > 1: a strided view, as the VAE hands over)
    resid: bool = False
    ldr_x: int = 0                # resid columns beyond cout_store
    ldo_x: int = 0                # output columns beyond cout_store
    gate: bool = False
    gate_split: int = 0
    act: int = 0
    inplace: bool = False
    bias: bool = True
    out_f32: bool = False
    tdup: int = 0
    wsums: bool = True
    gn: bool = False
    sampled: bool = False
    kk: float = 1.0               # the budget's k (literal; see the module docstring)
    key: str = ""                 # expected class_key at 256 CUs, "/"-joined


def _ru(x, m):
    return (x + m - 1) // m * m


def desc(c: Case) -> dict:
    """The dove_conv_desc fields ops.conv derives for this case (include/dove_hip.h), as a dict."""
    kt, kh, kw = c.k
    cin_pad = _ru(c.cin, 32) if c.cin <= 32 or c.cin % 64 else c.cin
    ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if c.pad is None else c.pad
    t_out = c.T if c.t_out is None else c.t_out
    if c.stride == 1:
        h_out, w_out = c.H << c.up, c.W << c.up
    else:
        h_out, w_out = (c.H + 1 - kh) // c.stride + 1, (c.W + 1 - kw) // c.stride + 1
    cs = _ru(c.cout, 4)
    cached = bool(c.cache)
    tdup = c.tdup if (c.tdup and c.wsums and kt == 3 and not (c.tdup == 2 and cached)) else 0
    return dict(nb=c.nb, t_in=c.T, h_in=c.H, w_in=c.W, cin=cin_pad, t_out=t_out, h_out=h_out, w_out=w_out, cout_pad=_ru(c.cout, 32),
                cout_store=cs, kt=kt, kh=kh, kw=kw, stride=c.stride, pad_h=ph, pad_w=pw, up=c.up, tmode=c.tmode, act=c.act,
                ldo=cs + c.ldo_x, ldr=(cs + c.ldr_x) if (c.resid or c.gate) else 0, gate_split=c.gate_split, resid=c.resid or c.gate,
                gate=c.gate, cached=cached, out_f32=c.out_f32, tdup=tdup, w_first=kt == 3 and not cached and c.wsums,
                w_sub=c.up == 1 and kt == 1 and kh == 3 and kw == 3 and c.wsums, w_pair=bool(tdup))


def lib_desc(c: Case, L):
    """dove_amd.lib.ConvDesc of the case with 1 for every non-null pointer: what the library's reporting entry points need."""
    d = desc(c)
    q = L.ConvDesc()
    for f in ("nb", "t_in", "h_in", "w_in", "cin", "t_out", "h_out", "w_out", "cout_pad", "cout_store", "kt", "kh", "kw", "stride", "pad_h",
              "pad_w", "up", "tmode", "act", "ldo", "ldr", "gate_split", "tdup"):
        setattr(q, f, d[f])
    q.out_f32 = int(d["out_f32"])
    q.x = q.w = q.out = 1
    for f in ("resid", "gate", "w_first", "w_sub", "w_pair"):
        setattr(q, f, 1 if d[f] else None)
    q.cache = 1 if d["cached"] else None
    q.bias = 1 if c.bias else None
    return q


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------
def select_kernel(d: dict) -> str:
    nb = max(d["nb"], 1)
    M = nb * d["t_out"] * d["h_out"] * d["w_out"]
    pointwise = (d["kt"] == 1 and d["kh"] == 1 and d["kw"] == 1 and d["stride"] == 1 and d["up"] == 0 and d["tmode"] == 0
                 and d["t_in"] == d["t_out"] and d["h_in"] == d["h_out"] and d["w_in"] == d["w_out"])
    if pointwise and d["cin"] == 32 and d["act"] == 0 and not d["resid"] and not d["gate"] and d["cout_store"] >= 128:
        return "smallk"
    if pointwise and d["cout_pad"] % 128 == 0 and M >= 4096:
        if (d["cout_pad"] % 256 == 0 and d["cout_store"] % 256 == 0 and d["cin"] % 128 == 0 and d["cin"] >= 256 and d["ldo"] < (1 << 20)
                and d["ldr"] < (1 << 20) and d["act"] in (0, 1)):
            return "gemm8p"
    conv3 = (d["kh"] == 3 and d["kw"] == 3 and d["stride"] == 1 and d["pad_h"] == 1 and d["pad_w"] == 1 and d["act"] == 0 and not d["gate"]
             and d["cout_pad"] % 128 == 0)
    if conv3:
        same = d["up"] == 0 and d["tmode"] == 0 and d["h_out"] == d["h_in"] and d["w_out"] == d["w_in"] and d["w_out"] >= 16 and d["h_out"] >= 16
        ups = (d["up"] == 1 and d["kt"] == 1 and d["h_out"] == 2 * d["h_in"] and d["w_out"] == 2 * d["w_in"] and d["h_out"] >= 16
               and d["w_out"] >= 32)
        h4 = d["cout_store"] % 128 == 0 and d["cin"] % 64 == 0
        if same and h4:
            return "halo4x"
        if ups and h4 and d["w_sub"] and d["h_in"] >= 16 and d["w_in"] >= 32:
            return "halo4x_sub"
        if ups and h4:
            return "halo4x_up"
    return "igemm_fast" if d["up"] == 0 else "igemm"


KERNEL_NAME = {"smallk": "smallk_kernel", "gemm8p": "gemm8p_kernel", "halo4x": "conv3x3_halo4x_kernel", "halo4x_up": "conv3x3_halo4x_kernel",
               "halo4x_sub": "conv3x3_halo4x_kernel", "igemm_fast": "igemm_fast_kernel", "igemm": "igemm_kernel"}


def gemm_tail_split(d: dict, cus: int):
    """(rows_main | None, reason)"""
    M = d["t_out"] * d["h_out"] * d["w_out"]
    if d["t_out"] != 1 or d["h_out"] != 1 or max(d["nb"], 1) > 1:
        return None, "not_token_major"
    tiles_n = d["cout_pad"] // 256
    row_tiles = (M + 255) // 256
    ntiles = row_tiles * tiles_n
    if ntiles <= cus:
        return None, "le_cus"
    if ntiles % cus == 0:
        return None, "even"
    main_rt = (ntiles // cus) * cus // tiles_n
    if main_rt < 1 or main_rt >= row_tiles:
        return None, "main_rt"
    tail_rows = M - main_rt * 256
    if ((tail_rows + 127) // 128) * (d["cout_pad"] // 128) > 2 * cus:
        return None, "tail_blocks"
    return main_rt * 256, "taken"


def halo4x_plan(d: dict, cus: int) -> bool:
    tiles_w, tiles_h = (d["w_out"] + 31) // 32, (d["h_out"] + 15) // 16
    wrem = d["w_out"] % 32
    if wrem < 1 or wrem > 16:
        return False
    per = max(d["nb"], 1) * d["t_out"] * (d["cout_pad"] // 128)

    def rounds(tiles):
        return (tiles * per + cus - 1) // cus
    return rounds(tiles_h * (tiles_w - 1)) + rounds((d["h_out"] + 31) // 32) < rounds(tiles_h * tiles_w)


def gn_partial_rows(d: dict) -> int:
    k = select_kernel(d)
    if k not in ("halo4x", "halo4x_up", "halo4x_sub") or d["cout_store"] not in (128, 256, 512) or d["cout_store"] != d["cout_pad"]:
        return 0
    nb = max(d["nb"], 1)
    if k == "halo4x_sub":
        return nb * d["t_out"] * ((d["h_in"] + 15) // 16) * ((d["w_in"] + 31) // 32) * 16
    return nb * d["t_out"] * ((d["h_out"] + 15) // 16) * ((d["w_out"] + 31) // 32) * 4


def _tpw(ntiles, cus):
    if ntiles < cus:
        return "lt1"
    if ntiles == cus:
        return "1"
    return "multi" if ntiles % cus == 0 else "multi_off"


def _fast_key(d: dict) -> list:
    BN = 128 if d["cout_pad"] % 128 == 0 else (64 if d["cout_pad"] % 64 == 0 else 32)
    BK = 64 if d["cin"] % 64 == 0 else 32
    nk = d["kt"] * d["kh"] * d["kw"] * d["cin"] // BK
    twl = 7
    if d["h_out"] > 1:
        twl = 4 if d["w_out"] > 8 else (3 if d["w_out"] > 4 else 2)
    stride = "1" if d["stride"] == 1 else ("2even" if d["h_in"] % 2 == 0 and d["w_in"] % 2 == 0 else "2odd")
    front = "kt1" if d["kt"] == 1 else ("cache" if d["cached"] else "frame0")
    epi = "".join(ch for ch, on in (("a", d["act"] == 1), ("r", d["resid"]), ("g", d["gate"]), ("f", d["out_f32"])) if on) or "plain"
    key = [f"inst={BN}x{BK}", "nk=" + ("1" if nk == 1 else "2" if nk == 2 else "odd" if nk & 1 else "even"), f"tw={twl}", f"stride={stride}",
           f"front={front}", "nb=" + ("1" if d["nb"] <= 1 else "n"), f"epi={epi}"]
    if d["cout_store"] < d["cout_pad"]:
        key.append("st<pad")
    if d["cout_store"] % 8:
        key.append("st%8")
    return key


def _rem(v, m):
    r = v % m
    if r == 0:
        return "0"
    if m == 16:
        return "1..15"
    return "1..16" if r <= 16 else "17..31"


def class_key(c: Case, cus: int = 256) -> tuple:
    from dove_amd.ops import temporal_split
    d = desc(c)
    kern = select_kernel(d)
    nb = max(d["nb"], 1)
    M = nb * d["t_out"] * d["h_out"] * d["w_out"]
    key = [kern]
    if kern == "smallk":
        last = M % 128 or 128
        key.append("last=" + ("lt32" if last < 32 else "full" if last == 128 else "ragged" if last % 32 else "wave"))
        cs = d["cout_store"]
        key.append("cout=" + ("c128" if cs == 128 else "c256k" if cs % 256 == 0 else "ragged_y2" if cs > 256 else "lt256"))
        key.append(f"bias={int(c.bias)}")
    elif kern == "gemm8p":
        rows_main, why = gemm_tail_split(d, cus)
        Ml = rows_main if rows_main else M
        tiles_n = d["cout_pad"] // 256
        row_tiles = (Ml + 255) // 256
        last = Ml - (row_tiles - 1) * 256
        key.append("inst=" + ("gate" if d["gate"] else "gelu" if d["act"] == 1 else "plain_resid" if d["resid"] else "plain"))
        nk4 = d["cin"] // 128
        key.append("nk4=" + ("4+" if nk4 >= 4 else str(nk4)))
        key.append("last=" + ("1" if last == 1 else "le128" if last <= 128 else "129" if last == 129 else "full" if last == 256 else "mid"))
        t = _tpw(row_tiles * tiles_n, cus)
        key.append("tpw=" + ("1" if t in ("lt1", "1") else t))
        key.append("gm=" + ("1" if tiles_n <= 16 else "8full" if row_tiles % 8 == 0 else "8ragged"))
        key.append(f"split={why}")
        if d["gate"]:
            gs = d["gate_split"]
            key.append("gsplit=" + ("nosplit" if not rows_main else "main" if gs < rows_main else "edge" if gs == rows_main else "tail"))
        if rows_main:
            t = dict(d)
            t["w_in"] = t["w_out"] = M - rows_main
            key.append("tail=" + ",".join(_fast_key(t)))
        if c.cout < d["cout_store"]:
            key.append("cout<st")
        if c.inplace:
            key.append("inplace")
        if M * d["ldo"] * 2 > (256 << 20):
            key.append("nt_out")
        if d["ldo"] > d["cout_store"]:
            key.append("ldo>st")
    elif kern == "halo4x":
        key.append(f"kt={d['kt']}")
        if d["kt"] == 1:
            route, splits = "kt1", {0}
        else:
            route = (("tdup1_cache" if d["cached"] else "tdup1_nocache") if d["tdup"] == 1 else "tdup2" if d["tdup"] == 2 else
                     "cache" if d["cached"] else "nocache_wfirst" if d["w_first"] else "nocache_plain")
            names = {("w0", "w1", "w2"): 0, ("w012",): 1, ("w01", "w2"): 2, ("w0", "w12"): 3}
            splits = {names[tuple(w for w, _ in temporal_split(tl, d["tdup"], d["cached"], d["w_first"]))] for tl in range(d["t_out"])}
        key.append(f"route={route}")
        key.append("splits=" + "".join(str(s) for s in sorted(splits)))
        key.append("nb=" + ("1" if nb == 1 else "n_strided" if c.cache == "s" else "n"))
        key.append(f"kcn={d['cin'] // 32}")
        key.append(f"ctiles={d['cout_pad'] // 128}")
        key.append("hrem=" + _rem(d["h_out"], 16))
        key.append("wrem=" + _rem(d["w_out"], 32))
        if d["h_out"] == 16 and d["w_out"] == 16:
            key.append("min16")
        part = halo4x_plan(d, cus)
        tiles_h, tiles_w = (d["h_out"] + 15) // 16, (d["w_out"] + 31) // 32
        ntiles = nb * d["t_out"] * tiles_h * (tiles_w - (1 if part else 0)) * (d["cout_pad"] // 128)
        key.append("tpw=" + _tpw(ntiles, cus))
        if ntiles % 8:
            key.append("xcdrem")
        key.append("part=" + ("0" if not part else "1cut" if d["h_out"] % 32 else "1"))
        key.append("resid=" + ("0" if not d["resid"] else "ld>" if d["ldr"] > d["cout_store"] else "ld="))
        key.append("ldo=" + (">" if d["ldo"] > d["cout_store"] else "="))
        key.append("gn=" + (str(d["cout_store"]) if c.gn and gn_partial_rows(d) and d["ldo"] == d["cout_store"] else "0"))
    elif kern in ("halo4x_up", "halo4x_sub"):
        key.append(f"tmode={d['tmode']}")
        if kern == "halo4x_up":
            key.append("why=" + ("no_wsub" if not d["w_sub"] else "lowres_small"))
            key += ["hrem=" + _rem(d["h_out"], 16), "wrem=" + _rem(d["w_out"], 32)]
        else:
            key += ["hrem=" + _rem(d["h_in"], 16), "wrem=" + _rem(d["w_in"], 32)]
        key += [f"ctiles={d['cout_pad'] // 128}", f"kcn={d['cin'] // 32}"]
    elif kern == "igemm_fast":
        key += _fast_key(d)
    else:
        BN = 128 if d["cout_pad"] % 128 == 0 else (64 if d["cout_pad"] % 64 == 0 else 32)
        key += [f"tmode={d['tmode']}", f"inst={BN}x{64 if d['cin'] % 64 == 0 else 32}"]
    return tuple(key)


def partial_launches(c: Case, cus: int = 256) -> int:
    d = desc(c)
    return int(select_kernel(d) == "halo4x" and halo4x_plan(d, cus))


# ---- the classes every table must hold: (kernel, fields that one case's key must contain together) -----------------------------------------
REQUIRED = (
    [("smallk", f) for f in (["last=lt32"], ["last=ragged"], ["last=wave"], ["last=full"], ["cout=c128"], ["cout=lt256"], ["cout=ragged_y2"], ["cout=c256k"], ["bias=0"], ["bias=1"])]
    + [("gemm8p", f) for f in (
        ["inst=plain"], ["inst=gelu"], ["inst=gate"], ["inst=plain_resid"], ["nk4=2"], ["nk4=3"], ["nk4=4+"], ["last=1"], ["last=le128"],
        ["last=129"], ["last=full"], ["tpw=1"], ["tpw=multi"], ["tpw=multi_off"], ["gm=1"], ["gm=8full"], ["gm=8ragged"], ["cout<st"],
        ["split=taken"], ["split=not_token_major"], ["split=le_cus"], ["split=even"], ["split=tail_blocks"], ["gsplit=main"], ["gsplit=edge"],
        ["gsplit=tail"], ["inplace"], ["nt_out"], ["split=taken", "inst=gelu"])]
    + [("halo4x", f) for f in (
        ["kt=1"], ["kt=3"], ["route=cache"], ["route=nocache_wfirst", "splits=012"], ["route=nocache_plain"], ["route=tdup1_cache", "splits=23"],
        ["route=tdup1_nocache", "splits=123"], ["route=tdup2", "splits=123"], ["nb=n_strided"], ["nb=n", "gn=128"], ["kcn=2"], ["kcn=4"], ["kcn=16"], ["ctiles=1"],
        ["ctiles=2"], ["ctiles=4"], ["hrem=0"], ["hrem=1..15"], ["wrem=0"], ["wrem=1..16"], ["wrem=17..31"], ["min16"], ["tpw=lt1"], ["tpw=1"],
        ["tpw=multi_off"], ["xcdrem"], ["part=1"], ["part=1cut"], ["resid=ld>"], ["resid=ld="], ["ldo=>"], ["gn=128"], ["gn=256"], ["gn=512"])]
    + [("halo4x_up", f) for f in (["tmode=0"], ["tmode=1"], ["tmode=2"], ["why=lowres_small"], ["why=no_wsub"], ["hrem=1..15"], ["wrem=1..16"])]
    + [("halo4x_sub", f) for f in (["tmode=0"], ["tmode=1"], ["tmode=2"], ["hrem=1..15"], ["wrem=1..16"], ["hrem=0", "wrem=0"], ["ctiles=2"])]
    + [("igemm_fast", f) for f in (
        ["inst=128x64"], ["inst=128x32"], ["inst=64x64"], ["inst=64x32"], ["inst=32x64"], ["inst=32x32"], ["nk=1"], ["nk=2"], ["nk=odd"],
        ["nk=even"], ["tw=7"], ["tw=4"], ["tw=3"], ["tw=2"], ["stride=2even"], ["stride=2odd"], ["front=cache"], ["front=frame0"], ["nb=n"],
        ["epi=a"], ["epi=r"], ["epi=rg"], ["epi=f"], ["inst=64x32", "st<pad"], ["inst=32x64", "st<pad"], ["st%8"])]
    + [("igemm", f) for f in (["tmode=0"], ["tmode=1"], ["tmode=2"])]
)
# cases that sit one step outside a kernel's shape rule and must dispatch elsewhere: name -> kernel
NEAR_MISSES = {"sk_miss_cout64": "igemm_fast", "sk_miss_act": "igemm_fast", "sk_miss_resid": "igemm_fast", "g_miss_m4095": "igemm_fast",
               "g_miss_cin192": "igemm_fast", "g_miss_cout252": "igemm_fast", "h_miss_h15": "igemm_fast", "h_miss_cin32": "igemm_fast"}


def missing_classes(cases, cus: int = 256):
    keys = [class_key(c, cus) for c in cases]
    return [(k, f) for k, f in REQUIRED if not any(key[0] == k and all(x in key[1:] for x in f) for key in keys)]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def _lin(name, M, cin, cout, **kw):
    return Case(name, cin, cout, (1, 1, 1), 1, 1, M, **kw)


P1, C2, C3 = (1, 1, 1), (1, 3, 3), (3, 3, 3)
UP = dict(up=1, pad=(1, 1))
_ROWS = [
    # ---- smallk: SpatialNorm's conv_y || conv_b on the 16-channel latent (Cin_pad 32)
    Case("sk_lt32", 16, 128, P1, 1, 4, 5),
    Case("sk_ragged_y2", 16, 384, P1, 1, 2, 99),
    Case("sk_full_nobias", 16, 512, P1, 1, 16, 16, bias=False),
    Case("sk_wave_c256", 16, 256, P1, 1, 8, 24),
    Case("sk_lt256", 16, 192, P1, 1, 3, 50),
    Case("sk_miss_cout64", 16, 64, P1, 1, 4, 5),
    Case("sk_miss_act", 16, 128, P1, 1, 4, 5, act=1),
    Case("sk_miss_resid", 16, 128, P1, 1, 4, 5, resid=True),
    # ---- gemm8p
    _lin("g_plain_1row", 4097, 256, 256),
    _lin("g_gelu_le128", 4224, 384, 256, act=1),
    _lin("g_gate_129", 4225, 512, 256, gate=True, gate_split=1400),
    _lin("g_resid_full", 4096, 256, 256, resid=True),
    _lin("g_gelu_nk4_129", 4225, 512, 256, act=1),
    _lin("g_cout254", 4096, 256, 254),
    _lin("g_gate_inplace", 4097, 256, 256, gate=True, gate_split=4000, inplace=True),
    _lin("g_ldo_nt_out", 4096, 256, 256, ldo_x=32772 - 256),
    _lin("g_gm8_split", 4096, 256, 4352),
    Case("g_gm8_full_off", 256, 4352, P1, 1, 2, 2048),
    _lin("g_even_512tiles", 32768, 256, 1024, sampled=True),
    _lin("g_split_gate_main", 16500, 256, 1024, gate=True, gate_split=5000, inplace=True),
    _lin("g_split_gate_edge", 16500, 256, 1024, gate=True, gate_split=16384),
    _lin("g_split_gate_tail", 16500, 256, 1024, gate=True, gate_split=16384 + 50),
    _lin("g_split_gelu", 16500, 256, 1024, act=1),
    _lin("g_tail_blocks_off", 26500, 256, 1024),
    _lin("g_miss_m4095", 4095, 256, 256),
    _lin("g_miss_cin192", 4096, 192, 256),
    _lin("g_miss_cout252", 4096, 256, 252),
    # ---- conv3x3_halo4x, plain form
    Case("h_min16", 64, 128, C2, 1, 16, 16),
    Case("h_cache_2ct", 128, 256, C3, 2, 20, 37, cache="c"),
    Case("h_wfirst", 64, 128, C3, 3, 17, 50),
    Case("h_nocache_plain", 64, 128, C3, 2, 16, 33, wsums=False),
    Case("h_tdup1_cache", 64, 128, C3, 4, 16, 32, cache="c", tdup=1),
    Case("h_tdup1_nocache", 64, 128, C3, 4, 18, 20, tdup=1),
    Case("h_tdup2", 64, 128, C3, 5, 16, 40, tdup=2),
    Case("h_nb2_strided", 64, 128, C3, 2, 17, 33, nb=2, cache="s", resid=True),
    Case("h_kcn16_4ct", 512, 512, C2, 1, 16, 32),
    Case("h_one_round", 64, 128, C2, 64, 17, 33),
    Case("h_multi_off", 64, 128, C2, 65, 17, 33),
    Case("h_kpart_cut", 64, 128, C2, 128, 56, 40, sampled=True),
    Case("h_kpart_uncut", 64, 128, C2, 128, 64, 40, sampled=True),
    Case("h_resid_ldr", 64, 128, C2, 2, 19, 35, resid=True, ldr_x=4),
    Case("h_ldo", 128, 128, C3, 2, 16, 48, cache="c", ldo_x=4),
    Case("h_gn128", 64, 128, C2, 2, 20, 40, gn=True),
    Case("h_gn256_resid", 64, 256, C3, 2, 17, 33, cache="c", resid=True, gn=True),
    Case("h_gn512", 64, 512, C2, 1, 16, 32, gn=True),
    Case("h_nb2_gn", 64, 128, C3, 2, 16, 32, nb=2, cache="c", gn=True),
    Case("h_miss_h15", 64, 128, C2, 2, 15, 40),
    Case("h_miss_cin32", 3, 128, C3, 2, 16, 16),
    # ---- <kUp>: the upsample folded into the addressing
    Case("u_t0_lowres_small", 128, 128, C2, 2, 9, 17, gn=True, **UP),
    Case("u_t1_no_wsub", 64, 128, C2, 2, 16, 32, tmode=1, t_out=4, wsums=False, **UP),
    Case("u_t2_2ct", 64, 256, C2, 3, 12, 20, tmode=2, t_out=5, **UP),
    # ---- <kSub>: the sub-pixel form
    Case("s_t0_ragged", 128, 128, C2, 1, 17, 37, gn=True, **UP),
    Case("s_t1_exact", 64, 128, C2, 2, 16, 32, tmode=1, t_out=4, **UP),
    Case("s_t2_2ct", 64, 256, C2, 3, 18, 40, tmode=2, t_out=5, **UP),
    Case("s_t0_gn256", 64, 256, C2, 1, 16, 33, gn=True, **UP),
    # ---- igemm_fast
    _lin("f_32x32_nk1", 70, 32, 32),
    Case("f_64x64_nk2_tw4", 128, 64, P1, 2, 9, 11),
    _lin("f_128x64_nk1", 300, 64, 128),
    _lin("f_128x64_nk2_gate", 129, 128, 128, gate=True, gate_split=43),
    _lin("f_128x32_odd_gelu", 200, 96, 128, act=1),
    _lin("f_64x64_even_resid", 130, 256, 64, resid=True),
    Case("f_64x32_st60_tw3", 16, 60, P1, 2, 5, 7),
    Case("f_32x64_st24_tw2", 64, 24, P1, 2, 3, 4),
    Case("f_32x32_f32_cache", 32, 28, (3, 1, 1), 2, 6, 20, cache="c", out_f32=True, bias=False),
    Case("f_s2_even", 128, 128, C2, 2, 16, 20, stride=2, pad=(0, 0)),
    Case("f_s2_odd", 64, 64, C2, 2, 15, 9, stride=2, pad=(0, 0)),
    Case("f_kt3_frame0", 128, 128, C3, 3, 8, 12),
    Case("f_kt3_cache_nb2", 64, 64, C3, 2, 6, 10, nb=2, cache="c"),
    # ---- igemm (legacy): upsample-fused convs too small for the halo tile
    Case("l_up_t0", 128, 128, C2, 2, 6, 9, **UP),
    Case("l_up_t1", 64, 64, C2, 2, 6, 8, tmode=1, t_out=4, **UP),
    Case("l_up_t2", 96, 32, C2, 3, 5, 8, tmode=2, t_out=5, **UP),
]
# name -> (k of the budget, expected class_key at 256 CUs): literals, checked by tests/test_igemm_cases_cpu.py
_FT = "inst=128x64,nk=even,tw=7,stride=1,front=kt1,nb=1,epi="    # the igemm_fast tail of a split K = 256 GEMM
_H1 = "halo4x/kt=1/route=kt1/splits=0/nb=1/"
_H3 = "halo4x/kt=3/route="
_FA = "/stride=1/front=kt1/nb=1/epi="
EXPECT = {   # k = 16 k_chain rounded up to three digits; the trailing comment is the measured k_chain
    "sk_lt32": (17.9, "smallk/last=lt32/cout=c128/bias=1"),   # 1.116
    "sk_ragged_y2": (27.8, "smallk/last=ragged/cout=ragged_y2/bias=1"),   # 1.735
    "sk_full_nobias": (32.6, "smallk/last=full/cout=c256k/bias=0"),   # 2.035
    "sk_wave_c256": (26.6, "smallk/last=wave/cout=c256k/bias=1"),   # 1.660
    "sk_lt256": (31.5, "smallk/last=lt32/cout=lt256/bias=1"),   # 1.963
    "sk_miss_cout64": (19.5, "igemm_fast/inst=64x32/nk=1/tw=3" + _FA + "plain"),   # 1.216
    "sk_miss_act": (1.0, "igemm_fast/inst=128x32/nk=1/tw=3" + _FA + "a"),   # 0.000 (inside the GELU term)
    "sk_miss_resid": (23.8, "igemm_fast/inst=128x32/nk=1/tw=3" + _FA + "r"),   # 1.483
    "g_plain_1row": (16.5, "gemm8p/inst=plain/nk4=2/last=1/tpw=1/gm=1/split=le_cus"),   # 1.031
    "g_gelu_le128": (3.17, "gemm8p/inst=gelu/nk4=3/last=le128/tpw=1/gm=1/split=le_cus"),   # 0.198
    "g_gate_129": (19.4, "gemm8p/inst=gate/nk4=4+/last=129/tpw=1/gm=1/split=le_cus/gsplit=nosplit"),   # 1.207
    "g_resid_full": (17.7, "gemm8p/inst=plain_resid/nk4=2/last=full/tpw=1/gm=1/split=le_cus"),   # 1.102
    "g_gelu_nk4_129": (2.21, "gemm8p/inst=gelu/nk4=4+/last=129/tpw=1/gm=1/split=le_cus"),   # 0.138
    "g_cout254": (17.7, "gemm8p/inst=plain/nk4=2/last=full/tpw=1/gm=1/split=le_cus/cout<st"),   # 1.104
    "g_gate_inplace": (23.0, "gemm8p/inst=gate/nk4=2/last=1/tpw=1/gm=1/split=le_cus/gsplit=nosplit/inplace"),   # 1.435
    "g_ldo_nt_out": (17.3, "gemm8p/inst=plain/nk4=2/last=full/tpw=1/gm=1/split=le_cus/nt_out/ldo>st"),   # 1.081
    "g_gm8_split": (22.1, "gemm8p/inst=plain/nk4=2/last=full/tpw=1/gm=8ragged/split=taken/tail=" + _FT + "plain"),   # 1.375
    "g_gm8_full_off": (19.8, "gemm8p/inst=plain/nk4=2/last=full/tpw=multi_off/gm=8full/split=not_token_major"),   # 1.235
    "g_even_512tiles": (18.8, "gemm8p/inst=plain/nk4=2/last=full/tpw=multi/gm=1/split=even"),   # 1.173
    "g_split_gate_main": (21.4, "gemm8p/inst=gate/nk4=2/last=full/tpw=1/gm=1/split=taken/gsplit=main/tail=" + _FT + "rg/inplace"),   # 1.332
    "g_split_gate_edge": (22.5, "gemm8p/inst=gate/nk4=2/last=full/tpw=1/gm=1/split=taken/gsplit=edge/tail=" + _FT + "rg"),   # 1.401
    "g_split_gate_tail": (22.4, "gemm8p/inst=gate/nk4=2/last=full/tpw=1/gm=1/split=taken/gsplit=tail/tail=" + _FT + "rg"),   # 1.396
    "g_split_gelu": (3.5, "gemm8p/inst=gelu/nk4=2/last=full/tpw=1/gm=1/split=taken/tail=" + _FT + "a"),   # 0.219
    "g_tail_blocks_off": (23.4, "gemm8p/inst=plain/nk4=2/last=mid/tpw=multi_off/gm=1/split=tail_blocks"),   # 1.462
    "g_miss_m4095": (21.4, "igemm_fast/inst=128x64/nk=even/tw=7" + _FA + "plain"),   # 1.332
    "g_miss_cin192": (25.1, "igemm_fast/inst=128x64/nk=odd/tw=7" + _FA + "plain"),   # 1.568
    "g_miss_cout252": (23.4, "igemm_fast/inst=128x64/nk=even/tw=7" + _FA + "plain/st<pad/st%8"),   # 1.457
    "h_min16": (16.6, _H1 + "kcn=2/ctiles=1/hrem=0/wrem=1..16/min16/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 1.034
    "h_cache_2ct": (16.2, _H3 + "cache/splits=0/nb=1/kcn=4/ctiles=2/hrem=1..15/wrem=1..16/tpw=lt1/part=0/resid=0/ldo==/gn=0"),   # 1.008
    "h_wfirst": (15.8, _H3 + "nocache_wfirst/splits=012/nb=1/kcn=2/ctiles=1/hrem=1..15/wrem=17..31/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 0.984
    "h_nocache_plain": (14.1, _H3 + "nocache_plain/splits=0/nb=1/kcn=2/ctiles=1/hrem=0/wrem=1..16/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 0.878
    "h_tdup1_cache": (14.0, _H3 + "tdup1_cache/splits=23/nb=1/kcn=2/ctiles=1/hrem=0/wrem=0/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 0.869
    "h_tdup1_nocache": (20.3, _H3 + "tdup1_nocache/splits=123/nb=1/kcn=2/ctiles=1/hrem=1..15/wrem=17..31/tpw=lt1/part=0/resid=0/ldo==/gn=0"),   # 1.266
    "h_tdup2": (20.1, _H3 + "tdup2/splits=123/nb=1/kcn=2/ctiles=1/hrem=0/wrem=1..16/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 1.250
    "h_nb2_strided": (12.7, _H3 + "cache/splits=0/nb=n_strided/kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=lt1/part=0/resid=ld=/ldo==/gn=0"),   # 0.790
    "h_kcn16_4ct": (13.2, _H1 + "kcn=16/ctiles=4/hrem=0/wrem=0/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 0.824
    "h_one_round": (18.3, _H1 + "kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=1/part=0/resid=0/ldo==/gn=0"),   # 1.138
    "h_multi_off": (17.9, _H1 + "kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=multi_off/xcdrem/part=0/resid=0/ldo==/gn=0"),   # 1.113
    "h_kpart_cut": (16.0, _H1 + "kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=multi/part=1cut/resid=0/ldo==/gn=0"),   # 0.999
    "h_kpart_uncut": (16.2, _H1 + "kcn=2/ctiles=1/hrem=0/wrem=1..16/tpw=multi/part=1/resid=0/ldo==/gn=0"),   # 1.007
    "h_resid_ldr": (15.0, _H1 + "kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=lt1/part=0/resid=ld>/ldo==/gn=0"),   # 0.931
    "h_ldo": (13.0, _H3 + "cache/splits=0/nb=1/kcn=4/ctiles=1/hrem=0/wrem=1..16/tpw=lt1/xcdrem/part=0/resid=0/ldo=>/gn=0"),   # 0.808
    "h_gn128": (13.4, _H1 + "kcn=2/ctiles=1/hrem=1..15/wrem=1..16/tpw=lt1/part=0/resid=0/ldo==/gn=128"),   # 0.835
    "h_gn256_resid": (13.2, _H3 + "cache/splits=0/nb=1/kcn=2/ctiles=2/hrem=1..15/wrem=1..16/tpw=lt1/part=0/resid=ld=/ldo==/gn=256"),   # 0.820
    "h_gn512": (15.6, _H1 + "kcn=2/ctiles=4/hrem=0/wrem=0/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=512"),   # 0.973
    "h_nb2_gn": (14.1, _H3 + "cache/splits=0/nb=n/kcn=2/ctiles=1/hrem=0/wrem=0/tpw=lt1/xcdrem/part=0/resid=0/ldo==/gn=128"),   # 0.876
    "h_miss_h15": (19.0, "igemm_fast/inst=128x64/nk=odd/tw=4" + _FA + "plain"),   # 1.185
    "h_miss_cin32": (32.0, "igemm_fast/inst=128x32/nk=odd/tw=4/stride=1/front=frame0/nb=1/epi=plain"),   # 1.998
    "u_t0_lowres_small": (16.0, "halo4x_up/tmode=0/why=lowres_small/hrem=1..15/wrem=1..16/ctiles=1/kcn=4"),   # 0.999
    "u_t1_no_wsub": (15.8, "halo4x_up/tmode=1/why=no_wsub/hrem=0/wrem=0/ctiles=1/kcn=2"),   # 0.987
    "u_t2_2ct": (15.6, "halo4x_up/tmode=2/why=lowres_small/hrem=1..15/wrem=1..16/ctiles=2/kcn=2"),   # 0.973
    "s_t0_ragged": (18.7, "halo4x_sub/tmode=0/hrem=1..15/wrem=1..16/ctiles=1/kcn=4"),   # 1.168
    "s_t1_exact": (17.3, "halo4x_sub/tmode=1/hrem=0/wrem=0/ctiles=1/kcn=2"),   # 1.078
    "s_t2_2ct": (20.5, "halo4x_sub/tmode=2/hrem=1..15/wrem=1..16/ctiles=2/kcn=2"),   # 1.280
    "s_t0_gn256": (19.6, "halo4x_sub/tmode=0/hrem=0/wrem=1..16/ctiles=2/kcn=2"),   # 1.223
    "f_32x32_nk1": (18.6, "igemm_fast/inst=32x32/nk=1/tw=7" + _FA + "plain"),   # 1.160
    "f_64x64_nk2_tw4": (17.5, "igemm_fast/inst=64x64/nk=2/tw=4" + _FA + "plain"),   # 1.092
    "f_128x64_nk1": (18.1, "igemm_fast/inst=128x64/nk=1/tw=7" + _FA + "plain"),   # 1.128
    "f_128x64_nk2_gate": (17.0, "igemm_fast/inst=128x64/nk=2/tw=7" + _FA + "rg"),   # 1.061
    "f_128x32_odd_gelu": (1.42, "igemm_fast/inst=128x32/nk=odd/tw=7" + _FA + "a"),   # 0.089
    "f_64x64_even_resid": (17.2, "igemm_fast/inst=64x64/nk=even/tw=7" + _FA + "r"),   # 1.069
    "f_64x32_st60_tw3": (20.8, "igemm_fast/inst=64x32/nk=1/tw=3" + _FA + "plain/st<pad/st%8"),   # 1.297
    "f_32x64_st24_tw2": (9.67, "igemm_fast/inst=32x64/nk=1/tw=2" + _FA + "plain/st<pad"),   # 0.604
    "f_32x32_f32_cache": (16.7, "igemm_fast/inst=32x32/nk=odd/tw=4/stride=1/front=cache/nb=1/epi=f/st<pad/st%8"),   # 1.043
    "f_s2_even": (15.8, "igemm_fast/inst=128x64/nk=even/tw=4/stride=2even/front=kt1/nb=1/epi=plain"),   # 0.982
    "f_s2_odd": (16.6, "igemm_fast/inst=64x64/nk=odd/tw=2/stride=2odd/front=kt1/nb=1/epi=plain"),   # 1.031
    "f_kt3_frame0": (14.6, "igemm_fast/inst=128x64/nk=even/tw=4/stride=1/front=frame0/nb=1/epi=plain"),   # 0.907
    "f_kt3_cache_nb2": (13.4, "igemm_fast/inst=64x64/nk=odd/tw=4/stride=1/front=cache/nb=n/epi=plain"),   # 0.834
    "l_up_t0": (21.3, "igemm/tmode=0/inst=128x64"),   # 1.330
    "l_up_t1": (18.8, "igemm/tmode=1/inst=64x64"),   # 1.174
    "l_up_t2": (19.9, "igemm/tmode=2/inst=32x32"),   # 1.240
}
CASES = [dataclasses.replace(c, kk=EXPECT[c.name][0], key=EXPECT[c.name][1]) for c in _ROWS]


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(hash_key("igemm", *key))


def operands(c: Case, family: str) -> dict:
    """CPU operands of a case: x [nb T, H, W, cin_pad] bf16 (pad channels zero), cache [nb, kt-1, H, W, cin_pad] | None, pc (the product's
    PackedConv, packed on the CPU), resid [frames, Ho, Wo, ldr] bf16 | None, gate [2, cout_pad] fp32 | None."""
    from dove_amd import ops
    d = desc(c)
    kt, kh, kw = c.k
    g = _gen(c.name, family)
    shift = 3.0 if family == "offset" else 0.0
    assert family in FAMILIES

    def frames(n):
        t = torch.zeros(n, c.H, c.W, d["cin"])
        t[..., :c.cin] = torch.randn(n, c.H, c.W, c.cin, generator=g) + shift
        return t.to(BF)
    if c.tdup == 1:
        assert c.T % 2 == 0
        x = torch.cat([frames(c.T // 2).repeat_interleave(2, dim=0) for _ in range(c.nb)])
    elif c.tdup == 2:
        assert c.T % 2 == 1
        x = torch.cat([(lambda s: torch.cat([s[:1], s[1:].repeat_interleave(2, dim=0)]))(frames(1 + c.T // 2)) for _ in range(c.nb)])
    else:
        x = frames(c.nb * c.T)
    cache = None
    if c.cache:
        cache = frames(c.nb * (kt - 1)).view(c.nb, kt - 1, c.H, c.W, d["cin"])
        if c.tdup == 1:
            cache = cache[:, :1].expand(-1, 2, -1, -1, -1).contiguous()
    w = torch.randn(c.cout, c.cin, kt, kh, kw, generator=g) * (c.cin * kt * kh * kw) ** -0.5
    b = 0.1 * torch.randn(c.cout, generator=g) if c.bias else None
    pc = ops.pack_conv(w, b, "cpu", sub=True, pair=bool(c.tdup))
    nfr = c.nb * d["t_out"]
    resid = gate = None
    if d["resid"]:
        resid = torch.randn(nfr, d["h_out"], d["w_out"], d["ldr"], generator=g).to(BF)
    if c.gate:
        gate = 0.3 * torch.randn(2, d["cout_pad"], generator=g) + torch.tensor([0.6, -1.3])[:, None]
    return dict(x=x, cache=cache, pc=pc, resid=resid, gate=gate)


# ---- the float64 reference and the fp32 chain -----------------------------------------------------------------------------------------------
def _tmap(tl, tmode):
    return tl if tmode == 0 else (tl >> 1 if tmode == 1 else (0 if tl == 0 else 1 + ((tl - 1) >> 1)))


def _tables(pc):
    t = {}
    sp = pc.kh * pc.kw
    w = pc.w.double().view(pc.kt, sp, pc.cout_pad, pc.cin_pad)
    if pc.kt == 3:
        t.update(w0=w[0], w1=w[1], w2=w[2])
        wf = pc.w_first.double()
        t.update(w01f=wf[0], w012=wf[1])
        if pc.w_pair is not None:
            wp = pc.w_pair.double()
            t.update(w01p=wp[0], w12=wp[1])
    else:
        t["w"] = w[0]
        if pc.w_sub is not None:
            t["sub"] = pc.w_sub.double()
    return t


def _frame_groups(c, d, kern, tl, mut):
    """Temporal groups of local output frame tl: [(table name, source frame; negative = before the instance's first frame)]."""
    from dove_amd.ops import temporal_split
    if d["kt"] == 1:
        tm = d["tmode"]
        if mut == "tmode_swap" and tm:
            tm = 3 - tm
        return [("w", min(_tmap(tl, tm), c.T - 1))]
    if kern != "halo4x":
        return [("w0", tl - 2), ("w1", tl - 1), ("w2", tl)]
    tdup = d["tdup"]
    if mut == "tdup2_as_1" and tdup == 2:
        tdup = 1
    tq = tl ^ 1 if (mut == "wpair_parity" and tdup and tl >= 2) else tl
    groups = temporal_split(tq, tdup, d["cached"], d["w_first"])
    if tq != tl:
        groups = [(wn, fv + (tl - tq)) for wn, fv in groups]
    out = []
    for wn, fv in groups:
        if wn == "w01":
            wn = "w01p" if d["tdup"] else "w01f"
        if mut == "wfirst_swap" and wn in ("w01f", "w012"):
            wn = "w012" if wn == "w01f" else "w01f"
        out.append((wn, fv))
    return out


def _src(c, inp, b, fv, mut):
    if fv >= 0:
        return inp["x"][b * c.T + fv]
    if inp["cache"] is not None and mut != "front_frame0":
        return inp["cache"][b, c.k[0] - 1 + fv]
    if mut == "front_other" and inp["cache"] is None:
        # the reverse of front_frame0: a front that is NOT the replicated frame 0 where no cache exists (a stale cache pointer).  Frame 1 stands
        # in for it: the cases this mutant is listed for have T >= 2, no tdup and independent random frames, so frame 1 differs from frame 0
        return inp["x"][b * c.T + min(1, c.T - 1)]
    return inp["x"][b * c.T]


def _gather(src, d, oh, ow, dh, dw, mut):
    """[n, C] float64: the input pixels tap (dh, dw) reads for output pixels (oh, ow); zero outside the (upsampled) image."""
    Hl, Wl = src.shape[0] << d["up"], src.shape[1] << d["up"]
    org = 1 if (mut == "stride_origin" and d["stride"] == 2) else 0
    uh, uw = oh * d["stride"] - d["pad_h"] + dh + org, ow * d["stride"] - d["pad_w"] + dw + org
    ok = (uh >= 0) & (uh < Hl) & (uw >= 0) & (uw < Wl)
    if mut == "border_kept" and dh == 0 and dw == 1:
        ok = (uh >= -1) & (uh < Hl) & (uw >= 0) & (uw < Wl)     # the row above the image reads row 0 instead of zero
    if mut == "border_zeroed" and dh == 2 and dw == 1:
        ok = ok & (uh < Hl - 1)                                    # the image's last row is dropped for one tap
    ih, iw = uh.clamp(0, Hl - 1) >> d["up"], uw.clamp(0, Wl - 1) >> d["up"]
    return src[ih, iw].double() * ok[:, None]


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


def sample_rows(c: Case, cus: int = 256):
    """Flat pixel indices (over frames x Ho x Wo) a sampled case is checked at: the first and last tile in every direction, the rows around
    rows_main and gate_split, and N_RANDOM_SAMPLES random rows.  None: the case is checked everywhere."""
    if not c.sampled:
        return None
    d = desc(c)
    F, Ho, Wo = c.nb * d["t_out"], d["h_out"], d["w_out"]
    n = F * Ho * Wo
    pick = [torch.randint(0, n, (N_RANDOM_SAMPLES,), generator=_gen("rows", c.name))]
    if Ho == 1 and F == 1:
        marks = [0, n - 256, d["gate_split"] - 2]
        rm, _ = gemm_tail_split(d, cus)
        if rm:
            marks += [rm - 2, rm - 256]
        for m in marks:
            pick.append(torch.arange(max(m, 0), min(max(m, 0) + 260, n)))
    else:
        idx = torch.arange(n).view(F, Ho, Wo)
        th, tw = 32, 32                                             # covers the 16 x 32 and the 32 x 16 tile
        for f in (0, F - 1):
            for hs in (slice(0, th), slice(Ho - th, Ho)):
                pick.append(idx[f, hs, :].reshape(-1))              # whole rows: every tile column, the partial column included
            pick.append(idx[f, :, Wo - 16:].reshape(-1))
            pick.append(idx[f, :, :tw].reshape(-1))
    return torch.unique(torch.cat(pick))


def reference64(c: Case, inp: dict, rows=None, mut: str | None = None, chain: bool = False, cus: int = 256):
    """(ref, mag, gterm [, chain32]) float64 [n, cout_store] over the flat output pixels `rows` (None: all, in order).  `mut` names one
    deliberately wrong restatement (tests/test_igemm_cases_cpu.py).  `chain`: also the fp32 chain restatement of the kernel's K order
    (the un-rounded fp32 value the epilogue would hand to the output rounding)."""
    d = desc(c)
    kern = select_kernel(d)
    pc = inp["pc"]
    tabs = _tables(pc)
    cs, Cp = d["cout_store"], d["cin"]
    Ho, Wo, To = d["h_out"], d["w_out"], d["t_out"]
    F = c.nb * To
    if rows is None:
        rows = torch.arange(F * Ho * Wo)
    ref = torch.zeros(len(rows), cs, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    acc32 = torch.zeros(len(rows), cs, dtype=torch.float32) if chain else None
    bias = pc.bias.double()[:cs] if pc.bias is not None else None
    if bias is not None and mut == "bias_quad":
        bias = torch.roll(pc.bias.double(), -4)[:cs]
    if chain and kern == "smallk" and bias is not None:
        acc32 += bias.float()
    fr = rows // (Ho * Wo)
    taps = [(dh, dw) for dh in range(d["kh"]) for dw in range(d["kw"])]
    for f in torch.unique(fr).tolist():
        sel = (fr == f).nonzero()[:, 0]
        pix = rows[sel] - f * Ho * Wo
        oh, ow = pix // Wo, pix % Wo
        b, tl = divmod(f, To)
        groups = _frame_groups(c, d, kern, tl, mut)
        if kern == "halo4x_sub":
            parts = [(ph, ((oh & 1) * 2 + (ow & 1) == ph).nonzero()[:, 0]) for ph in range(4)]
        else:
            parts = [(None, torch.arange(len(pix)))]
        for ph, psel in parts:
            if len(psel) == 0:
                continue
            A, Wm = [], []                                          # per temporal group: [n, ntap, C], [ntap, cout_pad, C]
            for wn, fv in groups:
                src = _src(c, inp, b, fv, mut) if d["kt"] > 1 else inp["x"][b * c.T + fv]
                if ph is None:
                    A.append(torch.stack([_gather(src, d, oh[psel], ow[psel], dh, dw, mut) for dh, dw in taps], dim=1))
                    Wm.append(tabs[wn])
                else:                                               # 2 x 2 taps on the low-res grid with the phase's summed weights
                    py, px = ph >> 1, ph & 1
                    ly, lx = oh[psel] >> 1, ow[psel] >> 1
                    cols = []
                    for a2 in range(2):
                        for b2 in range(2):
                            ih, iw = ly + py + a2 - 1, lx + px + b2 - 1
                            ok = (ih >= 0) & (ih < c.H) & (iw >= 0) & (iw < c.W)
                            cols.append(src[ih.clamp(0, c.H - 1), iw.clamp(0, c.W - 1)].double() * ok[:, None])
                    A.append(torch.stack(cols, dim=1))
                    Wm.append(tabs["sub"][ph ^ 1 if (mut == "sub_phase" and ph < 2) else ph])
            A = torch.stack(A, dim=1)                               # [n, G, ntap, C]
            Wm = torch.stack(Wm, dim=0)[:, :, :cs].contiguous()     # [G, ntap, cs, C]
            if mut == "drop_chunk":
                A = A.clone()
                A[:, 0, A.shape[2] // 2, Cp - 32:] = 0
            if kern.startswith("halo4x"):                           # group -> 32-channel chunk -> tap
                G, nt = A.shape[1], A.shape[2]
                A2 = A.view(-1, G, nt, Cp // 32, 32).permute(0, 1, 3, 2, 4).reshape(len(psel), -1)
                W2 = Wm.view(G, nt, cs, Cp // 32, 32).permute(0, 3, 1, 4, 2).reshape(-1, cs)
                blk = 32
            else:                                                   # tap -> chunk (K contiguous inside a tap)
                A2 = A.reshape(len(psel), -1)
                W2 = Wm.permute(0, 1, 3, 2).reshape(-1, cs)
                blk = {"gemm8p": 32, "smallk": 2}.get(kern, 16)
            at = sel[psel]
            ref[at] = A2 @ W2
            mag[at] = A2.abs() @ W2.abs()
            if chain:
                a32 = acc32[at]
                for k0 in range(0, A2.shape[1], blk):
                    a32 = a32 + (A2[:, k0:k0 + blk] @ W2[k0:k0 + blk]).float()
                acc32[at] = a32
    # ---- epilogue ----
    gterm = torch.zeros_like(ref)
    if bias is not None:
        ref = ref + bias
        mag = mag + bias.abs()
        if chain and kern != "smallk":
            acc32 = acc32 + bias.float()
    act = d["act"] == 1
    if mut == "gelu_missing":
        act = False
    if mut == "gelu_on_gate" and c.gate:
        act = True
    if act:
        pre = ref
        ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0))) if mut == "gelu_erf" else _gelu64(pre)
        mag = GELU_LIP * mag
        gterm = 32 * EPS24 * torch.maximum(pre.abs(), ref.abs())
        if chain:
            acc32 = torch.nn.functional.gelu(acc32, approximate="tanh")
    if d["resid"]:
        r = inp["resid"].reshape(-1, d["ldr"])[rows][:, :cs]
        if mut == "resid_after_round":
            ref = ref.to(BF).double()
        if c.gate:
            rm, _ = gemm_tail_split(d, cus) if kern == "gemm8p" else (None, "")
            split = d["gate_split"] + (1 if mut == "gate_off1" else 0)
            cls = rows >= split
            if mut == "gate_unshifted" and rm:
                cls = torch.where(rows >= rm, rows - rm >= d["gate_split"], cls)
            gg = inp["gate"].double()[:, :cs][cls.long()]
            ref = r.double() + gg * ref
            mag = r.double().abs() + gg.abs() * mag
            gterm = gg.abs() * gterm
            if chain:
                acc32 = r.float() + gg.float() * acc32
        else:
            ref = r.double() + ref
            mag = r.double().abs() + mag
            if chain:
                acc32 = r.float() + acc32
    if chain:
        return ref, mag, gterm, acc32
    return ref, mag, gterm


# fused GroupNorm partial sums (conv3x3_halo4x's gn_flush): a value passes through at most 32 sequential fp32 adds in its lane (4 tile rows x
# 4 store rounds x 2 elements), 1 add of the lane's two halves, 3 shuffle levels and up to 2 adds that join quads into a group = 38 roundings,
# plus one for the square; the classical bound for a sum is depth x 2^-24 x sum |terms|
K_GN = 40.0


def gn_partials64(c: Case, stored, mut: str | None = None, dtype=torch.float64):
    """(partials, mags) float64 [rows, 64]: per (frame, 16 x 32 tile of the conv's grid [, phase], 4-row slot) and group the (sum, sum of squares)
    of the STORED output values over the slot's pixels inside the image - dove_conv_gn_partial_rows' layout.  `stored`: [frames, Ho, Wo,
    cout_store].  mut "rows_past_edge": the tile's rows and columns past the image contribute (their nearest valid pixel's value)."""
    d = desc(c)
    kern = select_kernel(d)
    cs = d["cout_store"]
    v = stored.to(dtype)                                           # float32: an fp32 restatement in another summation order
    F = v.shape[0]
    if kern == "halo4x_sub":                                       # tiles of the LOW-RES grid, a row per phase
        v = v.view(F, c.H, 2, c.W, 2, cs).permute(0, 2, 4, 1, 3, 5).reshape(F * 4, c.H, c.W, cs)
    Hh, Ww = v.shape[1], v.shape[2]
    th, tw = (Hh + 15) // 16, (Ww + 31) // 32
    vp = torch.zeros(v.shape[0], th * 16, tw * 32, cs, dtype=dtype)
    vp[:, :Hh, :Ww] = v
    if mut == "rows_past_edge":
        ih, iw = torch.arange(th * 16).clamp(max=Hh - 1), torch.arange(tw * 32).clamp(max=Ww - 1)
        vp = v[:, ih][:, :, iw]
    t = vp.view(-1, th, 4, 4, tw, 32, 32, cs // 32)              # [frame, tile row, slot, row, tile col, col, group, channel]

    def red(x):
        x = x.sum(dim=(3, 5, 7))                                  # [frame, th, slot, tw, group]
        if kern == "halo4x_sub":
            return x.view(F, 4, th, 4, tw, 32).permute(0, 2, 4, 1, 3, 5).reshape(-1, 32)
        return x.permute(0, 1, 3, 2, 4).reshape(-1, 32)
    s1, s2, m1 = red(t), red(t * t), red(t.abs())
    return torch.stack([s1, s2], dim=2).reshape(-1, 64), torch.stack([m1, s2], dim=2).reshape(-1, 64)


def ulp_out(ref, f32=False):
    """Unit in the last place of the output format at |ref| (bf16: 8 significand bits; fp32: 24), floored at the smallest normal binade."""
    e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1].double() - 1
    return torch.exp2(e - (23 if f32 else 7))


def budget(c: Case, ref, mag, gterm, k=None):
    return 0.5 * ulp_out(ref, c.out_f32) + (c.kk if k is None else k) * EPS24 * mag + gterm


def k_of(err, mag, gterm):
    """max (err - gterm) / (2^-24 mag); elements of zero magnitude must be exact."""
    z = mag == 0
    assert bool((err[z] == 0).all()), "an element that sums nothing is not zero"
    if bool(z.all()):
        return 0.0
    return float(((err - gterm).clamp_min(0)[~z] / (EPS24 * mag[~z])).max())
