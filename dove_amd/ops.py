"""torch-tensor front end of the C-ABI operators (allocation + argument marshalling only; all arithmetic is
in libdove_hip.so).  Activations are channels-last bf16: [T,H,W,C] (VAE) or [N,C] (DiT tokens)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as L


def _ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass
class PackedConv:
    """Weights repacked for the implicit-GEMM kernel: [taps][cout_pad][cin_pad] bf16, bias fp32 [cout_pad]."""
    w: torch.Tensor
    bias: torch.Tensor | None
    kt: int
    kh: int
    kw: int
    cin: int
    cin_pad: int
    cout: int
    cout_pad: int
    # kt == 3: [2][kh*kw][cout_pad][cin_pad] temporal sums w0 + w1 and w0 + w1 + w2 of the bf16 weights (fp32 sums, one rounding): what a causal
    # conv without a cache needs for its first two output frames, whose early taps all read the replicated frame 0 (dove_conv_desc.w_first)
    w_first: torch.Tensor | None = None
    # 3x3, kt == 1: [4 phases][2x2 taps][cout_pad][cin_pad] - the sub-pixel form of an upsample-fused conv (dove_conv_desc.w_sub): per output
    # phase the 3x3 weights summed over the taps that read the same low-res pixel (fp32 sums of the bf16 weights, one rounding)
    w_sub: torch.Tensor | None = None
    # kt == 3, on request: [2][kh*kw][cout_pad][cin_pad] - w0 + w1 and w1 + w2 for a conv whose input frames come in bit-identical pairs
    # (dove_conv_desc.w_pair / tdup: the first causal conv behind Upsample3D's time doubling); fp32 sums of the bf16 weights, one rounding
    w_pair: torch.Tensor | None = None

    @property
    def cout_store(self) -> int:
        return _ru(self.cout, 4)


def pack_conv(weight: torch.Tensor, bias: torch.Tensor | None, device, *, sub: bool = True, pair: bool = False) -> PackedConv:
    """weight: Conv3d [Cout,Cin,kt,kh,kw], Conv2d [Cout,Cin,kh,kw] or Linear [Cout,Cin] (any float dtype).
    ``sub``: build the sub-pixel sums of a 3x3 Conv2d (only an upsample-fused use reads them: the VAE passes False for its down-samplers);
    ``pair``: build the pair sums of a 3x3x3 conv (``conv(..., tdup=)``)."""
    w = weight.detach()
    if w.dim() == 2:
        w = w[:, :, None, None, None]
    elif w.dim() == 4:
        w = w[:, :, None]
    cout, cin, kt, kh, kw = w.shape
    cin_pad = _ru(cin, 32) if cin <= 32 or cin % 64 else cin
    cout_pad = _ru(cout, 32)
    wp = torch.zeros(kt * kh * kw, cout_pad, cin_pad, dtype=torch.bfloat16, device=device)
    wp[:, :cout, :cin] = w.to(device=device, dtype=torch.float32).permute(2, 3, 4, 0, 1).reshape(kt * kh * kw, cout, cin).to(torch.bfloat16)
    bp = None
    if bias is not None:
        bp = torch.zeros(cout_pad, dtype=torch.float32, device=device)
        bp[:cout] = bias.detach().to(device=device, dtype=torch.float32)
    wp = wp.contiguous()
    w_first = None
    if kt == 3:
        t = wp.float().view(3, kh * kw, cout_pad, cin_pad)
        s01 = t[0] + t[1]
        w_first = torch.stack([s01, s01 + t[2]]).to(torch.bfloat16).contiguous()
    w_pair = None
    if kt == 3 and pair:
        t = wp.float().view(3, kh * kw, cout_pad, cin_pad)
        w_pair = torch.stack([t[0] + t[1], t[1] + t[2]]).to(torch.bfloat16).contiguous()
    w_sub = None
    if kt == 1 and kh == 3 and kw == 3 and sub:
        t = wp.float().view(3, 3, cout_pad, cin_pad)
        w_sub = torch.zeros(4, 4, cout_pad, cin_pad, dtype=torch.float32, device=device)
        for py in range(2):
            for px in range(2):
                for dh in range(3):                       # fixed summation order (csrc/graph.hip pack_sub_kernel: the same)
                    for dw in range(3):
                        a, b = (py + dh + 1) // 2 - py, (px + dw + 1) // 2 - px
                        w_sub[2 * py + px, 2 * a + b] += t[dh, dw]
        w_sub = w_sub.to(torch.bfloat16).contiguous()
    return PackedConv(wp, bp, kt, kh, kw, cin, cin_pad, cout, cout_pad, w_first, w_sub, w_pair)


def temporal_split(tl: int, tdup: int, cached: bool, first_sums: bool = True):
    """Host restatement of csrc/igemm.hip h4_split + h4_set_nxt: the temporal groups conv3x3_halo4x runs for output frame tl of an instance,
    as [(weights, source frame)] with weights in {"w0", "w1", "w2", "w01", "w12", "w012"} (tap blocks of w / their pack-time sums) and the
    source an instance frame index (negative: before the first frame = the conv cache, else frame 0 replicated).
    tdup 0: no declaration (only the cache-less first two frames split, when ``first_sums``); 1: frames are pairs (0,1), (2,3), ... and the
    cache too; 2: frame 0 single, then pairs (1,2), (3,4), ... (no cache)."""
    plain = [("w0", tl - 2), ("w1", tl - 1), ("w2", tl)]
    if tdup == 0:
        if cached or not first_sums or tl > 1:
            return plain
        return [("w012", 0)] if tl == 0 else [("w01", 0), ("w2", 1)]
    if tdup == 1:
        if not cached and tl < 2:
            return [("w012", tl)]
        return [("w0", tl - 2), ("w12", tl)] if tl & 1 else [("w01", tl - 1), ("w2", tl)]
    if tl == 0:
        return [("w012", 0)]
    return [("w01", tl - 1), ("w2", tl)] if tl & 1 else [("w0", tl - 2), ("w12", tl)]


def temporal_groups(tl: int, tdup: int, cached: bool) -> int:
    return len(temporal_split(tl, tdup, cached))


_profiler = None


def set_profiler(records: list | None):
    """bench.py hook: when a list is installed, every igemm launch appends (key, algorithmic_flops, ev_start, ev_end, kernel_name,
    issued_flops) with HIP events recorded on the launch stream (issued < algorithmic where a weight-summed form skips duplicate taps)."""
    global _profiler
    _profiler = records


def conv_kernel_name(x_shape, pc: PackedConv, *, stride=1, pad=(None, None), up=0, tmode=0, t_out=None, hw_out=None, act=0, gated=False,
                     resid=False, nb=1, partial=False):
    """Kernel a conv / linear of this shape dispatches to (dove_conv_kernel_name; pure function of the descriptor, no GPU needed).
    ``partial=True``: the partial-tile launch mask of the call instead (dove_conv_partial_launches: 1 = last tile column, 2 = last tile row);
    ``x_shape`` is per instance, ``nb`` instances."""
    T, H, W, Cx = x_shape
    d = L.ConvDesc()
    d.nb = nb
    ph = (pc.kh - 1) // 2 if pad[0] is None else pad[0]
    pw = (pc.kw - 1) // 2 if pad[1] is None else pad[1]
    t_out = T if t_out is None else t_out
    if hw_out is None:
        hw_out = (H << up, W << up) if stride == 1 else ((H + 1 - pc.kh) // stride + 1, (W + 1 - pc.kw) // stride + 1)
    d.t_in, d.h_in, d.w_in, d.cin = T, H, W, Cx
    d.t_out, d.h_out, d.w_out = t_out, hw_out[0], hw_out[1]
    d.cout_pad, d.cout_store = pc.cout_pad, pc.cout_store
    d.kt, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = pc.kt, pc.kh, pc.kw, stride, ph, pw
    d.up, d.tmode, d.act = up, tmode, act
    d.ldo = pc.cout_store
    d.ldr = pc.cout_store if resid else 0
    d.resid = 1 if (resid or gated) else None                  # only tested for NULL-ness by the selection rule
    d.w_sub = 1 if (up == 1 and pc.kt == 1 and pc.kh == 3 and pc.kw == 3) else None
    d.gate = 1 if gated else None
    if partial:
        return int(L.load().dove_conv_partial_launches(C.byref(d)))
    return L.load().dove_conv_kernel_name(C.byref(d)).decode()


def conv(x: torch.Tensor, pc: PackedConv, *, cache: torch.Tensor | None = None, stride: int = 1, pad=(None, None),
         up: int = 0, tmode: int = 0, t_out: int | None = None, hw_out=None, resid: torch.Tensor | None = None,
         gate: torch.Tensor | None = None, gate_split: int = 0, act: int = 0, ldo: int | None = None,
         out: torch.Tensor | None = None,
         gn_eps: float | None = None, out_f32: bool = False, nb: int = 1, tdup: int = 0, weight_sums: bool = True) -> torch.Tensor:
    """Implicit-GEMM conv on channels-last x [T,H,W,cin_pad] -> [t_out,h_out,w_out,ldo].

    ``gn_eps``: the output feeds an nn.GroupNorm(32, C, eps) (resnet norm1/norm2, SpatialNorm's norm_layer).  When the
    dispatched kernel can fuse the statistics into its epilogue (``dove_conv_gn_partial_rows`` > 0), they are computed
    there and attached to the returned tensor as ``out.gn_stats`` ([32,2] mean / rstd, fp32) - `groupnorm_stats_of`
    then skips the separate pass over the tensor; otherwise nothing is attached and the caller's path is unchanged.

    ``nb`` > 1: x holds nb independent instances back to back along the frame axis ([nb*T, H, W, C]; ``t_out`` stays the per-instance
    count) - the same-shaped tiles of the tiled VAE in one launch (include/dove_hip.h dove_conv_desc.nb).  ``cache`` is then
    [nb, kt-1, H, W, C], possibly a strided view (dim 0) of the previous frame-batch's input; statistics come back as [nb, 32, 2].

    ``tdup`` (kt == 3, ``pc.w_pair`` packed): the caller declares that every instance's frames come in bit-identical pairs - 1: (0,1), (2,3), ...
    and the cache too; 2: frame 0 single, then (1,2), (3,4), ..., no cache (include/dove_hip.h dove_conv_desc.tdup): two temporal groups per
    frame instead of three.  ``weight_sums=False``: none of the pack-time weight sums (w_first / w_sub / w_pair) is handed over - the launch
    computes the reference's per-tap arithmetic."""
    L.require_cuda(x, resid, gate, out)
    assert x.dtype == torch.bfloat16 and x.dim() == 4, (x.dtype, x.shape)
    T, H, W, Cx = x.shape
    assert T % nb == 0, (T, nb)
    T //= nb
    if Cx != pc.cin_pad:
        raise RuntimeError(f"conv: input has {Cx} channels, packed weight expects {pc.cin_pad}")
    ph = (pc.kh - 1) // 2 if pad[0] is None else pad[0]
    pw = (pc.kw - 1) // 2 if pad[1] is None else pad[1]
    if t_out is None:
        t_out = T
    if hw_out is None:
        hw_out = (H << up, W << up) if stride == 1 else ((H + 1 - pc.kh) // stride + 1, (W + 1 - pc.kw) // stride + 1)
    if ldo is None:
        ldo = pc.cout_store
    odt = torch.float32 if out_f32 else torch.bfloat16        # out_f32: un-rounded accumulators (tap-split conv_out, conv_out_gather)
    if out is None:
        out = torch.empty(nb * t_out, hw_out[0], hw_out[1], ldo, dtype=odt, device=x.device)
    else:
        assert out.shape == (nb * t_out, hw_out[0], hw_out[1], ldo) and out.dtype == odt
    cache_stride = 0
    if cache is not None:
        if nb > 1:
            assert cache.shape == (nb, pc.kt - 1, H, W, Cx) and cache.dtype == torch.bfloat16 and cache.is_cuda, (cache.shape, x.shape)
            assert cache[0].is_contiguous() and cache.device == x.device
            cache_stride = cache.stride(0)
        else:
            L.require_cuda(cache)
            assert cache.shape == (pc.kt - 1, H, W, Cx) and cache.dtype == torch.bfloat16, (cache.shape, x.shape)
    d = L.ConvDesc()
    d.nb, d.cache_stride = nb, cache_stride
    if cache is None and pc.w_first is not None and weight_sums:
        d.w_first = pc.w_first.data_ptr()
    if up == 1 and pc.w_sub is not None and weight_sums:
        d.w_sub = pc.w_sub.data_ptr()
    if tdup and weight_sums and pc.w_pair is not None and pc.kt == 3 and not (tdup == 2 and cache is not None):
        d.tdup, d.w_pair = tdup, pc.w_pair.data_ptr()
    d.x, d.cache, d.w = x.data_ptr(), (cache.data_ptr() if cache is not None else None), pc.w.data_ptr()
    d.bias = pc.bias.data_ptr() if pc.bias is not None else None
    d.resid = resid.data_ptr() if resid is not None else None
    d.gate = gate.data_ptr() if gate is not None else None
    d.out = out.data_ptr()
    d.t_in, d.h_in, d.w_in, d.cin = T, H, W, Cx
    d.t_out, d.h_out, d.w_out = t_out, hw_out[0], hw_out[1]
    d.cout_pad, d.cout_store = pc.cout_pad, pc.cout_store
    d.kt, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = pc.kt, pc.kh, pc.kw, stride, ph, pw
    d.up, d.tmode, d.act = up, tmode, act
    d.ldo = ldo
    d.ldr = resid.shape[-1] if resid is not None else 0
    d.gate_split = gate_split
    d.out_f32 = int(out_f32)
    if resid is not None:
        assert resid.dtype == torch.bfloat16 and resid.numel() == nb * t_out * hw_out[0] * hw_out[1] * resid.shape[-1]
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.shape == (2, pc.cout_pad)
    partial = None
    if gn_eps is not None and ldo == pc.cout_store:
        rows = int(L.load().dove_conv_gn_partial_rows(C.byref(d)))
        if rows > 0:
            partial = torch.empty(rows, 64, dtype=torch.float32, device=x.device)
            d.gn_partial = partial.data_ptr()
    if _profiler is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.check(L.load().dove_conv_igemm_bf16(C.byref(d), L.stream_ptr()), "dove_conv_igemm_bf16")
    if _profiler is not None:
        e1.record()
        flops = 2.0 * nb * t_out * hw_out[0] * hw_out[1] * pc.cout * pc.cin * pc.kt * pc.kh * pc.kw
        name = L.load().dove_conv_kernel_name(C.byref(d)).decode()
        # MFMA work actually issued: the ALGORITHMIC count above is the reference's formulation; the weight-summed forms skip taps whose
        # input is a duplicate (w_first: 2 + 1 of the first two frames' 3 + 3 temporal taps per instance; w_sub: 5 of 9 spatial taps)
        real = flops
        if name == "conv3x3_halo4x_kernel":
            if d.tdup and pc.kt == 3 and up == 0:
                real = flops * sum(temporal_groups(tl, d.tdup, cache is not None) for tl in range(t_out)) / (3.0 * t_out)
            elif d.w_first and pc.kt == 3 and up == 0:
                real = flops * (1.0 - (2.0 + (1.0 if t_out > 1 else 0.0)) / (3.0 * t_out))
            elif d.w_sub and up == 1 and H >= 16 and W >= 32:
                real = flops * 4.0 / 9.0
        _profiler.append(((pc.cin, pc.cout, pc.kt * pc.kh * pc.kw), flops, e0, e1, name, real))
    if partial is None:
        if getattr(out, "gn_stats", None) is not None:      # a re-used `out` tensor must not keep statistics of old contents
            out.gn_stats = None
            out.gn_rows = None
    else:
        count = float(t_out * hw_out[0] * hw_out[1]) * (pc.cout_store // 32)
        if nb > 1:
            stats = torch.empty(nb, 32, 2, dtype=torch.float32, device=x.device)
            ws = _ws(x.device, nb * 512)                       # nb x 256 rows of 64 doubles
            L.check(L.load().dove_groupnorm_finalize_partials_nb(partial.data_ptr(), partial.shape[0] // nb, nb, count, gn_eps, L.ptr(ws),
                                                                 ws.numel() * 4, L.ptr(stats), L.stream_ptr()), "dove_groupnorm_finalize_partials_nb")
        else:
            stats = torch.empty(32, 2, dtype=torch.float32, device=x.device)
            L.check(L.load().dove_groupnorm_finalize_partials(partial.data_ptr(), partial.shape[0], count, gn_eps, L.ptr(_ws(x.device)),
                                                              L.ptr(stats), L.stream_ptr()), "dove_groupnorm_finalize_partials")
        out.gn_stats = (stats, gn_eps, out._version)           # torch's in-place counter: a later torch write voids them
        out.gn_rows = partial                                  # raw per-tile sums: dove_amd.dist combines them across a rank pair
    return out


def groupnorm_stats_of(x: torch.Tensor, eps: float, nb: int = 1) -> torch.Tensor:
    """GroupNorm(32) statistics of x: the ones its producing conv already computed (``conv(..., gn_eps=eps)``), else a
    pass over x.  ``nb`` > 1: x is nb instances back to back, one statistics scope each ([nb, 32, 2])."""
    have = getattr(x, "gn_stats", None)
    if have is not None and have[1] == eps and have[2] == x._version and have[0].numel() == nb * 64:
        return have[0]
    return groupnorm_stats(x, eps, nb)


def linear(x: torch.Tensor, pc: PackedConv, **kw) -> torch.Tensor:
    """x [N, cin_pad] -> [N, ldo]."""
    N = x.shape[0]
    out = kw.pop("out", None)
    resid = kw.pop("resid", None)
    y = conv(x.view(1, 1, N, x.shape[1]), pc, resid=None if resid is None else resid.view(1, 1, N, resid.shape[1]),
             out=None if out is None else out.view(1, 1, N, out.shape[1]), **kw)
    return y.view(N, y.shape[-1])


_gn_ws: dict = {}
GN_WS_ROWS = 4096        # partial rows of scratch: 9 frames x 256 blocks per frame at most (csrc/norm.hip gn_partial_launch)


def _ws(device, rows: int = GN_WS_ROWS):
    # one scratch buffer per (device, stream): the two-stream VAE mode runs GroupNorm statistics concurrently.  It only ever grows
    # (launches that used the old buffer are ordered before anything that re-uses its memory on the same stream)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream if torch.cuda.is_available() else 0)
    rows = max(rows, GN_WS_ROWS)
    if key not in _gn_ws or _gn_ws[key].numel() < rows * 64:
        _gn_ws[key] = torch.empty(rows * 64, dtype=torch.float32, device=device)
    return _gn_ws[key]


def _gn_rows_needed(x, frames: int) -> int:
    """Partial rows csrc/norm.hip gn_partial_launch writes for `frames` frames of x's frame size (at most 256 blocks per frame)."""
    fp = _frame_pix(x) or x.numel() // x.shape[-1]
    nsub = 256 // max(x.shape[-1] // 8, 1)
    return frames * min(256, -(-fp // (max(nsub, 1) * 32)))


def _frame_pix(x):
    """H*W of a [T,H,W,C] frame-batch (0 = "one frame" for anything else): the statistics kernels sum per frame share."""
    return x.shape[1] * x.shape[2] if x.dim() == 4 else 0


def groupnorm_stats(x: torch.Tensor, eps: float, nb: int = 1) -> torch.Tensor:
    """x [T,H,W,C] (one frame-batch) -> stats [32,2] (mean, rstd) fp32; ``nb`` > 1: [nb*T,H,W,C] -> [nb,32,2], one scope per instance."""
    L.require_cuda(x)
    assert x.dtype == torch.bfloat16
    Cc = x.shape[-1]
    frames = x.shape[0] if x.dim() == 4 else 1
    ws = _ws(x.device, _gn_rows_needed(x, frames))
    if nb > 1:
        assert x.dim() == 4 and x.shape[0] % nb == 0
        stats = torch.empty(nb, 32, 2, dtype=torch.float32, device=x.device)
        L.check(L.load().dove_groupnorm_stats_nb_bf16(L.ptr(x), nb, x.numel() // Cc // nb, _frame_pix(x), Cc, eps, L.ptr(ws), ws.numel() // 64,
                                                      L.ptr(stats), L.stream_ptr()), "dove_groupnorm_stats_nb_bf16")
        return stats
    stats = torch.empty(32, 2, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_groupnorm_stats_bf16(L.ptr(x), x.numel() // Cc, _frame_pix(x), Cc, eps, L.ptr(ws), ws.numel() // 64, L.ptr(stats),
                                               L.stream_ptr()), "dove_groupnorm_stats_bf16")
    return stats


def groupnorm_sums(x: torch.Tensor) -> torch.Tensor:
    """Raw per-group (sum, sum of squares) of one piece of a frame-batch, fp64 [32,2] (dove_amd.dist adds the pieces)."""
    L.require_cuda(x)
    assert x.dtype == torch.bfloat16
    Cc = x.shape[-1]
    sums = torch.empty(32, 2, dtype=torch.float64, device=x.device)
    ws = _ws(x.device, _gn_rows_needed(x, x.shape[0] if x.dim() == 4 else 1))
    L.check(L.load().dove_groupnorm_sums_bf16(L.ptr(x), x.numel() // Cc, _frame_pix(x), Cc, L.ptr(ws), ws.numel() // 64, L.ptr(sums),
                                              L.stream_ptr()), "dove_groupnorm_sums_bf16")
    return sums


def groupnorm_sums_of(x: torch.Tensor) -> torch.Tensor:
    """``groupnorm_sums`` of x, from the partial rows its producing conv wrote when there are any (no pass over x)."""
    rows = getattr(x, "gn_rows", None)
    if rows is None:
        return groupnorm_sums(x)
    sums = torch.empty(32, 2, dtype=torch.float64, device=x.device)
    L.check(L.load().dove_groupnorm_sums_from_partials(L.ptr(rows), rows.shape[0], L.ptr(_ws(x.device)), L.ptr(sums), L.stream_ptr()),
            "dove_groupnorm_sums_from_partials")
    return sums


def groupnorm_from_sums(sums: torch.Tensor, count: float, eps: float) -> torch.Tensor:
    """stats [32,2] (mean, rstd) from summed fp64 (sum, sumsq) over ``count`` elements per group.  ``count=None``: sums is the
    65-double message of dove_amd.dist's pair exchange, whose last entry is the element count (read on the device)."""
    L.require_cuda(sums)
    assert sums.dtype == torch.float64 and (sums.shape == (32, 2) if count is not None else sums.numel() == 65)
    stats = torch.empty(32, 2, dtype=torch.float32, device=sums.device)
    L.check(L.load().dove_groupnorm_finalize_sums(L.ptr(sums.contiguous()), 0.0 if count is None else float(count), eps, L.ptr(stats), L.stream_ptr()),
            "dove_groupnorm_finalize_sums")
    return stats


def groupnorm_apply(x, stats, gamma, beta, *, silu=True, yb=None, sshift=0, tmap=None, out=None, nb=1):
    """y = silu?(GN(x) [* Y + B]) with the SpatialNorm3D table yb [Tz,hz,wz,2C] gathered by nearest resize.  ``nb`` > 1: x [nb*T,..],
    stats [nb,32,2], yb [nb*Tz,..], ``tmap`` the frame map of ONE instance."""
    L.require_cuda(x, stats, gamma, beta, yb, out)
    T, H, W, Cc = x.shape
    assert T % nb == 0 and stats.numel() == nb * 64
    T //= nb
    if out is None:
        out = torch.empty_like(x)
    Tz = hz = wz = 0
    tm = None
    if yb is not None:
        assert yb.dtype == torch.bfloat16 and yb.shape[-1] == 2 * Cc and tmap is not None and len(tmap) == T and yb.shape[0] % nb == 0
        Tz, hz, wz = yb.shape[0] // nb, yb.shape[1], yb.shape[2]
        tm = (C.c_int * T)(*tmap)
    L.check(L.load().dove_groupnorm_apply_nb_bf16(L.ptr(x), L.ptr(out), nb, T, H, W, Cc, L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                                  int(silu), L.ptr(yb), Tz, hz, wz, sshift, tm, L.stream_ptr()),
            "dove_groupnorm_apply_nb_bf16")
    return out


def layernorm_modulate(x, gamma, beta, eps, mod=None, split=0, out=None):
    L.require_cuda(x, gamma, beta, mod, out)
    assert x.dtype == torch.bfloat16 and x.dim() == 2
    if out is None:
        out = torch.empty_like(x)
    if mod is not None:
        assert mod.dtype == torch.float32 and mod.shape == (2, 2, x.shape[1])
    L.check(L.load().dove_layernorm_modulate_bf16(L.ptr(x), L.ptr(out), x.shape[0], x.shape[1], eps, L.ptr(gamma),
                                                  L.ptr(beta), L.ptr(mod), split, L.stream_ptr()),
            "dove_layernorm_modulate_bf16")
    return out


def qkv_post(qkv, N, Npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, eps, Qh, Kh, Vt, v_order=1, norm2=None):
    """``v_order=1``: V^T rows in the quad-swapped key order ``attention`` reads (include/dove_hip.h); 0 = natural (pieces that
    are assembled later and converted with ``vt_quad_swap``).  ``norm2`` (fp32 [heads, 2], optional): receives the max squared row
    norms of the stored q / k rows per head - the score bound ``attention`` can use instead of a running maximum."""
    L.require_cuda(qkv, gq, bq, gk, bk, cos, sin, Qh, Kh, Vt, norm2)
    if norm2 is not None:
        assert norm2.dtype == torch.float32 and norm2.shape == (heads, 2) and norm2.is_contiguous()
    L.check(L.load().dove_qkv_post_bf16(L.ptr(qkv), N, Npad, heads, 64, text_len, L.ptr(gq), L.ptr(bq), L.ptr(gk), L.ptr(bk),
                                        L.ptr(cos), L.ptr(sin), qscale, eps, L.ptr(Qh), L.ptr(Kh), L.ptr(Vt), v_order, L.ptr(norm2),
                                        L.stream_ptr()), "dove_qkv_post_bf16")


def vt_quad_swap(Vt):
    """[..., 64, Npad] V^T rows: natural <-> quad-swapped key order, in place."""
    L.require_cuda(Vt)
    assert Vt.is_contiguous()
    L.check(L.load().dove_vt_quad_swap_bf16(L.ptr(Vt), Vt.numel() // Vt.shape[-1], Vt.shape[-1], L.stream_ptr()), "dove_vt_quad_swap_bf16")
    return Vt


def ulysses_place(rq, rk, rv, counts, hloc, N, Npad, Qh, Kh, Vt, norm2_out=None):
    """Receive side of the Ulysses all-to-all (include/dove_hip.h dove_ulysses_place_bf16): per-source-rank blocks of my heads ->
    the attention kernel's head-major operands (V^T quad-swapped, pad columns zero) in one launch.  ``norm2_out`` (fp32 [hloc, 2]): the
    blocks carry one extra row per head and the K blocks' extra rows the ranks' score-bound pairs; their maximum is written here."""
    L.require_cuda(rq, rk, rv, Qh, Kh, Vt, norm2_out)
    if norm2_out is not None:
        assert norm2_out.dtype == torch.float32 and norm2_out.shape == (hloc, 2)
    cnt = (C.c_longlong * len(counts))(*[int(c) for c in counts])
    L.check(L.load().dove_ulysses_place_bf16(L.ptr(rq), L.ptr(rk), L.ptr(rv), cnt, len(counts), hloc, N, Npad, L.ptr(Qh), L.ptr(Kh), L.ptr(Vt),
                                             L.ptr(norm2_out), L.stream_ptr()), "dove_ulysses_place_bf16")


def attention(Qh, Kh, Vt, N, Npad, heads, out, norm2=None):
    """``norm2`` (fp32 [heads, 2], IN/OUT; from the ``qkv_post`` call that produced Qh / Kh - or the element-wise maximum over the ranks
    sharing the rows): heads with finite entries run on the software-pipelined no-shift kernel; a head whose row sums leave that kernel's
    safe window is marked NaN in ``norm2[h, 0]`` and recomputed with the running maximum inside the same call (include/dove_hip.h).  None:
    the running maximum in every head.  ``attention_head_paths(norm2)`` afterwards names the kernel that produced each head."""
    L.require_cuda(Qh, Kh, Vt, out, norm2)
    if norm2 is not None:
        assert norm2.dtype == torch.float32 and norm2.shape == (heads, 2) and norm2.is_contiguous()
    L.check(L.load().dove_attention_fwd_bf16(L.ptr(Qh), L.ptr(Kh), L.ptr(Vt), L.ptr(out), N, Npad, heads, 64, out.shape[1], L.ptr(norm2),
                                             L.stream_ptr()), "dove_attention_fwd_bf16")
    return out


def attention_head_paths(norm2, heads=None):
    """Kernel names, one per head, of the ``attention`` call that was handed ``norm2`` (read AFTER the call; synchronises).  ``norm2=None``
    with ``heads``: a call without bounds."""
    lib = L.load()
    if norm2 is None:
        host, n = None, int(heads)
    else:
        host = norm2.detach().float().cpu().contiguous()
        n = host.shape[0]
    path = (C.c_int * n)()
    L.check(lib.dove_attention_head_paths(None if host is None else C.cast(host.data_ptr(), C.POINTER(C.c_float)), n, path),
            "dove_attention_head_paths")
    return [lib.dove_attention_path_name(int(v)).decode() for v in path]


def qkv_post_mx(qkv, N, Npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, eps, Q8, K8, V8t, Vs):
    """dove_qkv_post_mxfp8: e4m3 attention operands (Q8, K8 [heads][Npad][64], V8t [heads][64][Npad] u8; Vs [heads][Npad/64][64][2] u8)."""
    L.require_cuda(qkv, gq, bq, gk, bk, cos, sin, Q8, K8, V8t, Vs)
    L.check(L.load().dove_qkv_post_mxfp8(L.ptr(qkv), N, Npad, heads, 64, text_len, L.ptr(gq), L.ptr(bq), L.ptr(gk), L.ptr(bk),
                                         L.ptr(cos), L.ptr(sin), qscale, eps, L.ptr(Q8), L.ptr(K8), L.ptr(V8t), L.ptr(Vs),
                                         L.stream_ptr()), "dove_qkv_post_mxfp8")


def attention_mx(Q8, K8, V8t, Vs, N, Npad, heads, out):
    L.require_cuda(Q8, K8, V8t, Vs, out)
    L.check(L.load().dove_attention_fwd_mxfp8(L.ptr(Q8), L.ptr(K8), L.ptr(V8t), L.ptr(Vs), L.ptr(out), N, Npad, heads, 64,
                                              out.shape[1], L.stream_ptr()), "dove_attention_fwd_mxfp8")
    return out


def cl_im2col3x3_from_ncthw(x: torch.Tensor, cp: int, scale=1.0, shift=0.0) -> torch.Tensor:
    """[C,T,H,W] -> [T,H,W,cp] bf16 with the 3x3 neighbourhood in the channels ((dy*3+dx)*C + c; zero outside the frame and beyond 9C)."""
    L.require_cuda(x)
    Cc, T, H, W = x.shape
    y = torch.empty(T, H, W, cp, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_cl_im2col3x3_from_ncthw(L.ptr(x), L.dt_code(x), Cc, T, H, W, cp, scale, shift, L.ptr(y), L.stream_ptr()),
            "dove_cl_im2col3x3_from_ncthw")
    return y


def conv_out_gather(p: torch.Tensor, Cc: int, bias, dtype, scale=1.0, shift=0.0, lo=-math.inf, hi=math.inf) -> torch.Tensor:
    """Second half of the tap-split decoder.conv_out (include/dove_hip.h dove_conv_out_gather): p [T,H,W,ld] fp32 partial planes ->
    [Cc,T,H,W] ``dtype`` with the range map of ``ncthw_from_cl``."""
    L.require_cuda(p, bias)
    assert p.dtype == torch.float32 and p.dim() == 4
    T, H, W, ld = p.shape
    y = torch.empty(Cc, T, H, W, dtype=dtype, device=p.device)
    L.check(L.load().dove_conv_out_gather(L.ptr(p), ld, T, H, W, Cc, L.ptr(bias), scale, shift, lo, hi, L.ptr(y), L.dt_code(y),
                                          L.stream_ptr()), "dove_conv_out_gather")
    return y


def conv_out_gather_cl(p: torch.Tensor, Cc: int, bias, ld: int = 8) -> torch.Tensor:
    """The same gather for a spatial TILE (dove_conv_out_gather_cl): p [T,H,W,ldp] fp32 partial planes -> [T,H,W,ld] bf16 channels-last
    (channels >= Cc zero, no range map): tiles are cross-faded channels-last before the clip changes layout.  T may be nb x frames."""
    L.require_cuda(p, bias)
    assert p.dtype == torch.float32 and p.dim() == 4
    T, H, W, ldp = p.shape
    y = torch.empty(T, H, W, ld, dtype=torch.bfloat16, device=p.device)
    L.check(L.load().dove_conv_out_gather_cl(L.ptr(p), ldp, T, H, W, Cc, L.ptr(bias), L.ptr(y), ld, L.stream_ptr()), "dove_conv_out_gather_cl")
    return y


def tile_gather(x: torch.Tensor, t0: int, nt: int, th: int, tw: int, origins, im2col_cin: int = 0) -> torch.Tensor:
    """Same-shaped spatial tiles of a channels-last clip x [T,H,W,C] -> one tile-major batch [nb*nt, th, tw, C] (dove_tile_gather_bf16):
    frames [t0, t0+nt), tile n at origins[n] = (oy, ox).  ``im2col_cin`` > 0: x is the im2col'ed clip (cl_im2col3x3_from_ncthw) and the
    channels of taps that reach outside a tile are zeroed at its border (diffusers' tiles see zero padding at their own border)."""
    import ctypes as C
    L.require_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 4
    T, H, W, Cc = x.shape
    nb = len(origins)
    oy = (C.c_int * nb)(*[int(o[0]) for o in origins])
    ox = (C.c_int * nb)(*[int(o[1]) for o in origins])
    assert 0 <= t0 and t0 + nt <= T
    y = torch.empty(nb * nt, th, tw, Cc, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_tile_gather_bf16(L.ptr(x), H, W, Cc, t0, nt, th, tw, nb, oy, ox, im2col_cin, L.ptr(y), L.stream_ptr()),
            "dove_tile_gather_bf16")
    return y


def cl_from_ncthw(x: torch.Tensor, cp: int, scale=1.0, shift=0.0) -> torch.Tensor:
    """[C,T,H,W] fp32/bf16 -> [T,H,W,cp] bf16 (zero-padded channels)."""
    L.require_cuda(x)
    Cc, T, H, W = x.shape
    y = torch.empty(T, H, W, cp, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_cl_from_ncthw(L.ptr(x), L.dt_code(x), Cc, T * H * W, cp, scale, shift, L.ptr(y), L.stream_ptr()),
            "dove_cl_from_ncthw")
    return y


def ncthw_from_cl(x: torch.Tensor, Cc: int, dtype, scale=1.0, shift=0.0, lo=-math.inf, hi=math.inf) -> torch.Tensor:
    """[T,H,W,ld] bf16 -> [Cc,T,H,W] dtype, y = clamp(x*scale+shift, lo, hi)."""
    L.require_cuda(x)
    T, H, W, ld = x.shape
    y = torch.empty(Cc, T, H, W, dtype=dtype, device=x.device)
    L.check(L.load().dove_ncthw_from_cl(L.ptr(x), ld, Cc, T * H * W, scale, shift, lo, hi, L.ptr(y), L.dt_code(y),
                                        L.stream_ptr()), "dove_ncthw_from_cl")
    return y


def avgpool_time(x: torch.Tensor, nb: int = 1) -> torch.Tensor:
    """Downsample3D's temporal pool; ``nb`` > 1: x is nb instances [nb*T, H, W, C], pooled per instance."""
    L.require_cuda(x)
    T, H, W, Cc = x.shape
    assert T % nb == 0
    T //= nb
    if T == 1:
        return x
    To = 1 + (T - 1) // 2 if T % 2 else T // 2
    y = torch.empty(nb * To, H, W, Cc, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_avgpool_time_nb_bf16(L.ptr(x), nb, T, H * W * Cc, L.ptr(y), L.stream_ptr()), "dove_avgpool_time_nb_bf16")
    return y


def posterior_sample(moments_cl: torch.Tensor, latent_channels: int, noise: torch.Tensor, dtype) -> torch.Tensor:
    """moments [T,h,w,>=2L] bf16 + noise [L,T,h,w] -> sample [L,T,h,w] dtype."""
    L.require_cuda(moments_cl, noise)
    T, h, w, ld = moments_cl.shape
    out = torch.empty(latent_channels, T, h, w, dtype=dtype, device=noise.device)
    L.check(L.load().dove_posterior_sample(L.ptr(moments_cl), ld, latent_channels, T * h * w, L.ptr(noise), L.dt_code(noise),
                                           L.ptr(out), L.dt_code(out), L.stream_ptr()), "dove_posterior_sample")
    return out


def axpby(x, y, a: float, b: float):
    L.require_cuda(x, y)
    assert x.shape == y.shape and x.dtype == y.dtype
    out = torch.empty_like(x)
    L.check(L.load().dove_axpby(L.ptr(x), L.ptr(y), L.ptr(out), L.dt_code(x), x.numel(), a, b, L.stream_ptr()), "dove_axpby")
    return out


def patchify(x: torch.Tensor, pt: int, p: int, ld: int) -> torch.Tensor:
    """[T,C,h,w] -> tokens [Nv, ld] bf16 (features beyond C*pt*p*p zero)."""
    L.require_cuda(x)
    T, Cc, H, W = x.shape
    nv = (T // pt) * (H // p) * (W // p)
    feat = Cc * pt * p * p
    tok = (torch.zeros if ld > feat else torch.empty)(nv, ld, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_patchify(L.ptr(x), L.dt_code(x), T, Cc, H, W, pt, p, L.ptr(tok), ld, L.stream_ptr()), "dove_patchify")
    return tok


def unpatchify(tok: torch.Tensor, T, Cc, H, W, pt, p, dtype) -> torch.Tensor:
    L.require_cuda(tok)
    y = torch.empty(T, Cc, H, W, dtype=dtype, device=tok.device)
    L.check(L.load().dove_unpatchify(L.ptr(tok), tok.shape[1], T, Cc, H, W, pt, p, L.ptr(y), L.dt_code(y), L.stream_ptr()),
            "dove_unpatchify")
    return y


def gemv(W: torch.Tensor, bias, x: torch.Tensor, act_in: int = 0) -> torch.Tensor:
    """y = W @ act(x) + b for one vector; W [out,in] bf16, x fp32 [in] -> fp32 [out]."""
    L.require_cuda(W, bias, x)
    assert W.dtype == torch.bfloat16 and x.dtype == torch.float32 and x.numel() == W.shape[1]
    y = torch.empty(W.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.load().dove_gemv_bf16(L.ptr(W), L.ptr(bias), L.ptr(x), W.shape[1], W.shape[0], act_in, L.ptr(y), L.stream_ptr()),
            "dove_gemv_bf16")
    return y


def blend_edge(a: torch.Tensor, b: torch.Tensor, extent: int, axis: int) -> torch.Tensor:
    """diffusers blend_v (axis 0) / blend_h (axis 1) on channels-last tiles [T,H,W,ld], in place on b."""
    L.require_cuda(a, b)
    assert a.dtype == b.dtype == torch.bfloat16 and a.shape[0] == b.shape[0] and a.shape[3] == b.shape[3]
    L.check(L.load().dove_blend_edge_bf16(L.ptr(a), L.ptr(b), b.shape[0], a.shape[1], a.shape[2], b.shape[1], b.shape[2],
                                          b.shape[3], extent, axis, L.stream_ptr()), "dove_blend_edge_bf16")
    if getattr(b, "gn_stats", None) is not None:             # b changed in place: statistics its producing conv attached are stale
        b.gn_stats = None
        b.gn_rows = None
    return b


def preprocess_u8(frames: torch.Tensor, pad_f: int, pad_h: int, pad_w: int, upscale: int, dtype) -> torch.Tensor:
    """frames [F,H,W,3] uint8 -> [3, F+pad_f, (H+pad_h)*up, (W+pad_w)*up] dtype in [-1,1]."""
    L.require_cuda(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    F0, H0, W0, _ = frames.shape
    out = torch.empty(3, F0 + pad_f, (H0 + pad_h) * upscale, (W0 + pad_w) * upscale, dtype=dtype, device=frames.device)
    L.check(L.load().dove_preprocess_u8(L.ptr(frames), F0, H0, W0, pad_f, pad_h, pad_w, upscale, L.ptr(out), L.dt_code(out),
                                        L.stream_ptr()), "dove_preprocess_u8")
    return out


def postprocess_u8(video: torch.Tensor, Fo: int, Ho: int, Wo: int) -> torch.Tensor:
    """video [3,F,H,W] in [0,1] -> [Fo,Ho,Wo,3] uint8 (crop + x255 + truncate)."""
    L.require_cuda(video)
    _, F, H, W = video.shape
    out = torch.empty(Fo, Ho, Wo, 3, dtype=torch.uint8, device=video.device)
    L.check(L.load().dove_postprocess_u8(L.ptr(video), L.dt_code(video), F, H, W, Fo, Ho, Wo, L.ptr(out), L.stream_ptr()),
            "dove_postprocess_u8")
    return out


def _image_view(t: torch.Tensor) -> L.ImageView:
    codes = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.uint8: L.U8}
    if t.dtype not in codes:
        raise TypeError(f"image views are float32 / bfloat16 / uint8, got {t.dtype}")
    v = L.ImageView()
    v.data, v.dtype = t.data_ptr(), codes[t.dtype]
    v.sn, v.sc, v.sh, v.sw = t.stride()
    return v


def fr_metrics(pred: torch.Tensor, ref: torch.Tensor, flags: int) -> torch.Tensor:
    """pred, ref: [N,C,H,W] views (any strides, no copy) -> fp64 [N,2] {PSNR dB, SSIM} on the device (csrc/metrics.hip; NaN for a
    metric ``flags`` does not ask for)."""
    if pred.dim() != 4 or pred.shape != ref.shape:
        raise ValueError(f"fr_metrics: pred {tuple(pred.shape)} and ref {tuple(ref.shape)} must be the same [N,C,H,W] shape")
    if not (pred.is_cuda and ref.is_cuda) or pred.device != ref.device:
        raise RuntimeError("fr_metrics needs both images on the same HIP device (`cuda`); there is no CPU path")
    N, Cc, H, W = pred.shape
    lib = L.load()
    with torch.cuda.device(pred.device):
        ws = torch.empty(max(int(lib.dove_fr_metrics_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=pred.device)
        out = torch.empty(N, 2, dtype=torch.float64, device=pred.device)
        pv, rv = _image_view(pred), _image_view(ref)
        L.check(lib.dove_fr_metrics(C.byref(pv), C.byref(rv), N, Cc, H, W, flags, L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
                "dove_fr_metrics")
    return out


def niqe_features(img: torch.Tensor):
    """img: [N,C,H,W] view (any strides, no copy; uint8 / float32 / bfloat16, C in {1, 3}, H, W >= 96) -> (features fp64 [N,B,36],
    sharpness fp64 [N,B]) on the device, B = (H // 96) * (W // 96) blocks in row-major order (csrc/niqe.hip)."""
    if img.dim() != 4:
        raise ValueError(f"niqe_features: expected an [N,C,H,W] view, got shape {tuple(img.shape)}")
    if not img.is_cuda:
        raise RuntimeError("niqe_features needs the images on the HIP device (`cuda`); there is no CPU path")
    N, Cc, H, W = img.shape
    if H < 96 or W < 96:
        raise ValueError(f"niqe: H and W must be at least 96 (one 96 x 96 block), got {H} x {W}")
    B = (H // 96) * (W // 96)
    lib = L.load()
    with torch.cuda.device(img.device):
        ws = torch.empty(max(int(lib.dove_niqe_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=img.device)
        feats = torch.empty(N, B, 36, dtype=torch.float64, device=img.device)
        sharp = torch.empty(N, B, dtype=torch.float64, device=img.device)
        if N:
            v = _image_view(img)
            L.check(lib.dove_niqe_features(C.byref(v), N, Cc, H, W, L.ptr(ws), ws.numel(), L.ptr(feats), L.ptr(sharp), L.stream_ptr()),
                    "dove_niqe_features")
    return feats, sharp


def niqe_stats(features: torch.Tensor):
    """features: contiguous fp64 [N,B,36] on the device -> (mu fp64 [N,36], cov fp64 [N,36,36], counts int32 [N,2] = {blocks without a
    NaN, blocks with at least one non-NaN feature})."""
    if features.dim() != 3 or features.shape[2] != 36 or features.dtype != torch.float64 or features.shape[1] < 1:
        raise ValueError(f"niqe_stats: expected float64 [N,B>=1,36], got {tuple(features.shape)} {features.dtype}")
    L.require_cuda(features)
    N, B, _ = features.shape
    mu = torch.empty(N, 36, dtype=torch.float64, device=features.device)
    cov = torch.empty(N, 36, 36, dtype=torch.float64, device=features.device)
    counts = torch.empty(N, 2, dtype=torch.int32, device=features.device)
    if N:
        L.check(L.load().dove_niqe_stats(L.ptr(features), N, B, L.ptr(mu), L.ptr(cov), L.ptr(counts), L.stream_ptr()), "dove_niqe_stats")
    return mu, cov, counts


def niqe_distance(mu_a, cov_a, mu_b, cov_b) -> float:
    """sqrt(d pinv((cov_a + cov_b) / 2) d^T), d = mu_a - mu_b, of two 36-feature Gaussian models given as HOST float64 arrays (host code
    of the library: Jacobi eigen-solve, singular values at or below 36 eps sigma_max dropped).  NaN for a non-finite input."""
    import numpy as np
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (mu_a, cov_a, mu_b, cov_b)]
    for a, shape in zip(arrs, ((36,), (36, 36), (36,), (36, 36))):
        if a.shape != shape:
            raise ValueError(f"niqe_distance: expected shapes (36,), (36, 36), (36,), (36, 36), got {[x.shape for x in arrs]}")
    out = C.c_double(0.0)
    L.check(L.load().dove_niqe_distance(*(C.c_void_p(a.ctypes.data) for a in arrs), C.byref(out)), "dove_niqe_distance")
    return out.value


def color_fix(content: torch.Tensor, style: torch.Tensor, mode: int, out: torch.Tensor, clamp: bool = True,
              content_affine=(1.0, 0.0), style_affine=(1.0, 0.0)) -> torch.Tensor:
    """content, style, out: [N,3,H,W] views (any strides, no copy; float32 / bfloat16 / uint8) -> ``out`` filled with the colour fix of
    ``mode`` (L.COLORFIX_WAVELET / L.COLORFIX_ADAIN; csrc/colorfix.hip).  Each input is read as ``scale * raw + bias``."""
    if content.dim() != 4 or content.shape[1] != 3 or content.shape != style.shape or content.shape != out.shape:
        raise ValueError(f"color_fix: content {tuple(content.shape)}, style {tuple(style.shape)} and out {tuple(out.shape)} must be the "
                         "same [N,3,H,W] shape")
    if not (content.is_cuda and style.is_cuda and out.is_cuda) or content.device != style.device or content.device != out.device:
        raise RuntimeError("color_fix needs content, style and out on the same HIP device (`cuda`); there is no CPU path")
    N, _, H, W = content.shape
    lib = L.load()
    with torch.cuda.device(content.device):
        ws = torch.empty(max(int(lib.dove_color_fix_workspace_bytes(mode, N, H, W)), 8), dtype=torch.uint8, device=content.device)
        cv, sv, ov = _image_view(content), _image_view(style), _image_view(out)
        L.check(lib.dove_color_fix(C.byref(cv), content_affine[0], content_affine[1], C.byref(sv), style_affine[0], style_affine[1],
                                   N, H, W, mode, L.COLORFIX_CLAMP if clamp else 0, C.byref(ov), L.ptr(ws), ws.numel(), L.stream_ptr()),
                "dove_color_fix")
    return out


def yuv_frame_bytes(h: int, w: int, chroma: int) -> int:
    return int(L.load().dove_yuv_frame_bytes(h, w, chroma))


def rgb_to_yuv_u8(rgb: torch.Tensor, fmt: L.YuvFormat) -> torch.Tensor:
    """rgb: a [N,3,H,W] view (any strides, no copy; uint8, or float32 / bfloat16 in [0,1]) -> [N, frame_bytes] uint8 Y4M frame payloads
    (Y, U, V planes; csrc/yuv.hip).  ``fmt`` carries the forward matrix."""
    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb_to_yuv_u8: rgb {tuple(rgb.shape)} must be a [N,3,H,W] view")
    if not rgb.is_cuda:
        raise RuntimeError("rgb_to_yuv_u8 needs its input on the HIP device (`cuda`); there is no CPU path")
    N, _, H, W = rgb.shape
    lib = L.load()
    with torch.cuda.device(rgb.device):
        out = torch.empty(N, int(lib.dove_yuv_frame_bytes(H, W, fmt.chroma)), dtype=torch.uint8, device=rgb.device)
        v = _image_view(rgb)
        L.check(lib.dove_rgb_to_yuv_u8(C.byref(v), N, H, W, C.byref(fmt), L.ptr(out), L.stream_ptr()), "dove_rgb_to_yuv_u8")
    return out


def yuv_to_rgb_u8(payload: torch.Tensor, h: int, w: int, fmt: L.YuvFormat) -> torch.Tensor:
    """payload [N, frame_bytes] uint8 (contiguous Y4M frame payloads) -> [N,h,w,3] uint8 frames (csrc/yuv.hip).  ``fmt`` carries the inverse
    matrix."""
    L.require_cuda(payload)
    lib = L.load()
    fb = int(lib.dove_yuv_frame_bytes(h, w, fmt.chroma))
    if payload.dtype != torch.uint8 or payload.dim() != 2 or payload.shape[1] != fb or fb == 0:
        raise ValueError(f"yuv_to_rgb_u8: payload {tuple(payload.shape)} {payload.dtype} is not uint8 [N, {fb}] for {w}x{h}")
    N = payload.shape[0]
    out = torch.empty(N, h, w, 3, dtype=torch.uint8, device=payload.device)
    L.check(lib.dove_yuv_to_rgb_u8(L.ptr(payload), N, h, w, C.byref(fmt), L.ptr(out), L.stream_ptr()), "dove_yuv_to_rgb_u8")
    return out


def png_segment_rows(w: int, channels: int) -> int:
    """Rows of one deflate segment of the PNG encoder (host function; 0 for a bad argument)."""
    return int(L.load().dove_png_segment_rows(w, channels))


def png_bound(h: int, w: int, channels: int) -> int:
    """The most bytes one encoded h x w file can take (host function; 0 for a bad argument)."""
    return int(L.load().dove_png_bound(h, w, channels))


def png_encode(img: torch.Tensor):
    """img: a [N,C,H,W] view, C in {1, 3} (any strides, no copy; uint8, or float32 / bfloat16 in [0,1]) -> (files uint8 [N, png_bound],
    sizes int64 [N]) on the device: row i holds one complete PNG file in its first sizes[i] bytes (csrc/png.hip)."""
    if img.dim() != 4 or img.shape[1] not in (1, 3):
        raise ValueError(f"png_encode: img {tuple(img.shape)} must be a [N,1,H,W] or [N,3,H,W] view")
    if not img.is_cuda:
        raise RuntimeError("png_encode needs its input on the HIP device (`cuda`); there is no CPU path")
    N, Cc, H, W = img.shape
    lib = L.load()
    with torch.cuda.device(img.device):
        out = torch.empty(N, int(lib.dove_png_bound(H, W, Cc)), dtype=torch.uint8, device=img.device)
        sizes = torch.empty(N, dtype=torch.int64, device=img.device)
        if N:
            ws = torch.empty(max(int(lib.dove_png_workspace_bytes(N, H, W, Cc)), 8), dtype=torch.uint8, device=img.device)
            v = _image_view(img)
            L.check(lib.dove_png_encode(C.byref(v), N, H, W, Cc, L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(sizes), L.stream_ptr()),
                    "dove_png_encode")
    return out, sizes


def zlib_huffman(data: torch.Tensor, segment_bytes: int = 32768):
    """data: contiguous uint8 on the device -> (stream uint8 [bound], size int64 [1]) on the device: a zlib stream of literal-only
    dynamic-Huffman blocks, one per ``segment_bytes`` of input (the PNG encoder's deflate stage; csrc/png.hip)."""
    if data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError(f"zlib_huffman: expected a 1-D uint8 tensor, got {tuple(data.shape)} {data.dtype}")
    L.require_cuda(data)
    lib = L.load()
    n = data.numel()
    out = torch.empty(max(int(lib.dove_zlib_huffman_bound(n, segment_bytes)), 8), dtype=torch.uint8, device=data.device)
    ws = torch.empty(max(int(lib.dove_zlib_huffman_workspace_bytes(n, segment_bytes)), 8), dtype=torch.uint8, device=data.device)
    size = torch.empty(1, dtype=torch.int64, device=data.device)
    L.check(lib.dove_zlib_huffman(L.ptr(data), n, segment_bytes, L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(size), L.stream_ptr()),
            "dove_zlib_huffman")
    return out, size


JPEG_SUBSAMPLING = {"420": 0, "444": 1}                             # DOVE_JPEG_* of include/dove_hip.h


def jpeg_subsampling_code(subsampling) -> int:
    """'420' / '444' (or the DOVE_JPEG_* code itself) -> the code.  Host code: anything else raises ValueError."""
    if isinstance(subsampling, int) and not isinstance(subsampling, bool) and subsampling in JPEG_SUBSAMPLING.values():
        return subsampling
    if subsampling not in JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg subsampling {subsampling!r}: one of {sorted(JPEG_SUBSAMPLING)}")
    return JPEG_SUBSAMPLING[subsampling]


def jpeg_restart_mcus() -> int:
    """MCUs in one restart interval of the JPEG encoder (host function)."""
    return int(L.load().dove_jpeg_restart_mcus())


def jpeg_bound(h: int, w: int, subsampling="444") -> int:
    """The most bytes one encoded h x w file can take (host function; 0 for a bad shape)."""
    return int(L.load().dove_jpeg_bound(h, w, jpeg_subsampling_code(subsampling)))


def jpeg_encode(frames: torch.Tensor, quality=95, subsampling="444"):
    """frames: a [N,3,H,W] RGB view (any strides, no copy; uint8, or float32 / bfloat16 in [0,1]) -> (files uint8 [N, jpeg_bound], sizes
    int64 [N]) on the device: row i holds one complete baseline JFIF file in its first sizes[i] bytes (csrc/jpeg.hip).  ``quality``:
    1..100, a number or one per frame; ``subsampling``: '444' or '420'."""
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"jpeg_encode: frames {tuple(frames.shape)} must be a [N,3,H,W] view")
    if not frames.is_cuda:
        raise RuntimeError("jpeg_encode needs its input on the HIP device (`cuda`); there is no CPU path")
    sub = jpeg_subsampling_code(subsampling)
    N, _, H, W = frames.shape
    lib = L.load()
    with torch.cuda.device(frames.device):
        out = torch.empty(N, int(lib.dove_jpeg_bound(H, W, sub)), dtype=torch.uint8, device=frames.device)
        sizes = torch.empty(N, dtype=torch.int64, device=frames.device)
        if N:
            ws = torch.empty(max(int(lib.dove_jpeg_workspace_bytes(N, H, W, sub)), 16), dtype=torch.uint8, device=frames.device)
            v = _image_view(frames)
            L.check(lib.dove_jpeg_encode(C.byref(v), N, H, W, _per_frame(quality, N, C.c_int, "jpeg_encode"), sub, L.ptr(ws), ws.numel(),
                                         L.ptr(out), L.ptr(sizes), L.stream_ptr()), "dove_jpeg_encode")
    return out, sizes


def randn(shape, seed: int, stream_id: int = 0, dtype=torch.float32, offset: int = 0, device="cuda") -> torch.Tensor:
    """Standard normals of the library's counter-based generator (csrc/video.hip ``dove_randn``: Philox4x32-10 keyed by ``seed``, counter
    (element / 4, ``stream_id``), Box-Muller; tests/randn_ref.py is the definition): the elements [offset, offset + numel) of stream
    (seed, stream_id), row-major in ``shape``.  float32, or bfloat16 = the RNE rounding of the float32 value.  The same bits on every call,
    whatever the launch geometry or the split over calls - and the same a C host draws, which torch's generator cannot offer."""
    out = torch.empty(shape, dtype=dtype, device=device)
    L.require_cuda(out)
    L.check(L.load().dove_randn(L.ptr(out), L.dt_code(out), out.numel(), int(seed), int(stream_id), int(offset), L.stream_ptr()), "dove_randn")
    return out


def philox_u32(n: int, seed: int, stream_id: int = 0, offset: int = 0, device="cuda") -> torch.Tensor:
    """The raw Philox4x32-10 words behind ``randn``: the uint32 elements [offset, offset + n) of stream (seed, stream_id), as int64."""
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    L.require_cuda(out)
    L.check(L.load().dove_philox_u32(L.ptr(out), out.numel(), int(seed), int(stream_id), int(offset), L.stream_ptr()), "dove_philox_u32")
    return out.to(torch.int64) & 0xFFFFFFFF


# ---- degradation synthesis (csrc/degrade.hip; tests/degrade_ref.py is the definition) -----------------------------------------------
def _frames_f32(x: torch.Tensor, what: str):
    L.require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"{what}: frames {tuple(x.shape)} {x.dtype} must be float32 [N,H,W,3] (0..255 scale)")
    return x.shape[0], x.shape[1], x.shape[2]


def _per_frame(values, n: int, ctype, what: str):
    vals = [values] * n if isinstance(values, (int, float)) else list(values)
    if len(vals) != n:
        raise ValueError(f"{what}: {len(vals)} per-frame values for {n} frames")
    return (ctype * n)(*vals)


def blur2d(x: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    """cv2.filter2D(x, -1, kernel) with BORDER_REFLECT_101 on float32 [N,H,W,3] frames: ``kernel`` float32 [k,k] for all frames or
    [N,k,k] one per frame, k odd in 3..21."""
    N, H, W = _frames_f32(x, "blur2d")
    L.require_cuda(kernel)
    if kernel.dtype != torch.float32 or kernel.dim() not in (2, 3) or kernel.shape[-1] != kernel.shape[-2] or \
            (kernel.dim() == 3 and kernel.shape[0] != N):
        raise ValueError(f"blur2d: kernel {tuple(kernel.shape)} {kernel.dtype} must be float32 [k,k] or [{N},k,k]")
    out = torch.empty_like(x)
    L.check(L.load().dove_blur2d_f32(L.ptr(x), N, H, W, L.ptr(kernel), kernel.shape[-1], int(kernel.dim() == 3), L.ptr(out), L.stream_ptr()),
            "dove_blur2d_f32")
    return out


def resize(x: torch.Tensor, oh: int, ow: int, mode: int) -> torch.Tensor:
    """float32 [N,H,W,3] -> [N,oh,ow,3]; ``mode`` L.RESIZE_BILINEAR / L.RESIZE_BICUBIC (half-pixel centres, A = -0.75, clamped indices) or
    L.RESIZE_AREA (the pixel-area relation)."""
    N, H, W = _frames_f32(x, "resize")
    out = torch.empty(N, int(oh), int(ow), 3, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_resize_f32(L.ptr(x), N, H, W, int(oh), int(ow), int(mode), L.ptr(out), L.stream_ptr()), "dove_resize_f32")
    return out


def add_gaussian_noise(x: torch.Tensor, sigma, gray: bool, seed: int, stream_id: int = 0, frame0: int = 0) -> torch.Tensor:
    """x + sigma[n] * z on float32 [N,H,W,3] frames, z from the ``randn`` stream (seed, stream_id) at the index of (frame0 + n, y, x, c) -
    gray: of (frame0 + n, y, x), one draw per pixel.  ``sigma``: a number or one per frame."""
    N, H, W = _frames_f32(x, "add_gaussian_noise")
    out = torch.empty_like(x)
    L.check(L.load().dove_add_gaussian_noise_f32(L.ptr(x), N, H, W, _per_frame(sigma, N, C.c_float, "add_gaussian_noise"), int(bool(gray)),
                                                 int(seed), int(stream_id), int(frame0), L.ptr(out), L.stream_ptr()),
            "dove_add_gaussian_noise_f32")
    return out


def add_poisson_noise(x: torch.Tensor, scale, gray: bool, seed: int, stream_id: int = 0, frame0: int = 0) -> torch.Tensor:
    """x + scale[n] * (Poisson(v U) / U - v), v = clip(rint(x), 0, 255) (gray: of the luma) and U = 2^ceil(log2(distinct v of the frame));
    exact sampler on the Philox stream (seed, stream_id).  ``scale``: a number or one per frame."""
    N, H, W = _frames_f32(x, "add_poisson_noise")
    lib = L.load()
    out = torch.empty_like(x)
    ws = torch.empty(int(lib.dove_poisson_noise_workspace_bytes(N)), dtype=torch.uint8, device=x.device)
    L.check(lib.dove_add_poisson_noise_f32(L.ptr(x), N, H, W, _per_frame(scale, N, C.c_float, "add_poisson_noise"), int(bool(gray)), int(seed),
                                           int(stream_id), int(frame0), L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
            "dove_add_poisson_noise_f32")
    return out


def jpeg_roundtrip(x: torch.Tensor, quality) -> torch.Tensor:
    """float32 [N,H,W,3] -> uint8 [N,H,W,3]: baseline JPEG (4:2:0) at ``quality`` (1..100; a number or one per frame) and back, without
    the lossless entropy coding."""
    N, H, W = _frames_f32(x, "jpeg_roundtrip")
    lib = L.load()
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=x.device)
    ws = torch.empty(int(lib.dove_jpeg_roundtrip_workspace_bytes(N, H, W)), dtype=torch.uint8, device=x.device)
    L.check(lib.dove_jpeg_roundtrip(L.ptr(x), N, H, W, _per_frame(quality, N, C.c_int, "jpeg_roundtrip"), L.ptr(ws), ws.numel(), L.ptr(out),
                                    L.stream_ptr()), "dove_jpeg_roundtrip")
    return out


VCODEC_TOOLS = {"intra16": 1, "qpel": 2, "deblock": 4}              # DOVE_VCODEC_* of include/dove_hip.h


def vcodec_tools_mask(tools) -> int:
    """An int mask of VCODEC_TOOLS bits, or an iterable of its names -> the mask.  Host code: unknown bits and names raise ValueError."""
    if isinstance(tools, int) and not isinstance(tools, bool):
        if tools < 0 or tools & ~sum(VCODEC_TOOLS.values()):
            raise ValueError(f"vcodec tools {tools!r}: unknown bits (known: {VCODEC_TOOLS})")
        return tools
    if isinstance(tools, (str, bytes)) or not hasattr(tools, "__iter__"):
        raise ValueError(f"vcodec tools {tools!r}: an int mask or an iterable of names from {sorted(VCODEC_TOOLS)}")
    mask = 0
    for name in tools:
        if name not in VCODEC_TOOLS:
            raise ValueError(f"vcodec tool {name!r}: one of {sorted(VCODEC_TOOLS)}")
        mask |= VCODEC_TOOLS[name]
    return mask


def vcodec_roundtrip(x: torch.Tensor, bitrate: int, gop: int = 8, want_stats: bool = False, tools=0):
    """float32 [N,H,W,3] -> uint8 [N,H,W,3]: the video-compression step (csrc/vcodec.hip; tests/vcodec_ref.py is the definition).  Closed
    groups of ``gop`` frames, I then P with full-search integer motion, H.264 4x4 transform and quantiser on Y'CbCr 4:2:0, one QP per group
    found against ``bitrate`` (bits per frame) * frames.  ``want_stats``: also the QP and the bits of each group, int32 / int64 [ceil(N / gop)].
    ``tools``: the H.264 tool set (tests/vcodec_tools_ref.py is its definition) as a mask or as names of VCODEC_TOOLS - "intra16" (I frames
    predicted from their neighbours), "qpel" (quarter-sample motion), "deblock" (the in-loop edge filter); 0 is the plain codec."""
    tools = vcodec_tools_mask(tools)
    N, H, W = _frames_f32(x, "vcodec_roundtrip")
    if int(gop) != gop or gop <= 0:
        raise ValueError(f"vcodec_roundtrip: gop {gop!r} must be a positive integer")
    if int(bitrate) != bitrate or bitrate < 0:
        raise ValueError(f"vcodec_roundtrip: bitrate {bitrate!r} must be a non-negative integer (bits per frame)")
    lib = L.load()
    groups = -(-N // int(gop))
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=x.device)
    qp = torch.empty(groups, dtype=torch.int32, device=x.device)
    bits = torch.empty(groups, dtype=torch.int64, device=x.device)
    if tools:
        ws = torch.empty(int(lib.dove_vcodec_tools_workspace_bytes(N, H, W, int(gop), tools)), dtype=torch.uint8, device=x.device)
        L.check(lib.dove_vcodec_roundtrip_tools(L.ptr(x), N, H, W, int(bitrate), int(gop), tools, L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(qp),
                                                L.ptr(bits), L.stream_ptr()), "dove_vcodec_roundtrip_tools")
        return (out, qp, bits) if want_stats else out
    ws = torch.empty(int(lib.dove_vcodec_workspace_bytes(N, H, W, int(gop))), dtype=torch.uint8, device=x.device)
    L.check(lib.dove_vcodec_roundtrip(L.ptr(x), N, H, W, int(bitrate), int(gop), L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(qp), L.ptr(bits),
                                      L.stream_ptr()), "dove_vcodec_roundtrip")
    return (out, qp, bits) if want_stats else out


def motion_search_u8(cur: torch.Tensor, ref: torch.Tensor, search: int = 7, lam: int = 4):
    """uint8 [N,H,W] planes -> (mv int32 [N, ceil(H/16), ceil(W/16), 2] as (dy, dx), sad int32 [N, .., ..]): per 16x16 macroblock of
    ``cur`` the displacement in [-search, search]^2 into the edge-replicated ``ref`` that minimises
    (SAD + lam (se_len(dx) + se_len(dy)), |dy| + |dx|, dy, dx), and its SAD."""
    L.require_cuda(cur, ref)
    if cur.dtype != torch.uint8 or ref.dtype != torch.uint8 or cur.dim() != 3 or cur.shape != ref.shape:
        raise ValueError(f"motion_search_u8: cur {tuple(cur.shape)} {cur.dtype} and ref {tuple(ref.shape)} {ref.dtype} must be uint8 [N,H,W] "
                         "of one shape")
    N, H, W = cur.shape
    mv = torch.empty(N, -(-H // 16), -(-W // 16), 2, dtype=torch.int32, device=cur.device)
    sad = torch.empty(N, -(-H // 16), -(-W // 16), dtype=torch.int32, device=cur.device)
    L.check(L.load().dove_motion_search_u8(L.ptr(cur), L.ptr(ref), N, H, W, int(search), int(lam), L.ptr(mv), L.ptr(sad), L.stream_ptr()),
            "dove_motion_search_u8")
    return mv, sad


def stitch(chunk: torch.Tensor, piece: torch.Tensor, region: dict) -> torch.Tensor:
    """``tiling.stitch`` without the write counts (csrc/video.hip ``dove_stitch``): the valid box of ``piece`` [3,f,h,w] goes to its place in
    ``chunk`` [3,F,H,W]; both bfloat16 and contiguous, ``region`` a dict of ``tiling.get_valid_tile_region``."""
    L.require_cuda(chunk, piece)
    if chunk.dtype != torch.bfloat16 or piece.dtype != torch.bfloat16 or chunk.dim() != 4 or piece.dim() != 4 or chunk.shape[0] != 3 or piece.shape[0] != 3:
        raise ValueError(f"stitch: chunk {tuple(chunk.shape)} {chunk.dtype} and piece {tuple(piece.shape)} {piece.dtype} must be bfloat16 [3,F,H,W]")
    valid = (C.c_int * 6)(*(region[f"valid_{a}_{e}"] for a in "thw" for e in ("start", "end")))
    L.check(L.load().dove_stitch(L.ptr(piece), *piece.shape[1:], valid, L.ptr(chunk), *chunk.shape[1:], region["out_t_start"],
                                 region["out_h_start"], region["out_w_start"], L.stream_ptr()), "dove_stitch")
    return chunk


# ---- MXFP8 linears (BASELINE configs[4]; csrc/mxfp8.hip) ------------------------------------------------------------------
@dataclass
class PackedMx:
    """One operand in OCP MXFP8: q [rows][K] e4m3fn bytes, s [K/256][rows][2] words of four E8M0 block scales each."""
    q: torch.Tensor
    s: torch.Tensor
    rows: int
    K: int
    bias: torch.Tensor | None = None


def mx_quant(x: torch.Tensor) -> PackedMx:
    """x [rows, K] bf16 (K % 256 == 0) -> MXFP8 (per 32-element block: scale 2^ceil(log2(amax/448)), RNE to e4m3fn)."""
    L.require_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2
    rows, K = x.shape
    q = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(K // 256, rows, 2, dtype=torch.int32, device=x.device)
    L.check(L.load().dove_mx_quant_bf16(L.ptr(x), rows, K, L.ptr(q), L.ptr(s), L.stream_ptr()), "dove_mx_quant_bf16")
    return PackedMx(q, s, rows, K)


def pack_linear_mx(weight: torch.Tensor, bias: torch.Tensor | None, device) -> PackedMx:
    """nn.Linear weight [N, K] -> MXFP8 operand (quantised on the GPU from its bf16 rounding, like the bf16 path's weights)."""
    w = weight.detach().to(device=device, dtype=torch.bfloat16).contiguous()
    pm = mx_quant(w)
    if bias is not None:
        pm.bias = bias.detach().to(device=device, dtype=torch.float32).contiguous()
    return pm


def linear_mx(x: PackedMx, w: PackedMx, *, resid: torch.Tensor | None = None, gate: torch.Tensor | None = None, gate_split: int = 0,
              act: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """out [M, N] bf16 = epilogue(dequant(x) @ dequant(w)^T + bias); same epilogue contract as ``linear``."""
    M, N, K = x.rows, w.rows, w.K
    assert x.K == K
    L.require_cuda(x.q, x.s, w.q, w.s, resid, gate, out)
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.q.device)
    assert out.dtype == torch.bfloat16 and out.shape[0] == M
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.shape == (2, N)
    L.check(L.load().dove_linear_mxfp8(L.ptr(x.q), L.ptr(x.s), L.ptr(w.q), L.ptr(w.s), L.ptr(w.bias), L.ptr(resid), L.ptr(gate), L.ptr(out),
                                       M, N, K, out.shape[1], resid.shape[1] if resid is not None else 0, gate_split, act,
                                       L.stream_ptr()), "dove_linear_mxfp8")
    return out


# ---- T5 text-encoder operators (csrc/t5.hip) --------------------------------------------------------------------------------
def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    L.require_cuda(x, weight)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and weight.dtype == torch.float32
    y = torch.empty_like(x)
    L.check(L.load().dove_rmsnorm_bf16(L.ptr(x), L.ptr(y), x.shape[0], x.shape[1], eps, L.ptr(weight), L.stream_ptr()), "dove_rmsnorm_bf16")
    return y


def gated_gelu(x: torch.Tensor) -> torch.Tensor:
    """x [M, 2F] (wi_0 x || wi_1 x) -> gelu_new(x[:, :F]) * x[:, F:]."""
    L.require_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 16 == 0
    y = torch.empty(x.shape[0], x.shape[1] // 2, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().dove_gated_gelu_bf16(L.ptr(x), L.ptr(y), x.shape[0], x.shape[1] // 2, L.stream_ptr()), "dove_gated_gelu_bf16")
    return y


def attention_bias(qkv: torch.Tensor, bias: torch.Tensor, heads: int) -> torch.Tensor:
    """T5 self-attention on the fused projection qkv [N, 3*heads*64] with additive fp32 bias [heads, N, N] -> [N, heads*64]."""
    L.require_cuda(qkv, bias)
    N, D = qkv.shape[0], heads * 64
    assert qkv.dtype == torch.bfloat16 and qkv.shape[1] == 3 * D and bias.dtype == torch.float32 and bias.shape == (heads, N, N)
    out = torch.empty(N, D, dtype=torch.bfloat16, device=qkv.device)
    base = qkv.data_ptr()
    L.check(L.load().dove_attention_bias_bf16(C.c_void_p(base), C.c_void_p(base + 2 * D), C.c_void_p(base + 4 * D), 3 * D, L.ptr(bias),
                                              L.ptr(out), D, N, heads, 64, L.stream_ptr()), "dove_attention_bias_bf16")
    return out


# ---- optical flow (csrc/flow.hip, its convs in csrc/conv_f32.hip): fp32 channels-last operators that read and fill channel slices -------
def _cl_f32(t: torch.Tensor, what: str) -> int:
    """Check a float32 [N,H,W,C] tensor or channel-slice view of one (``buf[..., a:b]``) -> its pixel stride in elements."""
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_cuda:
        raise ValueError(f"{what}: need a float32 [N,H,W,C] tensor on the HIP device, got {tuple(t.shape)} {t.dtype} on {t.device}")
    N, H, W, Cc = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if N > 1 else Cc))
    ok = (Cc == 1 or t.stride(3) == 1) and ld >= Cc and (W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) and \
         (N == 1 or t.stride(0) == H * W * ld)
    if not ok:
        raise ValueError(f"{what}: {tuple(t.shape)} with strides {t.stride()} is not a channel slice of a contiguous [N,H,W,ld] buffer")
    return int(ld)


def _conv_f32(fn: str, x: torch.Tensor, w: torch.Tensor, bias, out, out_size, make_args, *, w_sides=None, per_channel=(), residual=None,
              want_name: bool = False):
    """The middle that conv2d_f32, convnet_conv_f32 and resnet_conv_f32 share: check ``w`` (square with a side in ``w_sides`` if given),
    ``bias`` and the ``per_channel`` (name, vector) pairs, size or check ``out`` by ``out_size(H, W, kh, kw)`` -> (ho, wo) (which raises for an
    image that is too small), let ``make_args(ldx, ldo)`` build the entry's struct, set its pointers, and call ``dove_<fn>``."""
    ldx = _cl_f32(x, f"{fn} x")
    L.require_cuda(w, bias, *(v for _, v in per_channel))
    N, H, W, cin = x.shape
    square = w_sides is not None
    if w.dtype != torch.float32 or w.dim() != 4 or w.shape[2] != cin or (square and (w.shape[0] != w.shape[1] or w.shape[0] not in w_sides)):
        rule = f"[k,k,{cin},Cout] with k {' or '.join(map(str, w_sides))}" if square else f"[kh,kw,{cin},Cout]"
        raise ValueError(f"{fn}: w {tuple(w.shape)} {w.dtype} must be float32 {rule}")
    kh, kw, _, cout = w.shape
    for nm, v in (("bias", bias), *per_channel):
        if v is not None and (v.dtype != torch.float32 or v.numel() != cout):
            raise ValueError(f"{fn}: {nm} must be float32 [{cout}]")
    shape = (N, *out_size(H, W, kh, kw), cout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"{fn}: out {tuple(out.shape)} must be {shape}")
    a = make_args(ldx, _cl_f32(out, f"{fn} out"))
    a.x, a.w, a.out = x.data_ptr(), w.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    for nm, v in per_channel:
        setattr(a, nm, v.data_ptr() if v is not None else None)
    if residual is not None:
        if tuple(residual.shape) != shape:
            raise ValueError(f"{fn}: residual {tuple(residual.shape)} must be {shape}")
        a.ldr, a.residual = _cl_f32(residual, f"{fn} residual"), residual.data_ptr()
    lib = L.load()
    L.check(getattr(lib, f"dove_{fn}")(C.byref(a), L.stream_ptr()), f"dove_{fn}")
    return (out, getattr(lib, f"dove_{fn}_kernel_name")(C.byref(a)).decode()) if want_name else out


def conv2d_f32(x: torch.Tensor, w: torch.Tensor, bias=None, *, stride: int = 1, act: int = 0, scale=None, shift=None, out_mul: float = 1.0,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """x [N,H,W,Cin] (a channel slice is fine), w float32 [kh,kw,Cin,Cout] -> out [N,Ho,Wo,Cout] = out_mul * act(scale * (conv + bias) +
    shift), zero padding k // 2.  ``out`` may be a channel slice of a wider buffer: only that slice is written."""
    def args(ldx, ldo):
        a = L.Conv2dF32Args()
        (a.n, a.h, a.w_in, a.cin), (a.kh, a.kw, _, a.cout) = x.shape, w.shape
        a.stride, a.act, a.out_mul, a.ldx, a.ldo = stride, act, out_mul, ldx, ldo
        return a

    return _conv_f32("conv2d_f32", x, w, bias, out,
                     lambda H, W, kh, kw: ((H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1), args,
                     per_channel=(("scale", scale), ("shift", shift)))


def instance_norm_f32(x: torch.Tensor, relu: bool = False, resid: torch.Tensor | None = None, eps: float = 1e-5) -> torch.Tensor:
    """InstanceNorm2d (no affine, biased variance) of contiguous float32 [N,H,W,C]; ``relu``: max(., 0); ``resid``: max(resid + ., 0)."""
    L.require_cuda(x, resid)
    if x.dtype != torch.float32 or x.dim() != 4 or (resid is not None and (resid.shape != x.shape or resid.dtype != x.dtype)):
        raise ValueError(f"instance_norm_f32: x {tuple(x.shape)} {x.dtype} must be float32 [N,H,W,C] and resid of the same shape")
    N, H, W, Cc = x.shape
    lib = L.load()
    ws = torch.empty(max(int(lib.dove_instance_norm_f32_workspace_bytes(N, H, W, Cc)), 8), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    L.check(lib.dove_instance_norm_f32(L.ptr(x), N, H, W, Cc, L.ptr(resid), int(bool(relu)), eps, L.ptr(ws), ws.numel(), L.ptr(out),
                                       L.stream_ptr()), "dove_instance_norm_f32")
    return out


def corr_pyramid_f32(fmap1: torch.Tensor, fmap2: torch.Tensor) -> list:
    """fmaps contiguous float32 [N,H,W,C] -> the all-pairs volume [N*H*W,H,W] scaled by 1/sqrt(C) and its three 2x2 average pools."""
    L.require_cuda(fmap1, fmap2)
    if fmap1.dtype != torch.float32 or fmap1.dim() != 4 or fmap2.shape != fmap1.shape or fmap2.dtype != fmap1.dtype:
        raise ValueError(f"corr_pyramid_f32: fmaps {tuple(fmap1.shape)} / {tuple(fmap2.shape)} must be the same float32 [N,H,W,C]")
    N, H, W, Cc = fmap1.shape
    lib = L.load()
    levels = [torch.empty(N * H * W, H, W, dtype=torch.float32, device=fmap1.device)]
    L.check(lib.dove_corr_volume_f32(L.ptr(fmap1), L.ptr(fmap2), N, H, W, Cc, 1.0 / math.sqrt(Cc), L.ptr(levels[0]), L.stream_ptr()),
            "dove_corr_volume_f32")
    for _ in range(3):
        src = levels[-1]
        dst = torch.empty(src.shape[0], src.shape[1] // 2, src.shape[2] // 2, dtype=torch.float32, device=src.device)
        L.check(lib.dove_avgpool2_f32(L.ptr(src), src.shape[0], src.shape[1], src.shape[2], L.ptr(dst), L.stream_ptr()), "dove_avgpool2_f32")
        levels.append(dst)
    return levels


def corr_lookup_f32(levels, coords: torch.Tensor, add_grid: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """levels: corr_pyramid_f32's four; coords [N,H,W,2] (x, y; a channel slice is fine; ``add_grid``: a flow, the pixel grid is added) ->
    [N,H,W,324]: channel = level * 81 + a * 9 + b samples (x / 2^level + a - 4, y / 2^level + b - 4)."""
    ldc = _cl_f32(coords, "corr_lookup_f32 coords")
    N, H, W, two = coords.shape
    if two != 2 or len(levels) != 4 or any(tuple(l.shape) != (N * H * W, H >> i, W >> i) or not l.is_contiguous() for i, l in enumerate(levels)):
        raise ValueError(f"corr_lookup_f32: coords {tuple(coords.shape)} and levels {[tuple(l.shape) for l in levels]} do not match")
    if out is None:
        out = torch.empty(N, H, W, 324, dtype=torch.float32, device=coords.device)
    L.check(L.load().dove_corr_lookup_f32(*(L.ptr(l) for l in levels), L.ptr(coords), ldc, int(bool(add_grid)), N, H, W, L.ptr(out),
                                          L.stream_ptr()), "dove_corr_lookup_f32")
    return out


def gru_gate_f32(r: torch.Tensor, hx: torch.Tensor, ch_h: int, rhx: torch.Tensor) -> torch.Tensor:
    """rhx[..., :ch_h] = r * hx[..., :ch_h], rhx[..., ch_h:] = hx[..., ch_h:]; hx, rhx contiguous [N,H,W,C], r [N,H,W,ch_h] (slice fine)."""
    ldr = _cl_f32(r, "gru_gate_f32 r")
    L.require_cuda(hx, rhx)
    if hx.shape != rhx.shape or r.shape[:3] != hx.shape[:3] or r.shape[3] != ch_h or hx.dtype != torch.float32 or rhx.dtype != torch.float32:
        raise ValueError("gru_gate_f32: shapes do not match")
    npix = hx.shape[0] * hx.shape[1] * hx.shape[2]
    L.check(L.load().dove_gru_gate_f32(L.ptr(r), ldr, L.ptr(hx), hx.shape[3], ch_h, hx.shape[3], npix, L.ptr(rhx), L.stream_ptr()),
            "dove_gru_gate_f32")
    return rhx


def gru_update_f32(z: torch.Tensor, q: torch.Tensor, hx: torch.Tensor) -> torch.Tensor:
    """hx[..., :ch_h] = (1 - z) * hx[..., :ch_h] + z * q in place; z, q [N,H,W,ch_h] (slices fine), hx contiguous [N,H,W,C]."""
    ldz, ldq = _cl_f32(z, "gru_update_f32 z"), _cl_f32(q, "gru_update_f32 q")
    L.require_cuda(hx)
    if z.shape != q.shape or z.shape[:3] != hx.shape[:3] or z.shape[3] > hx.shape[3] or hx.dtype != torch.float32:
        raise ValueError("gru_update_f32: shapes do not match")
    npix = hx.shape[0] * hx.shape[1] * hx.shape[2]
    L.check(L.load().dove_gru_update_f32(L.ptr(z), ldz, L.ptr(q), ldq, L.ptr(hx), hx.shape[3], z.shape[3], npix, L.stream_ptr()),
            "dove_gru_update_f32")
    return hx


def add_f32(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """out = a + b (``relu``: max(., 0)) on float32 [N,H,W,C] tensors or channel slices; ``out`` may be ``a`` or ``b``."""
    lda, ldb = _cl_f32(a, "add_f32 a"), _cl_f32(b, "add_f32 b")
    if out is None:
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    if a.shape != b.shape or out.shape != a.shape:
        raise ValueError("add_f32: shapes do not match")
    npix = a.shape[0] * a.shape[1] * a.shape[2]
    L.check(L.load().dove_add_f32(L.ptr(a), lda, L.ptr(b), ldb, L.ptr(out), _cl_f32(out, "add_f32 out"), a.shape[3], npix, int(bool(relu)),
                                  L.stream_ptr()), "dove_add_f32")
    return out


def convex_upsample_f32(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """flow [N,H,W,2] (a channel slice is fine), mask contiguous [N,H,W,576] -> [N,2,8H,8W]: RAFT's convex combination of the 3x3
    neighbours of 8 * flow under softmax(mask) over the 9 taps."""
    ldf = _cl_f32(flow, "convex_upsample_f32 flow")
    L.require_cuda(mask)
    N, H, W, two = flow.shape
    if two != 2 or tuple(mask.shape) != (N, H, W, 576) or mask.dtype != torch.float32:
        raise ValueError(f"convex_upsample_f32: flow {tuple(flow.shape)} and mask {tuple(mask.shape)} must be [N,H,W,2] and [N,H,W,576]")
    out = torch.empty(N, 2, 8 * H, 8 * W, dtype=torch.float32, device=flow.device)
    L.check(L.load().dove_convex_upsample_f32(L.ptr(flow), ldf, L.ptr(mask), N, H, W, L.ptr(out), L.stream_ptr()), "dove_convex_upsample_f32")
    return out


def flow_warp_error(img1: torch.Tensor, img2: torch.Tensor, flow_fw: torch.Tensor, flow_bw: torch.Tensor, want_warped: bool = False,
                    want_mask: bool = False):
    """img1, img2 [N,H,W,3] uint8 (read as value / 255) or float32 in [0, 1]; flow_fw, flow_bw float32 [N,2,H,W] ->
    (sums fp64 [N,2] = {masked squared error, mask count}, warped [N,H,W,3] or None, mask uint8 [N,H,W] or None: bit 0 the
    forward-backward check, bit 1 "the sample position lies inside the frame")."""
    L.require_cuda(img1, img2, flow_fw, flow_bw)
    if img1.dim() != 4 or img1.shape[3] != 3 or img2.shape != img1.shape or img2.dtype != img1.dtype or \
            img1.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"flow_warp_error: images {tuple(img1.shape)} {img1.dtype} / {tuple(img2.shape)} {img2.dtype} must be the same "
                         "uint8 or float32 [N,H,W,3]")
    N, H, W, _ = img1.shape
    for f in (flow_fw, flow_bw):
        if f.dtype != torch.float32 or tuple(f.shape) != (N, 2, H, W):
            raise ValueError(f"flow_warp_error: flow {tuple(f.shape)} {f.dtype} must be float32 {(N, 2, H, W)}")
    lib = L.load()
    dev = img1.device
    ws = torch.empty(max(int(lib.dove_flow_warp_error_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=dev)
    sums = torch.empty(N, 2, dtype=torch.float64, device=dev)
    warped = torch.empty(N, H, W, 3, dtype=torch.float32, device=dev) if want_warped else None
    mask = torch.empty(N, H, W, dtype=torch.uint8, device=dev) if want_mask else None
    L.check(lib.dove_flow_warp_error(L.ptr(img1), L.ptr(img2), L.U8 if img1.dtype == torch.uint8 else L.F32, L.ptr(flow_fw), L.ptr(flow_bw),
                                     N, H, W, L.ptr(ws), ws.numel(), L.ptr(sums), L.ptr(warped), L.ptr(mask), L.stream_ptr()),
            "dove_flow_warp_error")
    return sums, warped, mask


# ---- perceptual metrics (csrc/percep.hip, the trunk conv in csrc/conv_f32.hip): the fp32 trunk operators and the fp64 heads --------------
def _convnet_args(x_shape, ldx: int, w_shape, stride: int, pad, relu: bool, ldo: int | None = None) -> "L.ConvnetConvF32Args":
    N, H, W, cin = x_shape
    kh, kw, _, cout = w_shape
    a = L.ConvnetConvF32Args()
    a.n, a.h, a.w_in, a.cin, a.cout, a.kh, a.kw, a.stride, a.pad_h, a.pad_w, a.relu = N, H, W, cin, cout, kh, kw, stride, pad[0], pad[1], int(relu)
    a.ldx, a.ldo = ldx, cout if ldo is None else ldo
    return a


def convnet_conv_kernel_name(x_shape, w_shape, stride: int = 1, pad=(1, 1), ldx: int | None = None) -> str:
    """The kernel ``convnet_conv_f32`` runs for dense, aligned tensors of these shapes ('' for a shape it refuses); needs no device."""
    a = _convnet_args(x_shape, x_shape[3] if ldx is None else ldx, w_shape, stride, pad, True)
    a.x = a.w = a.out = 256                                            # placeholders: only their alignment is looked at
    return L.load().dove_convnet_conv_f32_kernel_name(C.byref(a)).decode()


def convnet_conv_f32(x: torch.Tensor, w: torch.Tensor, bias=None, *, stride: int = 1, pad=(1, 1), relu: bool = True,
                     out: torch.Tensor | None = None, want_name: bool = False):
    """x [N,H,W,Cin] (a channel slice is fine), w float32 [kh,kw,Cin,Cout] -> out [N,Ho,Wo,Cout] = conv + bias, ReLU'd if ``relu``;
    kernels up to 11 x 11, stride 1..4, zero padding ``pad`` below the kernel.  ``out`` may be a channel slice of a wider buffer.
    ``want_name``: also return the kernel that ran."""
    def out_size(H, W, kh, kw):
        ho, wo = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
        if ho < 1 or wo < 1:
            raise ValueError(f"convnet_conv_f32: image {H} x {W} is smaller than the kernel {kh} x {kw} with padding {tuple(pad)}")
        return ho, wo

    return _conv_f32("convnet_conv_f32", x, w, bias, out, out_size,
                     lambda ldx, ldo: _convnet_args(x.shape, ldx, w.shape, stride, pad, relu, ldo), want_name=want_name)


def percep_prep_f32(img: torch.Tensor, pre_mul: float, pre_add: float, mean, std, out: torch.Tensor | None = None) -> torch.Tensor:
    """img: an [N,C,H,W] view (any strides, no copy), C in {1, 3}, uint8 (read as u / 255) or float32 -> dense float32 [N,H,W,3] =
    ((pre_mul * v + pre_add) - mean[ch]) / std[ch]; one channel feeds all three."""
    if img.dim() != 4 or img.shape[1] not in (1, 3) or img.dtype not in (torch.uint8, torch.float32) or not img.is_cuda:
        raise ValueError(f"percep_prep_f32: need a uint8 / float32 [N,1|3,H,W] view on the HIP device, got {tuple(img.shape)} {img.dtype} "
                         f"on {img.device}")
    N, Cc, H, W = img.shape
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.float32, device=img.device)
    elif tuple(out.shape) != (N, H, W, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"percep_prep_f32: out must be contiguous float32 {(N, H, W, 3)}")
    v = _image_view(img)
    m3, s3 = (C.c_float * 3)(*[float(t) for t in mean]), (C.c_float * 3)(*[float(t) for t in std])
    L.check(L.load().dove_percep_prep_f32(C.byref(v), N, Cc, H, W, float(pre_mul), float(pre_add), m3, s3, L.ptr(out), L.stream_ptr()),
            "dove_percep_prep_f32")
    return out


def maxpool_f32(x: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """k x k max pool of stride ``stride`` without padding (floor sizes) of float32 [N,H,W,C] (a channel slice is fine)."""
    ldx = _cl_f32(x, "maxpool_f32 x")
    N, H, W, Cc = x.shape
    if H < k or W < k:
        raise ValueError(f"maxpool_f32: image {H} x {W} is smaller than the window {k}")
    out = torch.empty(N, (H - k) // stride + 1, (W - k) // stride + 1, Cc, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_maxpool_f32(L.ptr(x), ldx, N, H, W, Cc, k, stride, L.ptr(out), Cc, L.stream_ptr()), "dove_maxpool_f32")
    return out


def l2pool_f32(x: torch.Tensor) -> torch.Tensor:
    """DISTS' L2 pooling of float32 [N,H,W,C]: sqrt(sum_taps g x^2 + 1e-12), g = outer((1/4, 1/2, 1/4)), stride 2, zero padding 1."""
    ldx = _cl_f32(x, "l2pool_f32 x")
    N, H, W, Cc = x.shape
    out = torch.empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_l2pool_f32(L.ptr(x), ldx, N, H, W, Cc, L.ptr(out), Cc, L.stream_ptr()), "dove_l2pool_f32")
    return out


def _head_pair(x: torch.Tensor, y: torch.Tensor, what: str) -> int:
    ld = _cl_f32(x, f"{what} x")
    if y.shape != x.shape or _cl_f32(y, f"{what} y") != ld:
        raise ValueError(f"{what}: x {tuple(x.shape)} and y {tuple(y.shape)} must have one shape and one pixel stride")
    return ld


def lpips_layer(x: torch.Tensor, y: torch.Tensor, lin: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x, y float32 [N,H,W,C] feature maps, lin float32 [C]: out[n] (float64 [N]) += mean over pixels of
    sum_c lin[c] (x / (|x| + 1e-10) - y / (|y| + 1e-10))^2, evaluated in fp64."""
    ld = _head_pair(x, y, "lpips_layer")
    N, H, W, Cc = x.shape
    L.require_cuda(lin, out)
    if lin.dtype != torch.float32 or lin.numel() != Cc or out.dtype != torch.float64 or tuple(out.shape) != (N,):
        raise ValueError(f"lpips_layer: lin must be float32 [{Cc}] and out float64 [{N}]")
    lib = L.load()
    ws = torch.empty(max(int(lib.dove_lpips_layer_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=x.device)
    L.check(lib.dove_lpips_layer(L.ptr(x), L.ptr(y), ld, L.ptr(lin), N, H, W, Cc, L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
            "dove_lpips_layer")
    return out


def dists_layer(x: torch.Tensor, y: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x, y float32 [N,H,W,C], alpha, beta float64 [C] (already normalised): out[n] (float64 [N]) += sum_c alpha[c] S1 + beta[c] S2 with
    S1 = (2 mx my + 1e-6) / (mx^2 + my^2 + 1e-6), S2 = (2 cov + 1e-6) / (vx + vy + 1e-6) from fp64 statistics per channel."""
    ld = _head_pair(x, y, "dists_layer")
    N, H, W, Cc = x.shape
    L.require_cuda(alpha, beta, out)
    if any(t.dtype != torch.float64 or t.numel() != Cc for t in (alpha, beta)) or out.dtype != torch.float64 or tuple(out.shape) != (N,):
        raise ValueError(f"dists_layer: alpha, beta must be float64 [{Cc}] and out float64 [{N}]")
    lib = L.load()
    ws = torch.empty(max(int(lib.dove_dists_layer_workspace_bytes(N, H, W, Cc)), 8), dtype=torch.uint8, device=x.device)
    L.check(lib.dove_dists_layer(L.ptr(x), L.ptr(y), ld, L.ptr(alpha), L.ptr(beta), N, H, W, Cc, L.ptr(ws), ws.numel(), L.ptr(out),
                                 L.stream_ptr()), "dove_dists_layer")
    return out


# ---- CLIP-IQA (csrc/clipiqa.hip, the tower's conv in csrc/conv_f32.hip): CLIP RN50's fp32 ResNet operators, attention pool and score ---
def _resnet_args(x_shape, ldx: int, w_shape, stride: int, pool: int, relu: bool, ldo: int | None = None) -> "L.ResnetConvF32Args":
    N, H, W, cin = x_shape
    k, _, _, cout = w_shape
    a = L.ResnetConvF32Args()
    a.n, a.h, a.w_in, a.cin, a.cout, a.k, a.stride, a.pool, a.relu = N, H, W, cin, cout, k, stride, pool, int(relu)
    a.ldx, a.ldo = ldx, cout if ldo is None else ldo
    return a


def resnet_conv_kernel_name(x_shape, w_shape, stride: int = 1, pool: int = 1, ldx: int | None = None) -> str:
    """The kernel ``resnet_conv_f32`` runs for dense, aligned tensors of these shapes ('' for a shape it refuses); needs no device."""
    a = _resnet_args(x_shape, x_shape[3] if ldx is None else ldx, w_shape, stride, pool, True)
    a.x = a.w = a.out = 256                                            # placeholders: only their alignment is looked at
    return L.load().dove_resnet_conv_f32_kernel_name(C.byref(a)).decode()


def resnet_conv_f32(x: torch.Tensor, w: torch.Tensor, bias=None, *, stride: int = 1, pool: int = 1, residual: torch.Tensor | None = None,
                    relu: bool = True, out: torch.Tensor | None = None, want_name: bool = False):
    """x [N,H,W,Cin] (a channel slice is fine), w float32 [k,k,Cin,Cout], k in {1, 3} with padding k // 2 -> out [N,Ho,Wo,Cout] =
    relu?((conv + bias) + residual).  ``pool`` 2: the conv reads the 2 x 2 average of x (floor sizes); it and ``residual`` belong to the
    1 x 1 convs that run on pointwise_f32_kernel.  ``residual`` and ``out`` may be channel slices, and may be one tensor.
    ``want_name``: also return the kernel that ran."""
    if pool not in (1, 2) or stride not in (1, 2):
        raise ValueError(f"resnet_conv_f32: pool {pool} and stride {stride} must be 1 or 2")

    def out_size(H, W, k, _):
        ho, wo = (H // pool + 2 * (k // 2) - k) // stride + 1, (W // pool + 2 * (k // 2) - k) // stride + 1
        if ho < 1 or wo < 1:
            raise ValueError(f"resnet_conv_f32: image {H} x {W} is too small for pool {pool}")
        return ho, wo

    return _conv_f32("resnet_conv_f32", x, w, bias, out, out_size,
                     lambda ldx, ldo: _resnet_args(x.shape, ldx, w.shape, stride, pool, relu, ldo), w_sides=(1, 3), residual=residual,
                     want_name=want_name)


def avgpool_cl_f32(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """2 x 2, stride 2 average of float32 [N,H,W,C] (a channel slice is fine), floor sizes: ((a + b) + (c + d)) * 0.25 in fp32."""
    ldx = _cl_f32(x, "avgpool_cl_f32 x")
    N, H, W, Cc = x.shape
    if H < 2 or W < 2:
        raise ValueError(f"avgpool_cl_f32: image {H} x {W} is smaller than the window 2")
    if out is None:
        out = torch.empty(N, H // 2, W // 2, Cc, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (N, H // 2, W // 2, Cc):
        raise ValueError(f"avgpool_cl_f32: out {tuple(out.shape)} must be {(N, H // 2, W // 2, Cc)}")
    L.check(L.load().dove_avgpool_cl_f32(L.ptr(x), ldx, N, H, W, Cc, L.ptr(out), _cl_f32(out, "avgpool_cl_f32 out"), L.stream_ptr()),
            "dove_avgpool_cl_f32")
    return out


def clip_attnpool_f32(x: torch.Tensor, proj) -> torch.Tensor:
    """x float32 [N,H,W,2048] feature map, ``proj`` = (wq, bq, wk, bk, wv, bv, wc, bc) float32 as torch holds them ([out,in] weights) ->
    float32 [N,1024]: CLIP's attention pool without the positional embedding, evaluated in fp64 with the mean token as the only query."""
    ldx = _cl_f32(x, "clip_attnpool_f32 x")
    N, H, W, Cc = x.shape
    proj = tuple(proj)
    L.require_cuda(*proj)
    want = [(2048, 2048), (2048,)] * 3 + [(1024, 2048), (1024,)]
    if Cc != 2048 or len(proj) != 8 or any(t.dtype != torch.float32 or tuple(t.shape) != s for t, s in zip(proj, want)):
        raise ValueError(f"clip_attnpool_f32: x must have 2048 channels (got {Cc}) and proj must be float32 tensors of shapes {want}")
    lib = L.load()
    ws = torch.empty(max(int(lib.dove_clip_attnpool_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=x.device)
    out = torch.empty(N, 1024, dtype=torch.float32, device=x.device)
    L.check(lib.dove_clip_attnpool_f32(L.ptr(x), ldx, N, H, W, *[L.ptr(t) for t in proj], L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
            "dove_clip_attnpool_f32")
    return out


def clipiqa_score(emb: torch.Tensor, text: torch.Tensor, logit_scale: float) -> torch.Tensor:
    """emb float32 [N,D], text float64 [2P,D] (L2-normalised rows, positive then negative of each pair), ``logit_scale`` = exp of CLIP's
    parameter -> float64 [N]: the mean over the pairs of softmax(logit_scale * emb / |emb| . text_pair)[0], in fp64."""
    L.require_cuda(emb, text)
    if emb.dtype != torch.float32 or emb.dim() != 2 or text.dtype != torch.float64 or text.dim() != 2 or text.shape[1] != emb.shape[1] or \
            text.shape[0] < 2 or text.shape[0] % 2:
        raise ValueError(f"clipiqa_score: emb {tuple(emb.shape)} {emb.dtype} must be float32 [N,D] and text {tuple(text.shape)} {text.dtype} "
                         "float64 [2P,D]")
    out = torch.empty(emb.shape[0], dtype=torch.float64, device=emb.device)
    L.check(L.load().dove_clipiqa_score(L.ptr(emb), L.ptr(text), emb.shape[0], text.shape[0] // 2, emb.shape[1], float(logit_scale), L.ptr(out),
                                        L.stream_ptr()), "dove_clipiqa_score")
    return out


# ---- MUSIQ (csrc/musiq.hip): the patch gather, per-patch GroupNorm, LayerNorm, embeddings, fp32 attention, GELU and the fp64 head --------
def linear_f32(x: torch.Tensor, w: torch.Tensor, bias=None, *, residual: torch.Tensor | None = None, relu: bool = False,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """x float32 [M,K] rows (a column slice is fine), w float32 [1,1,K,N] (the Linear's weight transposed) -> [M,N] = relu?((x w + bias) +
    residual) on the 1 x 1 walk of ``resnet_conv_f32`` with the rows as pixels (K % 32 == 0, N % 4 == 0): one fp32 FMA chain in K order
    per output.  ``residual`` and ``out`` may be one tensor."""
    if x.dim() != 2 or (residual is not None and residual.dim() != 2) or (out is not None and out.dim() != 2):
        raise ValueError(f"linear_f32: x {tuple(x.shape)}, residual and out must be [M,K] / [M,N] matrices")
    as4 = lambda t: None if t is None else t.unsqueeze(0).unsqueeze(0)
    return resnet_conv_f32(as4(x), w, bias, residual=as4(residual), relu=relu, out=as4(out))[0, 0]


def _strided_on_device(what: str, *tensors) -> None:
    """``require_cuda`` for operands that may be strided views: on the current HIP device, no word about contiguity."""
    for t in tensors:
        if not t.is_cuda or t.device.index != torch.cuda.current_device():
            raise RuntimeError(f"{what}: tensors must be on the current HIP device (`cuda:{torch.cuda.current_device()}`), got {t.device}")


def musiq_scales(scales) -> "C.Array":
    """Three (rh, rw, pad_top, pad_left, resized) tuples -> the dove_musiq_scale[3] of ``musiq_patches_f32``."""
    arr = (L.MusiqScale * 3)()
    for a, (rh, rw, pt, pl, resized) in zip(arr, scales):
        a.rh, a.rw, a.pad_top, a.pad_left, a.resized = int(rh), int(rw), int(pt), int(pl), int(bool(resized))
    return arr


def musiq_patches_f32(img: torch.Tensor, scales, tokens: torch.Tensor, before: int = 0, side: int = 32) -> torch.Tensor:
    """img: an [N,1|3,H,W] view (uint8 read as u / 255, float32 or bfloat16 in [0,1]; any strides, no copy), ``scales`` three (rh, rw,
    pad_top, pad_left, resized), ``tokens`` int32 [T,4] on the device (scale, patch row, patch column, spatial index) -> float32
    [N T,side,side,3]: every token's 32 x 32 patch of 2 v - 1 at [before, before + 32) of its frame, 0 around it (before 2, side 37: the
    frame of the stem's 7 x 7 stride-2 conv).  Resized scales are bicubic in fp64, rounded once (csrc/musiq.hip)."""
    if img.dim() != 4 or img.shape[1] not in (1, 3) or not img.is_cuda:
        raise ValueError(f"musiq_patches_f32: need an [N,1|3,H,W] view on the HIP device, got {tuple(img.shape)} on {img.device}")
    _strided_on_device("musiq_patches_f32", img)
    L.require_cuda(tokens)
    if tokens.dtype != torch.int32 or tokens.dim() != 2 or tokens.shape[1] != 4 or not tokens.is_contiguous() or len(scales) != 3:
        raise ValueError("musiq_patches_f32: tokens must be contiguous int32 [T,4] and scales three tuples")
    N, Cc, H, W = img.shape
    T = tokens.shape[0]
    out = torch.empty(N * T, side, side, 3, dtype=torch.float32, device=img.device)
    if N * T == 0:
        return out
    v = _image_view(img)
    L.check(L.load().dove_musiq_patches_f32(C.byref(v), N, Cc, H, W, musiq_scales(scales), L.ptr(tokens), T, before, side, L.ptr(out),
                                            L.stream_ptr()), "dove_musiq_patches_f32")
    return out


def musiq_groupnorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, *, relu: bool = False, pool: bool = False,
                        y: torch.Tensor | None = None, gamma_y=None, beta_y=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """GroupNorm(32 groups) of every map of contiguous float32 [P,S,S,C] with fp64 two-pass statistics and one rounding; ``y``: the sum with
    the GroupNorm of a second operand of the same shape; ``relu``; ``pool``: the zero-'same' (0 before, 1 after) 3 x 3 stride-2 max pool of
    the result -> [P,S/2,S/2,C].  ``out`` may be ``x`` without the pool."""
    L.require_cuda(x, gamma, beta, y, gamma_y, beta_y)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != x.shape[2] or not x.is_contiguous():
        raise ValueError(f"musiq_groupnorm_f32: x {tuple(x.shape)} {x.dtype} must be contiguous float32 [P,S,S,C]")
    P, S, _, Cc = x.shape
    vecs = [gamma, beta] + ([gamma_y, beta_y] if y is not None else [])
    if any(t is None or t.dtype != torch.float32 or t.numel() != Cc or not t.is_contiguous() for t in vecs):
        raise ValueError(f"musiq_groupnorm_f32: gamma and beta (of both operands) must be float32 [{Cc}]")
    if y is not None and (y.shape != x.shape or y.dtype != torch.float32 or not y.is_contiguous()):
        raise ValueError(f"musiq_groupnorm_f32: y must be contiguous float32 {tuple(x.shape)}")
    shape = (P, S // 2, S // 2, Cc) if pool else (P, S, S, Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"musiq_groupnorm_f32: out must be contiguous float32 {shape}")
    if P == 0:
        return out
    L.check(L.load().dove_musiq_groupnorm_f32(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(gamma_y if y is not None else None),
                                              L.ptr(beta_y if y is not None else None), P, S, Cc, float(eps), int(bool(relu)), int(bool(pool)),
                                              L.ptr(out), L.stream_ptr()), "dove_musiq_groupnorm_f32")
    return out


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """LayerNorm over the last axis of float32 [R,D] rows (any row stride) with fp64 two-pass statistics and one rounding."""
    _strided_on_device("layernorm_f32", x)
    L.require_cuda(gamma, beta)
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1) or x.stride(0) < x.shape[1]:
        raise ValueError(f"layernorm_f32: x {tuple(x.shape)} {x.dtype} with strides {x.stride()} must be float32 [R,D] rows")
    R, D = x.shape
    if any(t.dtype != torch.float32 or t.numel() != D or not t.is_contiguous() for t in (gamma, beta)):
        raise ValueError(f"layernorm_f32: gamma and beta must be float32 [{D}]")
    if out is None:
        out = torch.empty(R, D, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (R, D) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"layernorm_f32: out must be contiguous float32 {(R, D)}")
    if R == 0:
        return out
    L.check(L.load().dove_layernorm_f32(L.ptr(x), x.stride(0), R, D, L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(out), D, L.stream_ptr()),
            "dove_layernorm_f32")
    return out


def musiq_embed_f32(emb: torch.Tensor, pos: torch.Tensor, scale_emb: torch.Tensor, cls: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """emb float32 [N T,D] patch embeddings, pos [100,D], scale_emb [3,D], cls [D], tokens int32 [T,4] -> float32 [N,T + 1,D]: the cls token,
    then (emb + pos[spatial index]) + scale_emb[scale] per token."""
    L.require_cuda(emb, pos, scale_emb, cls, tokens)
    T, D = tokens.shape[0], emb.shape[1]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (emb, pos, scale_emb, cls)) or emb.dim() != 2 or T == 0 or \
            emb.shape[0] % T or pos.shape[-1] != D or scale_emb.shape[-1] != D or cls.numel() != D or tokens.dtype != torch.int32:
        raise ValueError(f"musiq_embed_f32: emb {tuple(emb.shape)} must be contiguous float32 [N T,D] with T = {T} and the tables D wide")
    N = emb.shape[0] // T
    out = torch.empty(N, T + 1, D, dtype=torch.float32, device=emb.device)
    if N == 0:
        return out
    L.check(L.load().dove_musiq_embed_f32(L.ptr(emb), L.ptr(pos), L.ptr(scale_emb), L.ptr(cls), L.ptr(tokens), N, T, D, L.ptr(out), L.stream_ptr()),
            "dove_musiq_embed_f32")
    return out


def mha_f32_tiles() -> tuple:
    """(Q tile, KV tile) of ``mha_f32``'s kernel; needs no device."""
    q, kv = C.c_int(0), C.c_int(0)
    L.load().dove_mha_f32_tiles(C.byref(q), C.byref(kv))
    return q.value, kv.value


def mha_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float | None = None) -> torch.Tensor:
    """q, k, v float32 [N,T,heads * 64] (column slices of one QKV buffer are fine) -> softmax(scale q k^T) v per frame and head, float32
    [N,T,heads * 64]; flash-style fp32 MFMA attention (csrc/musiq.hip).  ``scale`` defaults to 1 / 8."""
    _strided_on_device("mha_f32", q, k, v)
    N, T, D = q.shape
    ok = lambda t: t.dtype == torch.float32 and tuple(t.shape) == (N, T, D) and t.stride(2) == 1 and t.stride(1) == q.stride(1) and \
        (N == 1 or t.stride(0) == T * t.stride(1))
    if D % 64 or not (ok(q) and ok(k) and ok(v)):
        raise ValueError(f"mha_f32: q, k, v must be float32 [N,T,64 heads] rows of one stride, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    out = torch.empty(N, T, D, dtype=torch.float32, device=q.device)
    if N * T == 0:
        return out
    L.check(L.load().dove_mha_f32(L.ptr(q), L.ptr(k), L.ptr(v), q.stride(1), N, T, D // 64, 0.125 if scale is None else float(scale), L.ptr(out), D,
                                  L.stream_ptr()), "dove_mha_f32")
    return out


def gelu_f32(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Exact-erf GELU of a contiguous float32 tensor in fp32: 0.5 x (1 + erff(x / sqrt 2)).  ``out`` may be ``x``."""
    L.require_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"gelu_f32: x {tuple(x.shape)} {x.dtype} must be contiguous float32")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("gelu_f32: out must be contiguous float32 of x's shape")
    if x.numel():
        L.check(L.load().dove_gelu_f32(L.ptr(x), x.numel(), L.ptr(out), L.stream_ptr()), "dove_gelu_f32")
    return out


def musiq_score(features: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """features float32 [N,D] (any row stride), head weight float32 [K,D] and bias [K] -> float64 [N]: the head in fp64; K = 1 gives the
    row, K > 1 the mean of softmax(row) over the ratings 1 .. K."""
    _strided_on_device("musiq_score", features)
    L.require_cuda(w, b)
    N, D = features.shape
    if features.dtype != torch.float32 or (D > 1 and features.stride(1) != 1) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != D or \
            not w.is_contiguous() or b.dtype != torch.float32 or b.numel() != w.shape[0]:
        raise ValueError(f"musiq_score: features {tuple(features.shape)} must be float32 [N,D] rows, w float32 [K,D], b float32 [K]")
    out = torch.empty(N, dtype=torch.float64, device=features.device)
    if N:
        L.check(L.load().dove_musiq_score(L.ptr(features), features.stride(0), L.ptr(w), L.ptr(b), N, D, w.shape[0], L.ptr(out), L.stream_ptr()),
                "dove_musiq_score")
    return out


# ---- FasterVQA / FAST-VQA (csrc/swin3d.hip): the fragment gather, 3-D windows, patch merging, window attention and the fp64 head ----------
def _int3(values, what: str) -> "C.Array":
    if len(values) != 3:
        raise ValueError(f"{what} must have three entries, got {tuple(values)}")
    return (C.c_int * 3)(*(int(v) for v in values))


def vqa_fragments_f32(clip: torch.Tensor, frames: torch.Tensor, offsets: torch.Tensor, fragment, mean, std, cols: bool = False) -> torch.Tensor:
    """clip: an [F,3,H,W] view (uint8, or float32 / bfloat16 in [0,1]; any strides, no copy), ``frames`` int32 [T] and ``offsets`` int32
    [gh,gw,t_groups,2] (row, column of each fragment's top-left source pixel) on the device, ``fragment`` = (fh, fw) -> float32
    [T,gh fh,gw fw,3]: (X - mean) / std in fp64, rounded once, X the uint8 value or 255 v.  ``cols``: the same values as the patch
    embedding's GEMM rows, float32 [T/2,gh fh/4,gw fw/4,96] (csrc/swin3d.hip)."""
    if clip.dim() != 4 or clip.shape[1] != 3 or not clip.is_cuda:
        raise ValueError(f"vqa_fragments_f32: need an [F,3,H,W] view on the HIP device, got {tuple(clip.shape)} on {clip.device}")
    _strided_on_device("vqa_fragments_f32", clip)
    L.require_cuda(frames, offsets)
    if frames.dtype != torch.int32 or frames.dim() != 1 or offsets.dtype != torch.int32 or offsets.dim() != 4 or offsets.shape[3] != 2:
        raise ValueError("vqa_fragments_f32: frames must be int32 [T] and offsets int32 [gh,gw,t_groups,2]")
    T, (gh, gw, tg, _), (fh, fw) = frames.shape[0], offsets.shape, fragment
    if T == 0 or tg == 0 or T % tg:
        raise ValueError(f"vqa_fragments_f32: {T} frames do not split into {tg} temporal groups")
    Hc, Wc = gh * fh, gw * fw
    if cols and (T % 2 or Hc % 4 or Wc % 4):
        raise ValueError(f"vqa_fragments_f32: the patch rows need an even T and canvas sides that are multiples of 4, got {T} x {Hc} x {Wc}")
    out = torch.empty((T // 2, Hc // 4, Wc // 4, 96) if cols else (T, Hc, Wc, 3), dtype=torch.float32, device=clip.device)
    v = _image_view(clip)
    L.check(L.load().dove_vqa_fragments_f32(C.byref(v), clip.shape[0], clip.shape[2], clip.shape[3], L.ptr(frames), T, L.ptr(offsets), gh, gw,
                                            fh, fw, tg, (C.c_double * 3)(*map(float, mean)), (C.c_double * 3)(*map(float, std)), int(bool(cols)),
                                            L.ptr(out), L.stream_ptr()), "dove_vqa_fragments_f32")
    return out


def _token_map(x: torch.Tensor, what: str):
    L.require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 5 or x.shape[4] % 4 or x.numel() == 0:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} must be contiguous float32 [B,D,H,W,C] with C a multiple of 4")
    return x.shape


def swin3d_padded(dims, window):
    """(padded dims, window count, window length) of a D x H x W map cut into ``window``-sized windows."""
    padded = tuple(-(-d // w) * w for d, w in zip(dims, window))
    return padded, (padded[0] // window[0]) * (padded[1] // window[1]) * (padded[2] // window[2]), window[0] * window[1] * window[2]


def swin3d_window_gather_f32(x: torch.Tensor, window, shift=(0, 0, 0)) -> torch.Tensor:
    """Token map float32 [B,D,H,W,C] -> windows float32 [B nW,N,C]: zero pad to multiples of ``window``, roll by -``shift``, partition
    (one pass; padded slots read 0).  ``window`` and ``shift`` are the clamped ones (0 <= shift < window)."""
    B, D, H, W, Cc = _token_map(x, "swin3d_window_gather_f32")
    _, nW, N = swin3d_padded((D, H, W), window)
    out = torch.empty(B * nW, N, Cc, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_swin3d_window_gather_f32(L.ptr(x), B, _int3((D, H, W), "dims"), Cc, _int3(window, "window"), _int3(shift, "shift"),
                                                   L.ptr(out), L.stream_ptr()), "dove_swin3d_window_gather_f32")
    return out


def swin3d_window_scatter_f32(windows: torch.Tensor, shortcut: torch.Tensor, window, shift=(0, 0, 0), out: torch.Tensor | None = None):
    """The inverse of ``swin3d_window_gather_f32`` plus the shortcut: windows float32 [B nW,N,C] and shortcut [B,D,H,W,C] -> shortcut +
    (windows merged, rolled back, cropped).  ``out`` may be ``shortcut``."""
    B, D, H, W, Cc = _token_map(shortcut, "swin3d_window_scatter_f32")
    L.require_cuda(windows)
    _, nW, N = swin3d_padded((D, H, W), window)
    if windows.dtype != torch.float32 or tuple(windows.shape) != (B * nW, N, Cc):
        raise ValueError(f"swin3d_window_scatter_f32: windows {tuple(windows.shape)} {windows.dtype} must be float32 {(B * nW, N, Cc)}")
    if out is None:
        out = torch.empty_like(shortcut)
    elif out.shape != shortcut.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("swin3d_window_scatter_f32: out must be contiguous float32 of the shortcut's shape")
    L.check(L.load().dove_swin3d_window_scatter_f32(L.ptr(windows), L.ptr(shortcut), B, _int3((D, H, W), "dims"), Cc, _int3(window, "window"),
                                                    _int3(shift, "shift"), L.ptr(out), L.stream_ptr()), "dove_swin3d_window_scatter_f32")
    return out


def swin3d_patch_merge_f32(x: torch.Tensor) -> torch.Tensor:
    """Token map float32 [B,D,H,W,C] -> [B,D,ceil(H/2),ceil(W/2),4 C]: the 2 x 2 neighbours (0,0), (1,0), (0,1), (1,1) side by side, odd
    H or W zero-padded."""
    B, D, H, W, Cc = _token_map(x, "swin3d_patch_merge_f32")
    out = torch.empty(B, D, (H + 1) // 2, (W + 1) // 2, 4 * Cc, dtype=torch.float32, device=x.device)
    L.check(L.load().dove_swin3d_patch_merge_f32(L.ptr(x), B * D, H, W, Cc, L.ptr(out), L.stream_ptr()), "dove_swin3d_patch_merge_f32")
    return out


def swin3d_attention_tiles() -> tuple:
    """(query tile, key tile, longest window) of ``swin3d_window_attention_f32``'s kernel; needs no device."""
    q, kv, mx = C.c_int(0), C.c_int(0), C.c_int(0)
    L.load().dove_swin3d_attention_tiles(C.byref(q), C.byref(kv), C.byref(mx))
    return q.value, kv.value, mx.value


def swin3d_window_attention_f32(qkv: torch.Tensor, heads: int, table: torch.Tensor, index: torch.Tensor, *, scale: float | None = None,
                                table_b: torch.Tensor | None = None, frag: torch.Tensor | None = None,
                                region: torch.Tensor | None = None) -> torch.Tensor:
    """qkv float32 [W,N,3 heads 32] (q, k, v side by side), ``table`` float32 [R,heads], ``index`` int32 [N,N] -> float32 [W,N,heads 32]:
    softmax(scale q k^T + table[index] + mask) v per window and head on the fp32 MFMA (csrc/swin3d.hip).  ``region`` int32 [w,N] (w divides
    W: the windows of one sample): -100 between tokens of different ids.  ``table_b`` with ``frag`` int32 [w,N]: the bias of token pairs
    whose ids differ comes from ``table_b``.  ``scale`` defaults to 1 / sqrt(32)."""
    L.require_cuda(qkv, table, index, table_b, frag, region)
    if qkv.dtype != torch.float32 or qkv.dim() != 3 or qkv.shape[2] != 3 * heads * 32 or qkv.numel() == 0:
        raise ValueError(f"swin3d_window_attention_f32: qkv {tuple(qkv.shape)} {qkv.dtype} must be float32 [W,N,{3 * heads * 32}] for {heads} heads of 32")
    Wn, N, _ = qkv.shape
    if N > swin3d_attention_tiles()[2]:
        raise ValueError(f"swin3d_window_attention_f32: a window of {N} tokens is longer than the kernel's {swin3d_attention_tiles()[2]}")
    tabs = [table] + ([table_b] if table_b is not None else [])
    if any(t.dtype != torch.float32 or t.dim() != 2 or t.shape != table.shape or t.shape[1] != heads for t in tabs):
        raise ValueError(f"swin3d_window_attention_f32: the bias tables must be float32 [R,{heads}] of one shape")
    if index.dtype != torch.int32 or tuple(index.shape) != (N, N):
        raise ValueError(f"swin3d_window_attention_f32: index must be int32 {(N, N)}, got {index.dtype} {tuple(index.shape)}")
    if table_b is not None and frag is None:
        raise ValueError("swin3d_window_attention_f32: a second table needs the fragment ids")
    idw = 1
    for name, t in (("frag", frag), ("region", region)):
        if t is None:
            continue
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != N or t.shape[0] == 0 or Wn % t.shape[0]:
            raise ValueError(f"swin3d_window_attention_f32: {name} must be int32 [w,{N}] with w dividing {Wn}, got {t.dtype} {tuple(t.shape)}")
        idw = t.shape[0]
    if frag is not None and region is not None and frag.shape != region.shape:
        raise ValueError("swin3d_window_attention_f32: frag and region must have one shape")
    D = heads * 32
    out = torch.empty(Wn, N, D, dtype=torch.float32, device=qkv.device)
    L.check(L.load().dove_swin3d_window_attention_f32(
        L.ptr(qkv), C.c_void_p(qkv.data_ptr() + 4 * D), C.c_void_p(qkv.data_ptr() + 8 * D), 3 * D, Wn, N, heads,
        1.0 / math.sqrt(32.0) if scale is None else float(scale), L.ptr(table), L.ptr(table_b), table.shape[0], L.ptr(index), L.ptr(frag),
        L.ptr(region), idw, L.ptr(out), D, L.stream_ptr()), "dove_swin3d_window_attention_f32")
    return out


def vqa_head_f64(features: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """features float32 [clips,tokens,D], fc_hid weight [hid,D] and bias [hid], fc_last weight [hid] and bias [1] -> float64 [clips]: the
    mean over tokens of fc_last(gelu(fc_hid(f))) in fp64 with fixed-order sums."""
    L.require_cuda(features, w1, b1, w2, b2)
    if features.dtype != torch.float32 or features.dim() != 3 or features.numel() == 0:
        raise ValueError(f"vqa_head_f64: features {tuple(features.shape)} {features.dtype} must be float32 [clips,tokens,D]")
    n, T, D = features.shape
    hid = w1.shape[0]
    if any(t.dtype != torch.float32 for t in (w1, b1, w2, b2)) or tuple(w1.shape) != (hid, D) or b1.numel() != hid or w2.numel() != hid or \
            b2.numel() != 1 or hid > 256:
        raise ValueError(f"vqa_head_f64: need float32 w1 [hid,{D}], b1 [hid], w2 [hid], b2 [1] with hid <= 256")
    out = torch.empty(n, dtype=torch.float64, device=features.device)
    L.check(L.load().dove_vqa_head_f64(L.ptr(features), D, n, T, D, L.ptr(w1), L.ptr(b1), hid, L.ptr(w2), L.ptr(b2), L.ptr(out), L.stream_ptr()),
            "dove_vqa_head_f64")
    return out


# ---- DOVER's aesthetic branch (csrc/convnext3d.hip): the depthwise 3 x 7 x 7 conv and the resized view ------------------------------------
def dwconv3d_tile(h: int, w: int) -> tuple:
    """(rows, columns) of the output tile one workgroup of ``dwconv3d_f32`` owns on an h x w map; needs no device."""
    th, tw = C.c_int(0), C.c_int(0)
    L.load().dove_dwconv3d_tile(int(h), int(w), C.byref(th), C.byref(tw))
    return th.value, tw.value


def dwconv3d_f32(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Depthwise Conv3d, kernel (3,7,7), zero padding (1,3,3), stride 1, on a channels-last map float32 [B,D,H,W,C]; ``w`` float32
    [3,7,7,C] (tap-major), ``bias`` [C].  Exact fp32: one fmaf chain per output from the bias over the taps in (kd, kh, kw) order.
    ``out`` must not alias ``x``."""
    B, D, H, W, Cc = _token_map(x, "dwconv3d_f32")
    L.require_cuda(w, bias)
    if not x.is_contiguous():
        raise ValueError("dwconv3d_f32: x must be contiguous")
    if w.dtype != torch.float32 or tuple(w.shape) != (3, 7, 7, Cc) or not w.is_contiguous() or bias.dtype != torch.float32 or \
            tuple(bias.shape) != (Cc,) or not bias.is_contiguous():
        raise ValueError(f"dwconv3d_f32: need contiguous float32 w [3,7,7,{Cc}] and bias [{Cc}], got {tuple(w.shape)} and {tuple(bias.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("dwconv3d_f32: out must be contiguous float32 of x's shape")
    elif out.data_ptr() < x.data_ptr() + 4 * x.numel() and x.data_ptr() < out.data_ptr() + 4 * out.numel():
        raise ValueError("dwconv3d_f32: out must not alias x (every output reads 147 inputs around it)")
    L.check(L.load().dove_dwconv3d_f32(L.ptr(x), B, D, H, W, Cc, L.ptr(w), L.ptr(bias), L.ptr(out), L.stream_ptr()), "dove_dwconv3d_f32")
    return out


_RESIZE_TAPS = {}


def resize_taps(n_in: int, n_out: int, antialias: bool = True) -> dict:
    """The tap table of one axis of torch's bilinear ``F.interpolate(align_corners=False)`` from ``n_in`` to ``n_out`` samples, in fp64:
    ``first`` int32 [n_out], ``count`` int32 [n_out], ``weights`` float64 [n_out,max] (zero past the count).  ``antialias``: the triangle
    filter of support max(in / out, 1); else two taps at max(0, scale (i + 0.5) - 0.5), the upper index clamped.  Taps of weight 0 at
    either end are dropped (n_in == n_out is the identity table).  Cached per (n_in, n_out, mode); ``device``: the uploads, per device."""
    key = (int(n_in), int(n_out), bool(antialias))
    if key in _RESIZE_TAPS:
        return _RESIZE_TAPS[key]
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_taps: {n_in} -> {n_out} samples")
    scale = n_in / n_out
    rows = []
    for i in range(n_out):
        if antialias:
            support, c = max(scale, 1.0), scale * (i + 0.5)
            lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
            wts = [max(0.0, 1.0 - abs((j - c + 0.5) / support)) for j in range(lo, hi)]
            total = sum(wts)
            wts = [v / total for v in wts]
        else:
            src = max(0.0, scale * (i + 0.5) - 0.5)
            lo = min(int(src), n_in - 1)
            lam = src - lo
            wts = [1.0 - lam, lam] if lo + 1 < n_in else [1.0]       # the clamped upper index is the lower one: (1 - l) v + l v
        while len(wts) > 1 and wts[-1] == 0.0:
            wts.pop()
        while len(wts) > 1 and wts[0] == 0.0:
            wts.pop(0)
            lo += 1
        rows.append((lo, wts))
    most = max(len(wts) for _, wts in rows)
    tab = np.zeros((n_out, 2), dtype=np.int32)
    weights = np.zeros((n_out, most), dtype=np.float64)
    for i, (lo, wts) in enumerate(rows):
        tab[i] = (lo, len(wts))
        weights[i, :len(wts)] = wts
    assert tab[:, 0].min() >= 0 and (tab[:, 0] + tab[:, 1]).max() <= n_in
    taps = {"first": tab[:, 0].copy(), "count": tab[:, 1].copy(), "table": tab, "weights": weights, "max": most, "device": {}}
    _RESIZE_TAPS[key] = taps
    return taps


def _taps_on(taps: dict, device):
    if device not in taps["device"]:
        taps["device"][device] = (torch.from_numpy(taps["table"]).to(device), torch.from_numpy(taps["weights"]).to(device))
    return taps["device"][device]


def vqa_resized_view_f32(clip: torch.Tensor, frames: torch.Tensor, size, mean, std, antialias: bool = True, cols: bool = False) -> torch.Tensor:
    """clip: an [F,3,H,W] view (uint8, or float32 / bfloat16 in [0,1]; any strides, no copy), ``frames`` int32 [T] on the device, ``size``
    = (oh, ow) -> float32 [T,oh,ow,3]: every picked frame resized bilinearly (``resize_taps``, both axes) in fp64 on X (the uint8 value
    or 255 v), then (X - mean) / std, rounded once.  ``cols``: the same values as the (2,4,4) patch embedding's GEMM rows, float32
    [T/2,oh/4,ow/4,96], in ``vqa_fragments_f32``'s column order (csrc/convnext3d.hip)."""
    if clip.dim() != 4 or clip.shape[1] != 3 or not clip.is_cuda:
        raise ValueError(f"vqa_resized_view_f32: need an [F,3,H,W] view on the HIP device, got {tuple(clip.shape)} on {clip.device}")
    _strided_on_device("vqa_resized_view_f32", clip)
    L.require_cuda(frames)
    if frames.dtype != torch.int32 or frames.dim() != 1 or frames.shape[0] == 0:
        raise ValueError("vqa_resized_view_f32: frames must be int32 [T], T >= 1")
    T, (oh, ow) = frames.shape[0], (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1 or (cols and (T % 2 or oh % 4 or ow % 4)):
        raise ValueError(f"vqa_resized_view_f32: the patch rows need an even T and view sides that are multiples of 4, got {T} x {oh} x {ow}")
    ty, tx = resize_taps(clip.shape[2], oh, antialias), resize_taps(clip.shape[3], ow, antialias)
    (ytab, yw), (xtab, xw) = _taps_on(ty, clip.device), _taps_on(tx, clip.device)
    out = torch.empty((T // 2, oh // 4, ow // 4, 96) if cols else (T, oh, ow, 3), dtype=torch.float32, device=clip.device)
    v = _image_view(clip)
    L.check(L.load().dove_vqa_resized_view_f32(C.byref(v), clip.shape[0], clip.shape[2], clip.shape[3], L.ptr(frames), T, L.ptr(ytab), L.ptr(yw),
                                               ty["max"], L.ptr(xtab), L.ptr(xw), tx["max"], oh, ow, (C.c_double * 3)(*map(float, mean)),
                                               (C.c_double * 3)(*map(float, std)), int(bool(cols)), L.ptr(out), L.stream_ptr()),
            "dove_vqa_resized_view_f32")
    return out


# ---- MANIQA (csrc/maniqa.hip): the batched strided GEMM, row softmax, 2-D window attention, crop gather, scale-add-transpose, fp64 head ----
BMM_B_TRANSPOSED, BMM_STORE_TRANSPOSED, BMM_BIAS_ROWS = 1, 2, 4      # DOVE_BMM_* of include/dove_hip.h


def _span(t: torch.Tensor) -> tuple:
    """[first byte, past the last byte) of the memory a strided view reaches."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    return t.data_ptr(), t.data_ptr() + t.element_size() * (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1)


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (a0, a1), (b0, b1) = _span(a), _span(b)
    return a0 < b1 and b0 < a1


def _same_view(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _rows3(t: torch.Tensor, what: str, name: str):
    """A float32 [B,R,C] or [R,C] operand with unit column stride -> (rows, cols, row stride, batch stride or None for a 2-D operand)."""
    if t.dtype != torch.float32 or t.dim() not in (2, 3) or t.numel() == 0 or (t.shape[-1] > 1 and t.stride(-1) != 1) or \
            (t.shape[-2] > 1 and t.stride(-2) < t.shape[-1]) or (t.dim() == 3 and t.stride(0) < 0):
        raise ValueError(f"{what}: {name} {tuple(t.shape)} {t.dtype} with strides {t.stride()} must be float32 [B,R,C] or [R,C] rows")
    ld = t.stride(-2) if t.shape[-2] > 1 else t.shape[-1]
    return t.shape[-2], t.shape[-1], ld, (None if t.dim() == 2 else (t.stride(0) if t.shape[0] > 1 else 0))


def bmm_f32_tiles() -> tuple:
    """(M, N, K) tile of ``bmm_f32``'s kernel; needs no device."""
    m, n, k = C.c_int(0), C.c_int(0), C.c_int(0)
    L.load().dove_bmm_f32_tiles(C.byref(m), C.byref(n), C.byref(k))
    return m.value, n.value, k.value


def bmm_f32_kernel_name(b_transposed: bool = False, store_transposed: bool = False) -> str:
    """The kernel ``bmm_f32`` runs for a layout; needs no device."""
    return L.load().dove_bmm_f32_kernel_name(BMM_B_TRANSPOSED * bool(b_transposed) + BMM_STORE_TRANSPOSED * bool(store_transposed)).decode()


def bmm_f32(a: torch.Tensor, b: torch.Tensor, *, b_transposed: bool = False, bias: torch.Tensor | None = None, bias_rows: bool = False,
            residual: torch.Tensor | None = None, alpha: float = 1.0, store_transposed: bool = False,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """Per batch, out = alpha (a b) (+ bias) (+ residual) in exact fp32 (csrc/maniqa.hip): every output is one fmaf chain over k ascending.
    ``a`` float32 [B,M,K] or [M,K] rows, ``b`` [B,K,N] / [K,N] rows, or with ``b_transposed`` [B,N,K] / [N,K] rows (q k^T); row and batch
    strides are free (multiples of 4; an expanded or 2-D operand is shared by the batch), K and N multiples of 4.  ``bias`` [N], or [M]
    with ``bias_rows``.  ``store_transposed``: out and ``residual`` are [B,N,M].  ``residual`` may be ``out``; ``out`` must not alias
    ``a`` or ``b``."""
    _strided_on_device("bmm_f32", a, b)
    M, K, lda, sa = _rows3(a, "bmm_f32", "a")
    if b_transposed:
        N, Kb, ldb, sb = _rows3(b, "bmm_f32", "b")
    else:
        Kb, N, ldb, sb = _rows3(b, "bmm_f32", "b")
    batches = {t.shape[0] for t in (a, b) if t.dim() == 3}
    if Kb != K or len(batches) > 1 or K % 4 or N % 4:
        raise ValueError(f"bmm_f32: a {tuple(a.shape)} and b {tuple(b.shape)} (transposed: {bool(b_transposed)}) must agree in K and the batch, "
                         f"K and N multiples of 4")
    B = batches.pop() if batches else 1
    sa, sb = sa or 0, sb or 0
    if any(v % 4 for v in (lda, ldb, sa, sb)) or a.data_ptr() % 16 or b.data_ptr() % 16:
        raise ValueError(f"bmm_f32: row strides {lda}, {ldb} and batch strides {sa}, {sb} must be multiples of 4 and a, b 16-byte aligned")
    shape = (N, M) if store_transposed else (M, N)
    if a.dim() == 3 or b.dim() == 3:
        shape = (B,) + shape
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    _strided_on_device("bmm_f32", out)
    for name, t in (("out", out), ("residual", residual)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda):
            raise ValueError(f"bmm_f32: {name} must be float32 {shape} on the device, got {t.dtype} {tuple(t.shape)}")
    _, _, ldo, so = _rows3(out, "bmm_f32", "out")
    if _overlap(out, a) or _overlap(out, b):
        raise ValueError("bmm_f32: out must not alias a or b (every output reads a row of a and a column of b)")
    ldr = sr = 0
    if residual is not None:
        _strided_on_device("bmm_f32", residual)
        _, _, ldr, sr = _rows3(residual, "bmm_f32", "residual")
        if _overlap(residual, out) and not _same_view(residual, out):
            raise ValueError("bmm_f32: residual must not alias out unless it is out")
    if bias is not None:
        L.require_cuda(bias)
        if bias.dtype != torch.float32 or bias.numel() != (M if bias_rows else N):
            raise ValueError(f"bmm_f32: bias must be float32 [{M if bias_rows else N}], got {bias.dtype} {tuple(bias.shape)}")
    flags = BMM_B_TRANSPOSED * bool(b_transposed) + BMM_STORE_TRANSPOSED * bool(store_transposed) + BMM_BIAS_ROWS * bool(bias is not None and bias_rows)
    L.check(L.load().dove_bmm_f32(L.ptr(a), lda, sa, L.ptr(b), ldb, sb, L.ptr(bias), L.ptr(residual), ldr, sr or 0, L.ptr(out), ldo, so or 0, B, M, N,
                                  K, float(alpha), flags, L.stream_ptr()), "dove_bmm_f32")
    return out


def softmax_rows_f32(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Softmax over the last axis of float32 [R,C] rows (any row stride): the true row maximum, the accurate expf, the row sum in a fixed
    order (csrc/maniqa.hip).  ``out`` may be ``x``."""
    _strided_on_device("softmax_rows_f32", x)
    if x.dim() != 2:
        raise ValueError(f"softmax_rows_f32: x {tuple(x.shape)} must be [R,C] rows")
    R, Cc, ldx, _ = _rows3(x, "softmax_rows_f32", "x")
    if out is None:
        out = torch.empty(R, Cc, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (R, Cc) or (_overlap(out, x) and not _same_view(out, x)):
        raise ValueError(f"softmax_rows_f32: out must be float32 {(R, Cc)} and x itself or apart from it")
    _strided_on_device("softmax_rows_f32", out)
    ldo = _rows3(out, "softmax_rows_f32", "out")[2]
    L.check(L.load().dove_softmax_rows_f32(L.ptr(x), ldx, R, Cc, L.ptr(out), ldo, L.stream_ptr()), "dove_softmax_rows_f32")
    return out


def window_attention_tiles() -> tuple:
    """(tile, longest window, widest head) of ``window_attention_f32``'s kernel; needs no device."""
    t, n, d = C.c_int(0), C.c_int(0), C.c_int(0)
    L.load().dove_window_attention_tiles(C.byref(t), C.byref(n), C.byref(d))
    return t.value, n.value, d.value


def window_attention_f32(qkv: torch.Tensor, heads: int, table: torch.Tensor, index: torch.Tensor, *, scale: float | None = None,
                         region: torch.Tensor | None = None) -> torch.Tensor:
    """qkv float32 [W,N,3 heads d] (q, k, v side by side; d a multiple of 32 up to 192, N <= 64), ``table`` float32 [R,heads], ``index``
    int32 [N,N] -> float32 [W,N,heads d]: softmax(scale q k^T + table[index] + mask) v per window and head on the fp32 MFMA
    (csrc/maniqa.hip).  ``region`` int32 [w,N] (w divides W: the windows of one sample): -100 between tokens of different ids.  ``scale``
    defaults to 1 / sqrt(d)."""
    L.require_cuda(qkv, table, index, region)
    if qkv.dtype != torch.float32 or qkv.dim() != 3 or qkv.numel() == 0 or heads < 1 or qkv.shape[2] % (3 * heads):
        raise ValueError(f"window_attention_f32: qkv {tuple(qkv.shape)} {qkv.dtype} must be float32 [W,N,3 heads d] for {heads} heads")
    Wn, N, _ = qkv.shape
    d = qkv.shape[2] // (3 * heads)
    _, max_n, max_d = window_attention_tiles()
    if N > max_n or d % 32 or d > max_d:
        raise ValueError(f"window_attention_f32: windows of {N} tokens and heads of {d} (at most {max_n} tokens; heads a multiple of 32 up to {max_d})")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != heads or table.shape[0] == 0:
        raise ValueError(f"window_attention_f32: the bias table must be float32 [R,{heads}], got {table.dtype} {tuple(table.shape)}")
    if index.dtype != torch.int32 or tuple(index.shape) != (N, N):
        raise ValueError(f"window_attention_f32: index must be int32 {(N, N)}, got {index.dtype} {tuple(index.shape)}")
    idw = 1
    if region is not None:
        if region.dtype != torch.int32 or region.dim() != 2 or region.shape[1] != N or region.shape[0] == 0 or Wn % region.shape[0]:
            raise ValueError(f"window_attention_f32: region must be int32 [w,{N}] with w dividing {Wn}, got {region.dtype} {tuple(region.shape)}")
        idw = region.shape[0]
    D = heads * d
    out = torch.empty(Wn, N, D, dtype=torch.float32, device=qkv.device)
    L.check(L.load().dove_window_attention_f32(
        L.ptr(qkv), C.c_void_p(qkv.data_ptr() + 4 * D), C.c_void_p(qkv.data_ptr() + 8 * D), 3 * D, Wn, N, heads, d,
        1.0 / math.sqrt(d) if scale is None else float(scale), L.ptr(table), table.shape[0], L.ptr(index), L.ptr(region), idw, L.ptr(out), D,
        L.stream_ptr()), "dove_window_attention_f32")
    return out


def maniqa_crops_f32(img: torch.Tensor, origins: torch.Tensor, side: int, patch: int) -> torch.Tensor:
    """img: an [N,1|3,H,W] view (uint8 read as u / 255, float32 or bfloat16 in [0,1]; any strides, no copy), ``origins`` int32 [crops,2]
    (row, column) on the device -> float32 [N crops (side / patch)^2, 3 patch^2]: every crop's (v - 0.5) / 0.5 in fp64, rounded once, as
    the rows of the patch embedding's GEMM (column c patch^2 + dy patch + dx; csrc/maniqa.hip)."""
    if img.dim() != 4 or img.shape[1] not in (1, 3) or not img.is_cuda:
        raise ValueError(f"maniqa_crops_f32: need an [N,1|3,H,W] view on the HIP device, got {tuple(img.shape)} on {img.device}")
    _strided_on_device("maniqa_crops_f32", img)
    L.require_cuda(origins)
    N, Cc, H, W = img.shape
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] == 0:
        raise ValueError("maniqa_crops_f32: origins must be int32 [crops,2]")
    if patch < 1 or side < patch or side % patch or H < side or W < side:
        raise ValueError(f"maniqa_crops_f32: crops of {side} (a multiple of the patch {patch}) do not fit a {H} x {W} frame")
    crops, g = origins.shape[0], side // patch
    out = torch.empty(N * crops * g * g, 3 * patch * patch, dtype=torch.float32, device=img.device)
    if N == 0:
        return out
    v = _image_view(img)
    L.check(L.load().dove_maniqa_crops_f32(C.byref(v), N, Cc, H, W, L.ptr(origins), crops, side, patch, L.ptr(out), L.stream_ptr()),
            "dove_maniqa_crops_f32")
    return out


def maniqa_tokens_f32(emb: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """emb float32 [n T,D] patch embeddings, cls [D], pos [T + 1,D] -> float32 [n,T + 1,D]: cls + pos[0], then emb + pos[1 + t]."""
    L.require_cuda(emb, cls, pos)
    if any(t.dtype != torch.float32 for t in (emb, cls, pos)) or emb.dim() != 2 or pos.dim() != 2 or pos.shape[0] < 2 or \
            pos.shape[1] != emb.shape[1] or cls.numel() != emb.shape[1] or emb.shape[0] == 0 or emb.shape[0] % (pos.shape[0] - 1):
        raise ValueError(f"maniqa_tokens_f32: emb {tuple(emb.shape)} must be float32 [n T,D] with pos {tuple(pos.shape)} = [T + 1,D] and cls [D]")
    T, D = pos.shape[0] - 1, emb.shape[1]
    n = emb.shape[0] // T
    out = torch.empty(n, T + 1, D, dtype=torch.float32, device=emb.device)
    L.check(L.load().dove_maniqa_tokens_f32(L.ptr(emb), L.ptr(cls), L.ptr(pos), n, T, D, L.ptr(out), L.stream_ptr()), "dove_maniqa_tokens_f32")
    return out


def mix_f32(a: torch.Tensor, r: torch.Tensor | None = None, alpha: float = 1.0, transpose: bool = False,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """out = alpha a (+ r), each step rounded on its own, on float32 [B,R,C] or [R,C] rows (free row and batch strides); ``transpose``:
    out is [B,C,R].  Without ``transpose`` out may be ``a`` or ``r``; with it, it must be apart from both (csrc/maniqa.hip)."""
    _strided_on_device("mix_f32", a)
    R, Cc, lda, sa = _rows3(a, "mix_f32", "a")
    B = a.shape[0] if a.dim() == 3 else 1
    ldr = sr = 0
    if r is not None:
        _strided_on_device("mix_f32", r)
        if r.shape != a.shape:
            raise ValueError(f"mix_f32: r {tuple(r.shape)} must have a's shape {tuple(a.shape)}")
        _, _, ldr, sr = _rows3(r, "mix_f32", "r")
    shape = tuple(a.shape[:-2]) + ((Cc, R) if transpose else (R, Cc))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"mix_f32: out must be float32 {shape}, got {tuple(out.shape)}")
    _strided_on_device("mix_f32", out)
    _, _, ldo, so = _rows3(out, "mix_f32", "out")
    for t in (a, r):
        if t is not None and _overlap(out, t) and (transpose or not _same_view(out, t)):
            raise ValueError("mix_f32: out must not alias an input" + (" under transpose" if transpose else " unless it is that input"))
    L.check(L.load().dove_mix_f32(L.ptr(a), lda, sa or 0, L.ptr(r), ldr, sr or 0, float(alpha), B, R, Cc, int(bool(transpose)), L.ptr(out), ldo,
                                  so or 0, L.stream_ptr()), "dove_mix_f32")
    return out


def maniqa_score(hidden: torch.Tensor, wf: torch.Tensor, bf: torch.Tensor, ww: torch.Tensor, bw: torch.Tensor, want_crops: bool = False):
    """hidden float32 [frames,crops,positions,2 hid] (the two branches' ReLU'd hidden units side by side), wf / ww float32 [hid], bf / bw
    [1] -> float64 [frames]: per position f = relu(wf . h + bf), w = sigmoid(ww . h' + bw) in fp64; per crop sum f w / sum w; the mean
    over a frame's crops, every sum in a fixed order.  ``want_crops``: also the crops' scores, float64 [frames,crops]."""
    L.require_cuda(hidden, wf, bf, ww, bw)
    if hidden.dtype != torch.float32 or hidden.dim() != 4 or hidden.numel() == 0 or hidden.shape[3] % 2:
        raise ValueError(f"maniqa_score: hidden {tuple(hidden.shape)} {hidden.dtype} must be float32 [frames,crops,positions,2 hid]")
    n, crops, T, two = hidden.shape
    hid = two // 2
    if any(t.dtype != torch.float32 for t in (wf, bf, ww, bw)) or wf.numel() != hid or ww.numel() != hid or bf.numel() != 1 or bw.numel() != 1:
        raise ValueError(f"maniqa_score: need float32 wf [{hid}], bf [1], ww [{hid}], bw [1]")
    out, per_crop = torch.empty(n, dtype=torch.float64, device=hidden.device), torch.empty(n, crops, dtype=torch.float64, device=hidden.device)
    L.check(L.load().dove_maniqa_score(L.ptr(hidden), two, n, crops, T, hid, L.ptr(wf), L.ptr(bf), L.ptr(ww), L.ptr(bw), L.ptr(per_crop), L.ptr(out),
                                       L.stream_ptr()), "dove_maniqa_score")
    return (out, per_crop) if want_crops else out
