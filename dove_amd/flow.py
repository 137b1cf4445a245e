"""Optical flow (RAFT, the basic model) and the E*warp temporal-consistency metric on the GPU, all in fp32 (csrc/flow.hip).

The network is the reference's ``finetune/utils/RAFT`` (``raft.py``, ``extractor.py``, ``update.py``, ``corr.py``): two encoders at 1/8
resolution, the all-pairs correlation pyramid, and ``iters`` rounds of lookup -> motion encoder -> separable ConvGRU -> flow head, with
the convex upsampling of the last round.  This module walks it in Python, as ``vae.py`` walks the VAE; every operator is a kernel of the
library (``ops.conv2d_f32`` ...) and activations are channels-last fp32 whose producers write straight into the concat buffers
``[h | inp | motion | flow]``.  The flow itself is the state (the reference keeps ``coords1`` and subtracts the grid; in exact arithmetic
the same thing).

The metric is defined here - the reference's ``eval_ewarp.py`` imports an ``ewarp`` module it does not ship - from Lai et al.'s warping
error on the reference's own ``flow_warp`` and ``fbConsistencyCheck``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import lib as L
from . import ops
from .iqa import load_state_dict
from .netweights import Weights, bn_affine, checked, he_normal, pack_conv_weight, random_tensors, strip     # flow.pack_conv_weight stays a name

BN_EPS = 1e-5
HDIM = CDIM = 128
MIN_SIDE = 128          # padded H, W below this leave the coarsest correlation level 1 px wide, where the reference divides by W - 1 = 0
COUNTERS = {"fnet_frames": 0, "cnet_frames": 0, "pair_groups": 0}     # launches of the walk, for tests and tools


# ------------------------------------------------------------------ weights ------------------------------------------------------------------
def _encoder_shapes(prefix: str, out_dim: int, batch_norm: bool) -> dict:
    s = {}

    def bn(name, c):
        if batch_norm:
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                s[f"{name}.{leaf}"] = (c,)
            s[f"{name}.num_batches_tracked"] = ()

    def conv(name, cout, cin, kh, kw):
        s[f"{name}.weight"] = (cout, cin, kh, kw)
        s[f"{name}.bias"] = (cout,)

    bn(f"{prefix}.norm1", 64)
    conv(f"{prefix}.conv1", 64, 3, 7, 7)
    cin = 64
    for layer, planes, stride in (("layer1", 64, 1), ("layer2", 96, 2), ("layer3", 128, 2)):
        for blk in (0, 1):
            p = f"{prefix}.{layer}.{blk}"
            conv(f"{p}.conv1", planes, cin, 3, 3)
            conv(f"{p}.conv2", planes, planes, 3, 3)
            bn(f"{p}.norm1", planes)
            bn(f"{p}.norm2", planes)
            if blk == 0 and stride == 2:
                bn(f"{p}.norm3", planes)
                conv(f"{p}.downsample.0", planes, cin, 1, 1)
                bn(f"{p}.downsample.1", planes)           # the same module as norm3, registered a second time
            cin = planes
    conv(f"{prefix}.conv2", out_dim, 128, 1, 1)
    return s


def raft_param_shapes() -> dict:
    """name -> shape of the basic RAFT model's ``state_dict()`` (tests/golden/raft_state_shapes.json holds the reference's own list)."""
    s = {}
    s.update(_encoder_shapes("fnet", 256, False))
    s.update(_encoder_shapes("cnet", HDIM + CDIM, True))
    u = "update_block"
    for name, cout, cin, kh, kw in (("encoder.convc1", 256, 324, 1, 1), ("encoder.convc2", 192, 256, 3, 3), ("encoder.convf1", 128, 2, 7, 7),
                                    ("encoder.convf2", 64, 128, 3, 3), ("encoder.conv", 126, 256, 3, 3),
                                    ("gru.convz1", 128, 384, 1, 5), ("gru.convr1", 128, 384, 1, 5), ("gru.convq1", 128, 384, 1, 5),
                                    ("gru.convz2", 128, 384, 5, 1), ("gru.convr2", 128, 384, 5, 1), ("gru.convq2", 128, 384, 5, 1),
                                    ("flow_head.conv1", 256, 128, 3, 3), ("flow_head.conv2", 2, 256, 3, 3),
                                    ("mask.0", 256, 128, 3, 3), ("mask.2", 576, 256, 1, 1)):
        s[f"{u}.{name}.weight"] = (cout, cin, kh, kw)
        s[f"{u}.{name}.bias"] = (cout,)
    return s


def random_raft_state(seed: int) -> dict:
    """A rule-generated state dict of the basic model (tests and tools; a flow network that means nothing, with healthy magnitudes):
    one numpy generator per name; conv weights normal with std sqrt(2 / fan_in), conv biases 0.05 * normal, BatchNorm weight and
    running_var uniform in [0.5, 1.5], BatchNorm bias and running_mean 0.1 * normal.  ``downsample.1`` repeats ``norm3``."""
    def rule(name, shape, rng):
        leaf = name.rsplit(".", 1)[1]
        if len(shape) == 4:
            return he_normal(rng, shape)
        if leaf == "running_var" or (leaf == "weight" and len(shape) == 1):
            return rng.uniform(0.5, 1.5, shape)
        if leaf in ("running_mean",) or ".norm" in name or ".downsample.1." in name:
            return 0.1 * rng.standard_normal(shape)
        return 0.05 * rng.standard_normal(shape)

    shapes = raft_param_shapes()
    drawn = random_tensors({n: s for n, s in shapes.items() if not n.endswith(".num_batches_tracked")}, seed,
                           lambda name: name.replace(".downsample.1.", ".norm3."), rule)
    return {n: drawn[n] if n in drawn else torch.zeros((), dtype=torch.int64) for n in shapes}


def fold_batch_norm(weight, bias, running_mean, running_var, eps: float = BN_EPS):
    """Eval-mode BatchNorm as y = scale * x + shift, computed in fp64 -> (scale, shift) float32."""
    return tuple(t.float() for t in bn_affine(weight, bias, running_mean, running_var, eps))


@dataclass
class ConvLayer:
    w: torch.Tensor
    b: torch.Tensor
    scale: torch.Tensor | None = None
    shift: torch.Tensor | None = None


@dataclass
class RaftWeights(Weights):
    convs: dict = field(default_factory=dict)       # name -> ConvLayer

    @classmethod
    def load(cls, path: str, small: bool = False) -> "RaftWeights":
        """A ``raft-things.pth``-style checkpoint: a state dict, possibly with the ``module.`` prefix of DataParallel."""
        if small:
            raise NotImplementedError("the small RAFT model is not built: dove_amd.flow runs the basic model only")
        return cls.from_state_dict(load_state_dict(path))

    @classmethod
    def from_state_dict(cls, sd: dict) -> "RaftWeights":
        sd = strip(sd)
        if any(k.startswith("update_block.gru.convz.") or k.startswith("fnet.layer1.0.conv3.") for k in sd):
            raise NotImplementedError("this is a small-model RAFT checkpoint: dove_amd.flow runs the basic model only")
        checked(sd, raft_param_shapes(), "RAFT checkpoint", exact=True, say_shape=False)
        convs = {}

        def layer(name, norm=None):
            scale = shift = None
            if norm is not None:
                scale, shift = fold_batch_norm(*(sd[f"{norm}.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var")))
            return ConvLayer(pack_conv_weight(sd[f"{name}.weight"]), sd[f"{name}.bias"].float().contiguous(), scale, shift)

        for prefix in ("fnet", "cnet"):
            bn = prefix == "cnet"
            convs[f"{prefix}.conv1"] = layer(f"{prefix}.conv1", f"{prefix}.norm1" if bn else None)
            for lname, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
                for blk in (0, 1):
                    p = f"{prefix}.{lname}.{blk}"
                    convs[f"{p}.conv1"] = layer(f"{p}.conv1", f"{p}.norm1" if bn else None)
                    convs[f"{p}.conv2"] = layer(f"{p}.conv2", f"{p}.norm2" if bn else None)
                    if blk == 0 and stride == 2:
                        convs[f"{p}.downsample.0"] = layer(f"{p}.downsample.0", f"{p}.norm3" if bn else None)
        convs["fnet.conv2"] = layer("fnet.conv2")
        w, b = sd["cnet.conv2.weight"], sd["cnet.conv2.bias"].float()
        convs["cnet.conv2.net"] = ConvLayer(pack_conv_weight(w[:HDIM]), b[:HDIM].contiguous())         # tanh half
        convs["cnet.conv2.inp"] = ConvLayer(pack_conv_weight(w[HDIM:]), b[HDIM:].contiguous())         # relu half
        u = "update_block"
        for name in ("encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv", "gru.convq1", "gru.convq2",
                     "flow_head.conv1", "flow_head.conv2", "mask.0", "mask.2"):
            convs[name] = layer(f"{u}.{name}")
        for d in ("1", "2"):                                # z and r read the same input: one conv of 256 output channels
            w = torch.cat([sd[f"{u}.gru.convz{d}.weight"], sd[f"{u}.gru.convr{d}.weight"]], 0)
            b = torch.cat([sd[f"{u}.gru.convz{d}.bias"], sd[f"{u}.gru.convr{d}.bias"]], 0)
            convs[f"gru.convzr{d}"] = ConvLayer(pack_conv_weight(w), b.float().contiguous())
        return cls(convs=convs)


# ------------------------------------------------------------------ planning ------------------------------------------------------------------
def input_pad(h: int, w: int):
    """``InputPadder(dims, 'sintel')``: (left, right, top, bottom) of the replicate padding to multiples of 8, centred."""
    ph, pw = (((h // 8) + 1) * 8 - h) % 8, (((w // 8) + 1) * 8 - w) % 8
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def workspace_bytes(h: int, w: int, pairs: int) -> int:
    """Device bytes ``pairs`` frame pairs of padded size h x w need at once: the correlation pyramid ((h w / 64)^2 floats per pair and
    its three pools), the buffers of one update round, the feature maps, and the encoders' activations for 2 * pairs frames."""
    h8, w8 = h // 8, w // 8
    hw = h8 * w8
    corr = hw * sum((h8 >> l) * (w8 >> l) for l in range(4))
    per_pixel = 324 + 256 + 256 + 128 + 384 + 384 + 256 + 128 + 256 + 2 + 256 + 576 + 128      # one update round, the mask head, flow_up
    features = 2 * 256 + 256
    encoder = 2 * (4 * 64 * (h // 2) * (w // 2) + 3 * h * w)
    return 4 * pairs * (corr + hw * (per_pixel + features) + encoder)


def plan_pair_groups(n_pairs: int, h: int, w: int, free_bytes: int) -> list:
    """[(start, stop), ...] covering range(n_pairs): the largest groups whose ``workspace_bytes`` fit ``free_bytes``."""
    one = workspace_bytes(h, w, 1)
    if one > free_bytes:
        raise MemoryError(f"one {h}x{w} frame pair needs {one / 2**30:.1f} GiB for its all-pairs correlation volume and activations, "
                          f"{free_bytes / 2**30:.1f} GiB are free: compute the flow at a lower resolution")
    g = max(1, min(n_pairs, free_bytes // one))
    return [(s, min(s + g, n_pairs)) for s in range(0, n_pairs, g)]


def _free_bytes(device) -> int:
    free, _ = torch.cuda.mem_get_info(device)
    cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return int(0.8 * (free + cached))


# ------------------------------------------------------------------ the walk ------------------------------------------------------------------
def _conv(W: RaftWeights, name: str, x, stride=1, act=L.ACT_NONE, **kw):
    l = W.convs[name]
    return ops.conv2d_f32(x, l.w, l.b, stride=stride, act=act, scale=l.scale, shift=l.shift, **kw)


def _encoder(W: RaftWeights, prefix: str, x: torch.Tensor) -> torch.Tensor:
    """BasicEncoder up to layer3: x [N,H,W,3] -> [N,H/8,W/8,128].  fnet: InstanceNorm kernels; cnet: BatchNorm folded into the convs."""
    inst = prefix == "fnet"
    y = _conv(W, f"{prefix}.conv1", x, 2, L.ACT_NONE if inst else L.ACT_RELU)
    if inst:
        y = ops.instance_norm_f32(y, relu=True)
    for lname, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        for blk in (0, 1):
            s = stride if blk == 0 else 1
            p = f"{prefix}.{lname}.{blk}"
            if inst:
                a = ops.instance_norm_f32(_conv(W, f"{p}.conv1", y, s), relu=True)
                b = _conv(W, f"{p}.conv2", a)
                sc = ops.instance_norm_f32(_conv(W, f"{p}.downsample.0", y, s)) if s == 2 else y
                y = ops.instance_norm_f32(b, relu=True, resid=sc)
            else:
                a = _conv(W, f"{p}.conv1", y, s, L.ACT_RELU)
                b = _conv(W, f"{p}.conv2", a, 1, L.ACT_RELU)
                sc = _conv(W, f"{p}.downsample.0", y, s) if s == 2 else y
                y = ops.add_f32(sc, b, relu=True)
    return y


def _features(W: RaftWeights, x: torch.Tensor, chunk: int) -> torch.Tensor:
    """fnet: [F,H,W,3] -> [F,H/8,W/8,256], ``chunk`` frames at a time (InstanceNorm is per frame: the split changes nothing)."""
    out = []
    for s in range(0, x.shape[0], chunk):
        COUNTERS["fnet_frames"] += min(chunk, x.shape[0] - s)
        out.append(_conv(W, "fnet.conv2", _encoder(W, "fnet", x[s:s + chunk])))
    return torch.cat(out) if len(out) > 1 else out[0]


def _context(W: RaftWeights, x: torch.Tensor, chunk: int) -> torch.Tensor:
    """cnet: [F,H,W,3] -> [F,H/8,W/8,256] = [tanh(net) | relu(inp)], each half written into its slice."""
    F, H, Wd, _ = x.shape
    out = torch.empty(F, H // 8, Wd // 8, HDIM + CDIM, dtype=torch.float32, device=x.device)
    for s in range(0, F, chunk):
        COUNTERS["cnet_frames"] += min(chunk, F - s)
        y = _encoder(W, "cnet", x[s:s + chunk])
        _conv(W, "cnet.conv2.net", y, 1, L.ACT_TANH, out=out[s:s + chunk, :, :, :HDIM])
        _conv(W, "cnet.conv2.inp", y, 1, L.ACT_RELU, out=out[s:s + chunk, :, :, HDIM:])
    return out


def _iterate(W: RaftWeights, fmap1, fmap2, ctx, iters: int, flow_init, taps):
    """One group of pairs: fmaps [B,h,w,256], ctx [B,h,w,256], flow_init [B,h,w,2] or None -> (flow_low [B,h,w,2], flow_up [B,2,8h,8w])."""
    B, h, w, _ = fmap1.shape
    dev = fmap1.device
    COUNTERS["pair_groups"] += 1
    levels = ops.corr_pyramid_f32(fmap1, fmap2)
    hx = torch.empty(B, h, w, 384, dtype=torch.float32, device=dev)         # [h | inp | motion features | flow]
    rhx = torch.empty_like(hx)
    corflo = torch.empty(B, h, w, 256, dtype=torch.float32, device=dev)     # [cor | flo]
    corr = torch.empty(B, h, w, 324, dtype=torch.float32, device=dev)
    hx[..., :256] = ctx
    flow = hx[..., 382:]
    if flow_init is None:
        flow.zero_()
    else:
        flow.copy_(flow_init)
    net = hx[..., :HDIM]
    mask = None
    for it in range(iters):
        ops.corr_lookup_f32(levels, flow, add_grid=True, out=corr)
        cor = _conv(W, "encoder.convc1", corr, 1, L.ACT_RELU)
        _conv(W, "encoder.convc2", cor, 1, L.ACT_RELU, out=corflo[..., :192])
        flo = _conv(W, "encoder.convf1", flow, 1, L.ACT_RELU)
        _conv(W, "encoder.convf2", flo, 1, L.ACT_RELU, out=corflo[..., 192:])
        _conv(W, "encoder.conv", corflo, 1, L.ACT_RELU, out=hx[..., 256:382])
        for d in ("1", "2"):                                                # 1 x 5, then 5 x 1
            zr = _conv(W, f"gru.convzr{d}", hx, 1, L.ACT_SIGMOID)
            ops.gru_gate_f32(zr[..., HDIM:], hx, HDIM, rhx)
            q = _conv(W, f"gru.convq{d}", rhx, 1, L.ACT_TANH)
            ops.gru_update_f32(zr[..., :HDIM], q, hx)
        delta = _conv(W, "flow_head.conv2", _conv(W, "flow_head.conv1", net, 1, L.ACT_RELU))
        if taps is not None and it == 0:
            taps.setdefault("corr0", []).append(corr.clone())
            taps.setdefault("delta0", []).append(delta.clone())
        if it == iters - 1:                                                 # only the last round's upsampled flow is returned
            mask = _conv(W, "mask.2", _conv(W, "mask.0", net, 1, L.ACT_RELU), out_mul=0.25)
        ops.add_f32(flow, delta, out=flow)
    flow_low = flow.contiguous()
    if mask is None:                                                        # iters == 0: the initial flow, upsampled by its own mask
        mask = _conv(W, "mask.2", _conv(W, "mask.0", net, 1, L.ACT_RELU), out_mul=0.25)
    return flow_low, ops.convex_upsample_f32(flow, mask)


def _prepare(images: torch.Tensor):
    """[N,3,H,W] in [-1,1] -> (channels-last padded [N,H',W',3] float32, pad)."""
    pad = input_pad(images.shape[-2], images.shape[-1])
    x = torch.nn.functional.pad(images.float(), pad, mode="replicate") if any(pad) else images.float()
    if x.shape[-2] < MIN_SIDE or x.shape[-1] < MIN_SIDE:
        raise ValueError(f"RAFT needs padded sides of at least {MIN_SIDE} px (got {x.shape[-2]}x{x.shape[-1]}): the coarsest correlation "
                         "level would be 1 px wide")
    return x.permute(0, 2, 3, 1).contiguous(), pad


def _unpad(x: torch.Tensor, pad):
    l, r, t, b = pad
    return x[..., t:x.shape[-2] - b, l:x.shape[-1] - r].contiguous()


def _run_pairs(W, fmaps, ctxs, i1, i2, ic, iters, flow_init, group, taps):
    n, (h8, w8) = len(i1), fmaps.shape[1:3]
    dev = fmaps.device
    if group is None:
        groups = plan_pair_groups(n, h8 * 8, w8 * 8, _free_bytes(dev))
    else:
        groups = [(s, min(s + group, n)) for s in range(0, n, group)]
    lows, ups = [], []
    i1, i2, ic = (torch.as_tensor(v, device=dev) for v in (i1, i2, ic))
    for s, e in groups:
        fi = None if flow_init is None else flow_init[s:e].permute(0, 2, 3, 1)
        lo, up = _iterate(W, fmaps[i1[s:e]], fmaps[i2[s:e]], ctxs[ic[s:e]], iters, fi, taps)
        lows.append(lo.permute(0, 3, 1, 2))
        ups.append(up)
    return torch.cat(lows).contiguous(), torch.cat(ups)


def _encoder_chunk(dev, h, w, group):
    return max(1, 2 * (group if group is not None else max(1, _free_bytes(dev) // workspace_bytes(h, w, 1))))


@torch.no_grad()
def raft_flow(weights: RaftWeights, img1: torch.Tensor, img2: torch.Tensor, iters: int = 20, flow_init: torch.Tensor | None = None,
              group: int | None = None, taps: dict | None = None):
    """RAFT's ``forward(image1, image2, iters, flow_init, test_mode=True)`` -> (flow_low [N,2,H'/8,W'/8], flow_up [N,2,H,W]).

    Images are [N,3,H,W] in [-1, 1] on the HIP device.  Sizes that are no multiple of 8 are padded as ``InputPadder(dims, 'sintel')``
    pads them and ``flow_up`` is cropped back (``flow_low`` and ``flow_init`` live on the padded 1/8 grid).  Pairs run in groups sized
    from ``workspace_bytes`` against the free memory (``group`` forces a size); a pair's result does not depend on the grouping.
    ``taps``: a dict that receives the channels-last ``fmap1``, and the first round's correlation lookup and ``delta_flow``."""
    if img1.dim() != 4 or img1.shape[1] != 3 or img1.shape != img2.shape:
        raise ValueError(f"raft_flow: images {tuple(img1.shape)} / {tuple(img2.shape)} must be the same [N,3,H,W]")
    if not (img1.is_cuda and img2.is_cuda):
        raise RuntimeError("raft_flow needs the images on the HIP device (`cuda`); there is no CPU path")
    with torch.cuda.device(img1.device):
        W = weights.to(img1.device)
        n = img1.shape[0]
        x, pad = _prepare(torch.cat([img1, img2]))
        chunk = _encoder_chunk(x.device, x.shape[1], x.shape[2], group)
        fmaps = _features(W, x, chunk)
        ctxs = _context(W, x[:n], chunk)
        if taps is not None:
            taps["fmap1"] = fmaps[:n].clone()
        idx = list(range(n))
        low, up = _run_pairs(W, fmaps, ctxs, idx, [n + i for i in idx], idx, iters, flow_init, group, taps)
        if taps is not None:
            for k in ("corr0", "delta0"):
                taps[k] = torch.cat(taps[k])
        return low, _unpad(up, pad)


def frames_to_images(frames_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [F,H,W,3] -> float32 [F,3,H,W] in [-1, 1]: 2 * (v / 255) - 1 with an IEEE division, as ``to_tensor`` on the host gives it
    (a division by a Python scalar on the device is a multiplication by the rounded reciprocal)."""
    x = frames_u8.permute(0, 3, 1, 2).float()
    return 2.0 * (x / torch.full((), 255.0, device=x.device)) - 1.0


@torch.no_grad()
def clip_flows(weights: RaftWeights, frames_u8: torch.Tensor, iters: int = 20, group: int | None = None):
    """frames uint8 [F,H,W,3] -> (fw, bw) float32 [F-1,2,H,W] on the device: the flows t -> t+1 and t+1 -> t of every neighbouring pair.
    Both encoders run once per frame, not once per pair and direction."""
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8 or frames_u8.shape[0] < 2:
        raise ValueError(f"clip_flows: frames {tuple(frames_u8.shape)} {frames_u8.dtype} must be uint8 [F>=2,H,W,3]")
    dev = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        W = weights.to(dev)
        F = frames_u8.shape[0]
        x, pad = _prepare(frames_to_images(frames_u8.to(dev)))
        chunk = _encoder_chunk(dev, x.shape[1], x.shape[2], group)
        fmaps, ctxs = _features(W, x, chunk), _context(W, x, chunk)
        a, b = list(range(F - 1)), list(range(1, F))
        _, up = _run_pairs(W, fmaps, ctxs, a + b, b + a, a + b, iters, None, group, None)
        up = _unpad(up, pad)
        return up[:F - 1].contiguous(), up[F - 1:].contiguous()


# ------------------------------------------------------------------ the metric ------------------------------------------------------------------
def summarize_pairs(sums) -> dict:
    """``sums`` [P,2] = per pair {masked squared error over the 3 channels, mask count} -> the clip's warping error.

    E_t = sum / (3 * count); the clip value is the mean of E_t over pairs that have a valid pixel, times 1000 (the paper's x 10^-3 unit);
    NaN when no pair has one."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    ok = sums[:, 1] > 0
    per_pair = np.where(ok, sums[:, 0] / (3.0 * np.where(ok, sums[:, 1], 1.0)), np.nan)
    value = float(1000.0 * per_pair[ok].mean()) if ok.any() else float("nan")
    return {"warping_error": value, "pairs": int(len(sums)), "pairs_without_valid_pixels": int((~ok).sum()),
            "per_pair": [float(v) for v in per_pair]}


@torch.no_grad()
def warping_error(frames_u8: torch.Tensor, weights: RaftWeights, iters: int = 20, group: int | None = None) -> dict:
    """E*warp of one clip, uint8 [F,H,W,3].  With images in [0, 1] and C = 3, per pair
    E_t = sum_p M_p sum_c (I_t - warp(I_t+1, F_t->t+1))^2 / (C * sum_p M_p), M the forward-backward consistency mask times "the sample
    position lies inside the frame"; see ``summarize_pairs`` for the clip value."""
    fw, bw = clip_flows(weights, frames_u8, iters, group)
    with torch.cuda.device(fw.device):
        fr = frames_u8.to(fw.device).contiguous()
        sums, _, _ = ops.flow_warp_error(fr[:-1], fr[1:], fw, bw)
        return summarize_pairs(sums.cpu().numpy())
