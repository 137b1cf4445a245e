"""What the metric networks' weights share, written once: the state-dict check, the weight packing, the rule-generated state dicts of
the tests and tools, the weights object that uploads itself once per device, the host tables that do the same, and the MLP half of a
pre-LN transformer block.

This module imports none of the metric modules; percep, flow, clipiqa, musiq, fastvqa, dover and maniqa import it.  A metric module keeps the shapes of
its checkpoint, its packing (what is folded, fused or split) and the rule of its random draws."""
from __future__ import annotations

import dataclasses
import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops


# ---------------------------------------------------------------- state dicts ----------------------------------------------------------------
def strip(sd: dict) -> dict:
    """A top-level ``state_dict`` unwrapped and DataParallel's ``module.`` prefix removed."""
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def checked(sd: dict, want: dict, what: str, exact: bool = False, say_shape: bool = True) -> dict:
    """``sd`` if it has every name of ``want`` with its shape, else ValueError.  ``exact``: an entry outside ``want`` is refused too.
    ``say_shape``: a missing entry's message ends with the shape it should have."""
    for name, shape in want.items():
        if name not in sd:
            raise ValueError(f"{what}: {name} is missing" + (f" (expected shape {tuple(shape)})" if say_shape else ""))
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f"{what}: {name} has shape {tuple(sd[name].shape)}, expected {tuple(shape)}")
    if exact:
        for name in sd:
            if name not in want:
                raise ValueError(f"{what}: unexpected entry {name}")
    return sd


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,kh,kw] -> the kernel's [kh,kw,Cin,Cout] float32."""
    return w.float().permute(2, 3, 1, 0).contiguous()


def pack_linear_weight(w: torch.Tensor) -> torch.Tensor:
    """[out,in...] -> the 1 x 1 walk's [1,1,in,out] float32."""
    return w.detach().float().flatten(1).t().contiguous()[None, None]


def bn_affine(gamma, beta, mean, var, eps: float):
    """Eval-mode BatchNorm as y = scale * x + shift -> (scale, shift) in fp64."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() - mean.double() * scale


# ------------------------------------------------------------ rule-generated states ------------------------------------------------------------
def random_tensors(shapes: dict, seed: int, key, rule, draw=()) -> dict:
    """name -> float32 tensor of ``rule(name, shape, rng)`` for every (name, shape), each with its own numpy generator keyed by
    (seed, crc32 of ``key(name)``, *draw): a tensor's values depend on nothing but its key."""
    out = {}
    for name, shape in shapes.items():
        rng = np.random.default_rng([int(seed), zlib.crc32(key(name).encode()), *draw])
        out[name] = torch.from_numpy(np.asarray(rule(name, shape, rng), dtype=np.float32))
    return out


def he_normal(rng, shape):
    """Normal with std sqrt(2 / fan-in)."""
    return rng.standard_normal(shape) * math.sqrt(2.0 / float(np.prod(shape[1:])))


def fan_in_normal(rng, shape):
    """Normal with std 1 / sqrt(fan-in)."""
    return rng.standard_normal(shape) / math.sqrt(float(np.prod(shape[1:])))


# ------------------------------------------------------------------ devices ------------------------------------------------------------------
def _moved(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device)
    if isinstance(v, dict):
        return {k: _moved(x, device) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_moved(x, device) for x in v)
    if dataclasses.is_dataclass(v) and not isinstance(v, type):
        return dataclasses.replace(v, **{f.name: _moved(getattr(v, f.name), device) for f in dataclasses.fields(v)})
    return v


@dataclass
class Weights:
    """Base of a network's weights: a dataclass whose public fields hold the packed tensors in dicts, lists, tuples and dataclasses."""
    device: torch.device = torch.device("cpu")
    _copies: dict = field(default_factory=dict, repr=False)      # device -> the copy made for it, so a metric uploads once

    def to(self, device):
        """``self`` on its own device, else the one copy on ``device`` (``cuda``: the current index) with every tensor moved."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        if device not in self._copies:
            public = {f.name: _moved(getattr(self, f.name), device) for f in dataclasses.fields(self) if not f.name.startswith("_")}
            self._copies[device] = type(self)(**{**public, "device": device})
        return self._copies[device]


def nearest_index(count: int, grid: int) -> np.ndarray:
    """torch's nearest-neighbour ``F.interpolate`` of arange(grid) to ``count`` points: floor(i * (grid / count)) in float32, at most
    grid - 1."""
    scale = np.float32(grid) / np.float32(count)
    return np.minimum(np.floor(np.arange(count, dtype=np.float32) * scale).astype(np.int64), grid - 1)


def device_tables(geo: dict, device, names) -> tuple:
    """The host tables ``geo[name]`` (tensor, array or None) on ``device``, uploaded once and kept in ``geo['device']``."""
    if device not in geo["device"]:
        up = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device)
        geo["device"][device] = tuple(up(geo[n]) for n in names)
    return geo["device"][device]


# -------------------------------------------------------------------- walk --------------------------------------------------------------------
def prenorm_mlp_f32(rows: torch.Tensor, h: torch.Tensor, p: dict, norm: str, fc1: str, fc2: str, eps: float) -> None:
    """The MLP half of a pre-LN block on token rows float32 [M,C], in place: rows += fc2(gelu(fc1(LayerNorm(rows)))).  ``h`` [M,C] takes
    the norm's output; ``p`` holds ``{norm,fc1,fc2}.{weight,bias}``."""
    ops.layernorm_f32(rows, p[norm + ".weight"], p[norm + ".bias"], eps, out=h)
    m = ops.linear_f32(h, p[fc1 + ".weight"], p[fc1 + ".bias"])
    ops.gelu_f32(m, out=m)
    ops.linear_f32(m, p[fc2 + ".weight"], p[fc2 + ".bias"], residual=rows, out=rows)
