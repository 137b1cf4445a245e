"""Degradation synthesis: ground-truth frames -> a low-quality clip, on the GPU (csrc/degrade.hip).

The pipeline is the RealESRGAN-style two-stage one the DOVE paper's synthetic test sets come from (the reference's
finetune/datasets/degradation.py with finetune/configs/degradation.yaml): random blur, random resize, Gaussian / Poisson noise, JPEG, then
the same again with a shuffled tail that ends at 1 / scale of the input size.  It is split in two:

* ``Degrader(config, scale, seed).recipe(frames, height, width)`` draws every random parameter on the host and returns a **recipe**: a
  JSON-serialisable dict whose ``steps`` are concrete operator calls (blur-kernel family and parameters per frame, target size and mode,
  noise kind / level / gray / stream id, per-frame JPEG qualities).
* ``apply_recipe(frames_u8, recipe, frame0)`` runs a recipe on the device.  Every step works frame by frame, so a clip may be processed
  in blocks: ``frame0`` is the index of the block's first frame in the clip, and the result does not depend on the split.

The draws follow the reference's *distributions*, not its random streams: the reference mixes Python's ``random`` with numpy's global
state, so no seed reproduces it.  Here all host draws come from ``numpy.random.Generator(PCG64(seed))`` in one fixed order:

  for stage 1, then stage 2:  random_blur, random_resize, random_noise, random_jpeg, (random_mpeg: no draw from this generator);
  then the permutation of stage 2's degradation_with_shuffle, then its entries in the shuffled order (a group keeps its inner order).
  Every step first draws its ``prob`` uniform (also when ``prob`` is absent), then, if it runs:
    blur:   family, kernel size, sigma_x, sigma_y, angle, beta_gaussian, beta_plateau, omega; then per frame after the first the six
            ``*_step`` walk increments in that order (clipped to the parameter's range);
    resize: mode; without ``target_size``: up / down / keep, then the scale factor (not drawn for keep);
    noise:  kind, level, gray, then one walk increment per frame after the first;
    jpeg:   quality, then one walk increment per frame after the first (rounded and clipped as the reference does).
The device noise of a recipe uses ``dove_randn``'s Philox streams (recipe seed, stream id = the noise step's number in the recipe).

Video-codec steps (``random_mpeg``, ``RandomVideoCompression``) are recorded as skipped by default: nothing here encodes or decodes a real
bitstream.  ``Degrader(..., video_codec="sim")`` runs them as ``ops.vcodec_roundtrip`` instead (csrc/vcodec.hip; tests/vcodec_ref.py is
the definition): closed groups of ``gop`` frames, I then P frames with full-search integer motion per 16x16 macroblock, the H.264 4x4
transform and quantiser on Y'CbCr 4:2:0, and one QP per group found against ``bitrate`` bits per frame under an integer bit-count model.
It is what such a codec does to the pixels - blocking, ringing, errors that drift from frame to frame until the next I frame - and not a
codec: no sub-pel motion, no B frames, no intra macroblocks in P frames, no deblocking filter, no entropy coding, and the drawn codec name
(libx264 / h264 / mpeg4) is recorded without changing the arithmetic.  ``video_codec="sim-h264"`` draws exactly what ``"sim"`` draws and
adds ``"tools": ["intra16", "qpel", "deblock"]`` to each ``vcodec`` step: I frames predicted per macroblock from their neighbours,
quarter-sample motion and the in-loop deblocking filter (tests/vcodec_tools_ref.py is the definition); a step without ``tools`` runs as
``"sim"`` does.  The k-th codec step of a recipe draws from a generator of its own,
``PCG64([seed, VCODEC_STREAM, k])``: ``prob``, the codec name over ``codec_prob``, then ``bitrate = integers(lo, hi + 1)`` - so every
other step of the recipe is the same with and without the option.  The step couples the frames of a group: ``apply_recipe`` takes a
recipe with a ``vcodec`` step only in blocks that start and end on group boundaries (or at the recipe's last frame).

Other departures, each recorded or refused: ``resize_step != 0``, ``lanczos`` and unknown step types are refused; a blur-kernel size
whose half-width is not smaller than the current frame (where one reflection does not suffice) is left out of the size draw, and a blur
with no size left is recorded as skipped; a drawn target size is at least 1 (2 with ``is_size_even``).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

KERNEL_FAMILIES = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso", "sinc")
RESIZE_MODES = {"bilinear": 0, "bicubic": 1, "area": 2}          # L.RESIZE_*
RECIPE_VERSION = 1
_CODEC_STEPS = ("RandomVideoCompression",)
_NO_CODEC = "no video codec in this build"
VIDEO_CODECS = (None, "sim", "sim-h264")
VCODEC_TOOLS = ("intra16", "qpel", "deblock")                       # the names a vcodec step's "tools" may hold (ops.VCODEC_TOOLS)
VCODEC_STREAM = 0x76636F64                                       # "vcod": second word of the codec steps' own PCG64 seed
DEFAULT_GOP = 8


# ---- blur-kernel families ---------------------------------------------------------------------------------------------------------
def bessel_j1(x):
    """J1 by the trapezoid rule on Bessel's integral (1 / 2 pi) * int_0^2pi cos(t - x sin t) dt: the integrand is periodic and entire,
    so 256 nodes are exact to rounding for |x| < 100 (the error is of the size of J_255(x))."""
    x = np.asarray(x, dtype=np.float64)
    t = 2.0 * np.pi * np.arange(256) / 256.0
    return np.cos(t - x[..., None] * np.sin(t)).mean(-1)


def _grid(size: int):
    r = np.arange(size, dtype=np.float64) - (size - 1) / 2
    return np.meshgrid(r, r)                                     # x along columns, y along rows


def _inverse_covariance(sigma_x: float, sigma_y: float, angle: float) -> np.ndarray:
    """Inverse of R diag(sigma_x^2, sigma_y^2) R^T, R the rotation by ``angle``.  The 2x2 matrices are float32, as BasicSR-style kernel
    code keeps them: a kernel built from the float64 covariance differs from theirs in the 7th digit."""
    d = np.array([[sigma_x ** 2, 0], [0, sigma_y ** 2]]).astype(np.float32)
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]).astype(np.float32)
    return np.linalg.inv(np.matmul(rot, np.matmul(d, rot.T)))


def blur_kernel(family: str, size: int, sigma_x: float = 1.0, sigma_y: float = 1.0, angle: float = 0.0, beta: float = 1.0,
                omega: float = 1.0) -> np.ndarray:
    """One normalised float64 [size,size] kernel.  With q = p^T Sigma^-1 p at pixel offset p:
    Gaussian exp(-q / 2); generalized exp(-q^beta / 2); plateau 1 / (1 + q^beta); the iso families use sigma_x for both axes and no
    rotation.  ``sinc``: the circular low-pass omega J1(omega r) / (2 pi r), omega^2 / (4 pi) at the centre."""
    if family not in KERNEL_FAMILIES:
        raise ValueError(f"unknown blur-kernel family {family!r}: one of {', '.join(KERNEL_FAMILIES)}")
    if size % 2 != 1 or size < 1:
        raise ValueError(f"blur-kernel size {size} is not odd")
    gx, gy = _grid(size)
    if family == "sinc":
        r = np.hypot(gx, gy)
        r[size // 2, size // 2] = 1.0
        k = omega * bessel_j1(omega * r) / (2.0 * np.pi * r)
        k[size // 2, size // 2] = omega ** 2 / (4.0 * np.pi)
    else:
        inv = _inverse_covariance(sigma_x, sigma_x, 0.0) if family.endswith("iso") and not family.endswith("aniso") else \
            _inverse_covariance(sigma_x, sigma_y, angle)
        inv = inv.astype(np.float64)
        q = inv[0, 0] * gx * gx + (inv[0, 1] + inv[1, 0]) * gx * gy + inv[1, 1] * gy * gy
        if family.startswith("generalized"):
            k = np.exp(-0.5 * np.power(q, beta))
        elif family.startswith("plateau"):
            k = 1.0 / (np.power(q, beta) + 1.0)
        else:
            k = np.exp(-0.5 * q)
    return k / k.sum()


def kernel_from_params(family: str, size: int, p: dict) -> np.ndarray:
    """A recipe's kernel parameters -> the kernel (``beta`` is beta_gaussian or beta_plateau by family)."""
    beta = p["beta_plateau"] if family.startswith("plateau") else p["beta_gaussian"]
    return blur_kernel(family, size, p["sigma_x"], p["sigma_y"], p["angle"], beta, p["omega"])


# ---- config -> recipe -------------------------------------------------------------------------------------------------------------
def load_config(config) -> dict:
    """A dict, a ``.json`` file or a ``.yaml`` / ``.yml`` file in the reference's format (degradation_1, degradation_2)."""
    if isinstance(config, dict):
        return config
    path = os.fspath(config)
    with open(path) as f:
        if path.lower().endswith(".json"):
            return json.load(f)
        if path.lower().endswith((".yaml", ".yml")):
            import yaml
            return yaml.safe_load(f)
    raise ValueError(f"degradation config {path}: a dict, a .json or a .yaml file")


def _choice(rng, probs) -> int:
    p = np.asarray(probs, dtype=np.float64)
    return int(min(np.searchsorted(np.cumsum(p) / p.sum(), rng.random(), side="right"), len(p) - 1))


def _walk(rng, value, step, lo, hi, frames):
    """The reference's per-frame random walk: value, then value += U(-step, step) clipped to [lo, hi] for each later frame."""
    out = [float(value)]
    for _ in range(frames - 1):
        value = float(np.clip(value + rng.uniform(-step, step), lo, hi))
        out.append(value)
    return out


class Degrader:
    """``config``: the reference's degradation settings (dict, JSON or YAML path).  ``scale``: the final size is (int(H / scale),
    int(W / scale)).  ``seed``: of the host draws and of the device noise."""

    _STAGE_STEPS = (("random_blur", "RandomBlur"), ("random_resize", "RandomResize"), ("random_noise", "RandomNoise"),
                    ("random_jpeg", "RandomJPEGCompression"), ("random_mpeg", "RandomVideoCompression"))

    def __init__(self, config, scale: int = 4, seed: int = 42, video_codec: str | None = None, gop: int = DEFAULT_GOP):
        self.config = load_config(config)
        self.scale, self.seed = scale, int(seed)
        if scale <= 0:
            raise ValueError(f"scale {scale} must be positive")
        if video_codec not in VIDEO_CODECS:
            raise ValueError(f"video_codec {video_codec!r}: None (codec steps are recorded as skipped), 'sim' or 'sim-h264'")
        if int(gop) != gop or gop <= 0:
            raise ValueError(f"gop {gop!r} must be a positive integer")
        self.video_codec, self.gop = video_codec, int(gop)
        self.stages = []
        for name in ("degradation_1", "degradation_2"):
            if name not in self.config:
                raise ValueError(f"degradation config has no {name!r}")
            stage = self.config[name]
            steps = [(typ, stage[key].get("params", {})) for key, typ in self._STAGE_STEPS if key in stage]
            shuffle = None
            if "degradation_with_shuffle" in stage:
                sh = stage["degradation_with_shuffle"]
                shuffle = {"entries": [self._entry(e) for e in sh["degradations"]], "shuffle_idx": sh.get("shuffle_idx")}
            unknown = set(stage) - {k for k, _ in self._STAGE_STEPS} - {"degradation_with_shuffle"}
            if unknown:
                raise ValueError(f"{name}: unknown step(s) {sorted(unknown)}")
            for typ, params in steps:
                self._check(typ, params)
            self.stages.append((name, steps, shuffle))

    def _entry(self, e):
        if isinstance(e, (list, tuple)):
            return [self._entry(s) for s in e]
        typ, params = e.get("type"), e.get("params", {})
        self._check(typ, params)
        return (typ, params)

    @staticmethod
    def _check(typ, params):
        if typ in _CODEC_STEPS:
            if "codec" in params and len(params["codec"]) != len(params.get("codec_prob", ())):
                raise ValueError("RandomVideoCompression: codec and codec_prob differ in length")
            return
        if typ == "RandomResize":
            for opt, p in zip(params["resize_opt"], params["resize_prob"]):
                if opt.lower() == "lanczos" and p > 0:
                    raise NotImplementedError("RandomResize: resize_opt 'lanczos' is not implemented (bilinear, bicubic, area are)")
                if opt.lower() not in RESIZE_MODES and opt.lower() != "lanczos":
                    raise NotImplementedError(f"RandomResize: unknown resize_opt {opt!r}")
            if params.get("resize_step", 0) != 0 and params.get("target_size") is None:
                raise NotImplementedError("RandomResize: resize_step != 0 gives every frame its own size; a clip needs one size")
        elif typ == "RandomBlur":
            for fam in params["kernel_list"]:
                if fam not in KERNEL_FAMILIES:
                    raise NotImplementedError(f"RandomBlur: unknown kernel family {fam!r}")
        elif typ == "RandomNoise":
            for kind in params["noise_type"]:
                if kind.lower() not in ("gaussian", "poisson"):
                    raise NotImplementedError(f"RandomNoise: unknown noise_type {kind!r}")
        elif typ != "RandomJPEGCompression":
            raise NotImplementedError(f"unknown degradation type {typ!r}")

    def recipe(self, frames: int, height: int, width: int, seed: int | None = None) -> dict:
        """The recipe for a clip of ``frames`` frames of ``height`` x ``width`` (``seed`` overrides the Degrader's)."""
        seed = self.seed if seed is None else int(seed)
        rng = np.random.Generator(np.random.PCG64(seed))
        st = {"rng": rng, "F": int(frames), "h": int(height), "w": int(width), "streams": 0, "steps": [], "seed": seed, "codecs": 0}
        target = (int(height / self.scale), int(width / self.scale))
        for name, steps, shuffle in self.stages:
            for typ, params in steps:
                self._draw(st, name, typ, params)
            if shuffle is not None:
                entries = list(shuffle["entries"])
                idx = shuffle["shuffle_idx"] if shuffle["shuffle_idx"] is not None else list(range(len(entries)))
                if idx:
                    perm = rng.permutation(len(idx))
                    picked = [entries[i] for i in idx]
                    for j, i in enumerate(idx):
                        entries[i] = picked[perm[j]]
                for e in entries:
                    for typ, params in (e if isinstance(e, list) else [e]):
                        if typ == "RandomResize" and "target_size" in params:
                            params = dict(params, target_size=target)
                        self._draw(st, name + ".shuffle", typ, params)
        return {"version": RECIPE_VERSION, "seed": seed, "scale": self.scale, "frames": st["F"], "input_size": [int(height), int(width)],
                "output_size": [st["h"], st["w"]], "steps": st["steps"]}

    def _draw(self, st, stage, typ, params):
        rng, F = st["rng"], st["F"]
        if typ in _CODEC_STEPS:
            if self.video_codec is None:
                st["steps"].append({"op": "skipped", "stage": stage, "type": typ, "reason": _NO_CODEC})
                return
            own = np.random.Generator(np.random.PCG64([st["seed"], VCODEC_STREAM, st["codecs"]]))
            st["codecs"] += 1
            if own.random() > params.get("prob", 1):
                st["steps"].append({"op": "skipped", "stage": stage, "type": typ, "reason": "prob"})
                return
            codec = params["codec"][_choice(own, params["codec_prob"])]
            lo, hi = params["bitrate"]
            st["steps"].append({"op": "vcodec", "stage": stage, "codec": str(codec), "bitrate": int(own.integers(int(lo), int(hi) + 1)),
                                "gop": self.gop})
            if self.video_codec == "sim-h264":
                st["steps"][-1]["tools"] = list(VCODEC_TOOLS)
            return
        if rng.random() > params.get("prob", 1):
            st["steps"].append({"op": "skipped", "stage": stage, "type": typ, "reason": "prob"})
            return
        if typ == "RandomBlur":
            fam = params["kernel_list"][_choice(rng, params["kernel_prob"])]
            sizes = [k for k in params["kernel_size"] if k // 2 < min(st["h"], st["w"])]
            if not sizes:
                st["steps"].append({"op": "skipped", "stage": stage, "type": typ,
                                    "reason": f"no kernel size fits a {st['h']} x {st['w']} frame"})
                return
            size = int(sizes[int(rng.integers(len(sizes)))])
            omega_range = params.get("omega") or ([math.pi / 3, math.pi] if size < 13 else [math.pi / 5, math.pi])
            names = (("sigma_x", params.get("sigma_x", [0, 0])), ("sigma_y", params.get("sigma_y", [0, 0])),
                     ("angle", params.get("rotate_angle", [-math.pi, math.pi])), ("beta_gaussian", params.get("beta_gaussian", [0.5, 4])),
                     ("beta_plateau", params.get("beta_plateau", [1, 2])), ("omega", omega_range))
            step_keys = {"angle": "rotate_angle_step"}
            value = {n: float(rng.uniform(r[0], r[1])) for n, r in names}
            steps = {n: params.get(step_keys.get(n, n + "_step"), 0) for n, _ in names}
            per_frame = any(s != 0 for s in steps.values())
            plist = [dict(value)]
            for _ in range(F - 1):
                for n, r in names:
                    value[n] = float(np.clip(value[n] + rng.uniform(-steps[n], steps[n]), r[0], r[1]))
                plist.append(dict(value))
            st["steps"].append({"op": "blur", "stage": stage, "family": fam, "size": size, "params": plist if per_frame else plist[:1]})
        elif typ == "RandomResize":
            mode = params["resize_opt"][_choice(rng, params["resize_prob"])].lower()
            tsize, how, factor = params.get("target_size"), "target", None
            if tsize is None:
                how = ("up", "down", "keep")[_choice(rng, params["resize_mode_prob"])]
                lo, hi = params["resize_scale"]
                factor = rng.uniform(1, hi) if how == "up" else rng.uniform(lo, 1) if how == "down" else 1
                oh, ow = st["h"] * factor, st["w"] * factor
                least = 1
                if params.get("is_size_even", False):
                    oh, ow, least = 2 * (oh // 2), 2 * (ow // 2), 2
                tsize = (max(int(oh), least), max(int(ow), least))
            st["h"], st["w"] = int(tsize[0]), int(tsize[1])
            st["steps"].append({"op": "resize", "stage": stage, "size": [st["h"], st["w"]], "mode": mode, "how": how, "factor": None if factor is None else float(factor)})
        elif typ == "RandomNoise":
            kind = params["noise_type"][_choice(rng, params["noise_prob"])].lower()
            key, level_key = ("gaussian", "gaussian_sigma") if kind == "gaussian" else ("poisson", "poisson_scale")
            lo, hi = params[level_key]
            level = rng.uniform(lo, hi)
            gray = bool(rng.random() < params[key + "_gray_noise_prob"])
            levels = _walk(rng, level, params.get(level_key + "_step", 0), lo, hi, F)
            st["steps"].append({"op": "noise", "stage": stage, "kind": kind, "gray": gray, "level": levels, "stream_id": st["streams"]})
            st["streams"] += 1
        else:                                                    # RandomJPEGCompression
            lo, hi = params["quality"]
            step = params.get("quality_step", 0)
            q = round(rng.uniform(lo, hi))
            qs = [int(q)]
            for _ in range(F - 1):
                q = round(float(np.clip(q + rng.uniform(-step, step), lo, hi)))
                qs.append(int(q))
            st["steps"].append({"op": "jpeg", "stage": stage, "quality": qs})


def bicubic_recipe(frames: int, height: int, width: int, scale: int = 4) -> dict:
    """``--preset bicubic``: one bicubic resize to (int(H / scale), int(W / scale))."""
    size = [int(height / scale), int(width / scale)]
    return {"version": RECIPE_VERSION, "seed": 0, "scale": scale, "frames": int(frames), "input_size": [int(height), int(width)],
            "output_size": size, "steps": [{"op": "resize", "stage": "preset", "size": size, "mode": "bicubic"}]}


# ---- recipe -> device -------------------------------------------------------------------------------------------------------------
def _frame_slice(values, frame0: int, n: int, what: str):
    if len(values) < frame0 + n:
        raise ValueError(f"recipe step {what} has {len(values)} per-frame values; frames {frame0}..{frame0 + n - 1} were asked for")
    return values[frame0:frame0 + n]


def check_block(recipe: dict, frame0: int, n: int):
    """A ``vcodec`` step codes closed groups of ``gop`` frames: a block of n frames from frame0 must start on a group boundary and end on one
    or at the recipe's last frame, or the result would depend on the split.  Its ``tools``, if any, are names of VCODEC_TOOLS."""
    for i, step in enumerate(recipe["steps"]):
        if step["op"] != "vcodec":
            continue
        tools = step.get("tools", [])
        if not isinstance(tools, (list, tuple)) or any(name not in VCODEC_TOOLS for name in tools):
            raise ValueError(f"recipe step {i} (vcodec): tools {tools!r} must be a list of names from {list(VCODEC_TOOLS)}")
        gop = int(step["gop"])
        if gop <= 0:
            raise ValueError(f"recipe step {i} (vcodec): gop {gop} must be positive")
        if frame0 % gop != 0 or ((frame0 + n) % gop != 0 and frame0 + n != recipe["frames"]):
            raise ValueError(f"recipe step {i} (vcodec) codes groups of {gop} frames: frames {frame0}..{frame0 + n - 1} of {recipe['frames']} "
                             f"do not start and end on a group boundary - give --block a multiple of the group length {gop}")


def apply_recipe(frames_u8, recipe: dict, frame0: int = 0):
    """frames_u8: uint8 [F,H,W,3] (a tensor on the HIP device, or a host tensor / array that is moved there) -> uint8 [F,h,w,3] on the
    device: uint8(clip(x, 0, 255)) of the recipe's last step.  ``frame0``: the clip index of the first frame given.  A recipe with a
    ``vcodec`` step takes whole groups only (``check_block``)."""
    import torch

    from . import ops
    if recipe.get("version") != RECIPE_VERSION:
        raise ValueError(f"recipe version {recipe.get('version')!r}: this build reads version {RECIPE_VERSION}")
    t = torch.as_tensor(frames_u8)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"apply_recipe: frames must be uint8 [F,H,W,3], got {t.dtype} {tuple(t.shape)}")
    if list(t.shape[1:3]) != list(recipe["input_size"]):
        raise ValueError(f"apply_recipe: frames are {tuple(t.shape[1:3])}, the recipe was drawn for {tuple(recipe['input_size'])}")
    n = t.shape[0]
    check_block(recipe, frame0, n)
    x = t.cuda().contiguous().float()
    last_u8 = None
    for i, step in enumerate(recipe["steps"]):
        op = step["op"]
        if op == "skipped":
            continue
        last_u8 = None
        if op == "blur":
            plist = step["params"]
            if len(plist) == 1:
                k = kernel_from_params(step["family"], step["size"], plist[0])
            else:
                k = np.stack([kernel_from_params(step["family"], step["size"], p) for p in _frame_slice(plist, frame0, n, f"{i} (blur)")])
            x = ops.blur2d(x, torch.from_numpy(k.astype(np.float32)).cuda())
        elif op == "resize":
            x = ops.resize(x, step["size"][0], step["size"][1], RESIZE_MODES[step["mode"]])
        elif op == "noise":
            level = _frame_slice(step["level"], frame0, n, f"{i} (noise)")
            fn = ops.add_gaussian_noise if step["kind"] == "gaussian" else ops.add_poisson_noise
            x = fn(x, level, step["gray"], recipe["seed"], step["stream_id"], frame0)
        elif op == "jpeg":
            last_u8 = ops.jpeg_roundtrip(x, _frame_slice(step["quality"], frame0, n, f"{i} (jpeg)"))
            x = last_u8.float()
        elif op == "vcodec":
            last_u8 = ops.vcodec_roundtrip(x, step["bitrate"], step["gop"], tools=step.get("tools", ()))
            x = last_u8.float()
        else:
            raise ValueError(f"recipe step {i}: unknown op {op!r}")
    return last_u8 if last_u8 is not None else x.clamp(0, 255).to(torch.uint8)


# ---- command line -----------------------------------------------------------------------------------------------------------------
class _Clip:
    """One input clip read ``block`` frames at a time: a PNG/JPG folder, an ``.npy`` array (memory-mapped) or a ``.y4m`` file."""

    def __init__(self, path, yuv_matrix, yuv_range):
        self.path, self._rd, self._pos = path, None, 0
        if os.path.isdir(path):
            from PIL import Image
            self._names = sorted(n for n in os.listdir(path) if n.lower().endswith((".png", ".jpg", ".jpeg")))
            if not self._names:
                raise ValueError(f"no frames in {path}")
            with Image.open(os.path.join(path, self._names[0])) as im:
                self.width, self.height = im.size
            self.frames, self.kind = len(self._names), "png"
        elif path.lower().endswith(".npy"):
            self._arr = np.load(path, mmap_mode="r")
            if self._arr.dtype != np.uint8 or self._arr.ndim != 4 or self._arr.shape[3] != 3:
                raise ValueError(f"expected uint8 [F,H,W,3], got {self._arr.dtype} {self._arr.shape}")
            self.frames, self.height, self.width = self._arr.shape[:3]
            self.kind = "npy"
        elif path.lower().endswith(".y4m"):
            from . import y4m, yuv
            f = open(path, "rb")
            self._rd = y4m.Y4MReader(f)
            self._file = f
            self._fmt = yuv.format_of_reader(self._rd, yuv_matrix, yuv_range)
            self.height, self.width = self._rd.height, self._rd.width
            # a recipe needs the frame count up front: plain "FRAME\n" markers are assumed and the count is checked at the end
            self.frames = (os.path.getsize(path) - f.tell()) // (self._rd.frame_bytes + 6)
            self.kind = "y4m"
        else:
            raise ValueError(f"unsupported input {path}: a PNG folder, an .npy array or a .y4m file")

    def read(self, n: int):
        """Up to n frames, uint8 [k,H,W,3] on the device."""
        import torch
        n = min(n, self.frames - self._pos)
        if self.kind == "png":
            from PIL import Image
            arr = np.stack([np.asarray(Image.open(os.path.join(self.path, m)).convert("RGB")) for m in self._names[self._pos:self._pos + n]])
            out = torch.from_numpy(arr).cuda()
        elif self.kind == "npy":
            out = torch.from_numpy(np.ascontiguousarray(self._arr[self._pos:self._pos + n])).cuda()
        else:
            from . import yuv
            payload = self._rd.read(n)
            if payload.shape[0] != n:
                raise ValueError(f"{self.path}: {self.frames} frames were expected from the file size, the stream ended after "
                                 f"{self._pos + payload.shape[0]} (FRAME markers with parameters?)")
            out = yuv.yuv_to_rgb(payload.cuda(), self.height, self.width, self._fmt)
        self._pos += n
        return out

    def close(self):
        if self._rd is not None:
            self._rd.close()
            self._file.close()


def degrade_clip(path, out_stem, args, recipe=None):
    """One clip -> ``out_stem`` (.npy, a PNG folder or .y4m) and ``out_stem``.recipe.json; returns the recipe."""
    from . import yuv
    clip = _Clip(path, args.yuv_matrix, args.yuv_range)
    try:
        if recipe is None:
            if args.preset == "bicubic":
                recipe = bicubic_recipe(clip.frames, clip.height, clip.width, args.scale)
            else:
                codec = None if getattr(args, "video_codec", "none") == "none" else args.video_codec
                recipe = Degrader(args.config, args.scale, args.seed, codec, getattr(args, "gop", DEFAULT_GOP)).recipe(
                    clip.frames, clip.height, clip.width)
        elif recipe["frames"] < clip.frames or list(recipe["input_size"]) != [clip.height, clip.width]:
            raise ValueError(f"{path}: {clip.frames} frames of {clip.height} x {clip.width}, the recipe is for {recipe['frames']} of "
                             f"{recipe['input_size'][0]} x {recipe['input_size'][1]}")
        for f0 in range(0, clip.frames, args.block):                  # before anything is read or written
            check_block(recipe, f0, min(args.block, clip.frames - f0))
        oh, ow = recipe["output_size"]
        writer = mm = None
        if args.y4m_save:
            from . import y4m
            chroma = yuv.save_format_to_chroma(args.save_format)
            fmt = yuv.YuvFormat(chroma, args.yuv_matrix, args.yuv_range or "limited")
            writer = y4m.Y4MWriter(out_stem + ".y4m", ow, oh, args.fps, chroma, args.yuv_range == "full")
        elif args.png_save:
            from PIL import Image
            os.makedirs(out_stem, exist_ok=True)
        else:
            mm = np.lib.format.open_memmap(out_stem + ".npy", mode="w+", dtype=np.uint8, shape=(clip.frames, oh, ow, 3))
        try:
            for f0 in range(0, clip.frames, args.block):
                lq = apply_recipe(clip.read(args.block), recipe, f0)
                if writer is not None:
                    writer.write(yuv.rgb_to_yuv(lq, fmt).cpu())
                elif mm is not None:
                    mm[f0:f0 + lq.shape[0]] = lq.cpu().numpy()
                elif getattr(args, "png_encoder", "pil") == "gpu":
                    from . import png
                    png.save_frames(lq, out_stem, names=[f"{f0 + i:03d}.png" for i in range(lq.shape[0])])
                else:
                    for i, fr in enumerate(lq.cpu().numpy()):
                        Image.fromarray(fr).save(os.path.join(out_stem, f"{f0 + i:03d}.png"))
        finally:
            if writer is not None:
                writer.close()
            if mm is not None:
                mm.flush()
    finally:
        clip.close()
    with open(out_stem + ".recipe.json", "w") as f:
        json.dump(recipe, f)
    return recipe


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="Degrade ground-truth clips into low-quality ones on the GPU (dove_amd)")
    ap.add_argument("--input_dir", type=str, required=True, help="PNG folders, .npy arrays (uint8 [F,H,W,3]) and .y4m files")
    ap.add_argument("--output_path", type=str, default="./results")
    ap.add_argument("--config", type=str, default=None, help="degradation settings in the reference's format (.yaml / .json)")
    ap.add_argument("--preset", type=str, default=None, choices=("bicubic",), help="'bicubic': a plain bicubic 1/scale resize, no config")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--recipe_in", type=str, default=None, help="replay this recipe (.json) instead of drawing one")
    ap.add_argument("--png_save", action="store_true")
    ap.add_argument("--png_encoder", type=str, default="pil", choices=("pil", "gpu"),
                    help="who writes the --png_save files: PIL on the host, or the GPU encoder (dove_amd.png)")
    ap.add_argument("--y4m_save", action="store_true")
    ap.add_argument("--block", type=int, default=16, help="frames read, processed and written at a time")
    ap.add_argument("--video_codec", type=str, default="none", choices=("none", "sim", "sim-h264"),
                    help="'sim': run the config's video-compression steps as the GPU codec round trip (ops.vcodec_roundtrip); "
                         "'sim-h264': the same draws with the H.264 tool set (intra prediction, quarter-sample motion, deblocking); "
                         "'none': record them as skipped")
    ap.add_argument("--gop", type=int, default=DEFAULT_GOP, help="frames per closed group of --video_codec sim (--block must be a multiple)")
    ap.add_argument("--fps", type=int, default=16)
    ap.add_argument("--save_format", type=str, default="yuv444p")
    ap.add_argument("--yuv_matrix", type=str, default="bt601", choices=("bt601", "bt709"))
    ap.add_argument("--yuv_range", type=str, default=None, choices=("limited", "full"))
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.y4m_save and args.png_save:
        raise ValueError("--y4m_save and --png_save: choose one output form")
    if sum(x is not None for x in (args.config, args.preset, args.recipe_in)) != 1:
        raise ValueError("give exactly one of --config, --preset and --recipe_in")
    if args.block <= 0:
        raise ValueError(f"--block {args.block} must be positive")
    if args.gop <= 0:
        raise ValueError(f"--gop {args.gop} must be positive")
    if args.video_codec != "none" and args.block % args.gop != 0:
        raise ValueError(f"--block {args.block} must be a multiple of --gop {args.gop}: a group of frames is coded as a whole")
    recipe = None
    if args.recipe_in:
        with open(args.recipe_in) as f:
            recipe = json.load(f)
    names = sorted(n for n in os.listdir(args.input_dir)
                   if n.lower().endswith((".npy", ".y4m")) or os.path.isdir(os.path.join(args.input_dir, n)))
    if not names:
        raise ValueError(f"No clips (.npy, .y4m or PNG folders) found in {args.input_dir}")
    os.makedirs(args.output_path, exist_ok=True)
    for name in names:
        stem = name[:-4] if name.lower().endswith((".npy", ".y4m")) else name
        r = degrade_clip(os.path.join(args.input_dir, name), os.path.join(args.output_path, stem), args, recipe)
        done = [s["op"] for s in r["steps"] if s["op"] != "skipped"]
        print(f"[{name}] {r['frames']} frames {r['input_size'][0]}x{r['input_size'][1]} -> {r['output_size'][0]}x{r['output_size'][1]} | "
              f"steps: {', '.join(done) or 'none'}")
    print("All clips degraded.")


if __name__ == "__main__":
    main()
