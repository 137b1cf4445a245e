"""Generate tests/golden/colorfix_golden.npz by IMPORTING the reference's own finetune/scripts/color_fix_util.py.

Runs only where the reference tree is present.  The util imports torchvision (absent here) for ``ToTensor`` / ``ToPILImage``, which only
its PIL wrappers use; stub modules stand in, and the two core functions (``wavelet_reconstruction``,
``adaptive_instance_normalization``) run on torch alone.  The fixture holds data only: per case the two float32 inputs (values already
rounded to bfloat16, from tests/colorfix_ref.make_pair) and the reference's float32 outputs of both functions.  Before writing, the
generator asserts what the tests rely on: the reference's own fp32 result stays within 1e-6 of the float64 restatement, and truncated to
uint8 it stays inside the uint8 gate (no pixel off by more than one level, at most 1e-3 of them off at all)."""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DOVE_REFERENCE_ROOT", "/root/reference") + "/finetune/scripts/color_fix_util.py"
OUT = os.path.join(ROOT, "tests", "golden", "colorfix_golden.npz")
CASES = {"a": (2, 45, 37), "b": (1, 9, 12), "c": (1, 72, 104)}      # all below the 63-pixel support; 9x12 keeps every level on the clamp


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference():
    class _Any:
        def __init__(self, *a, **k):
            pass

    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms", ToTensor=_Any, ToPILImage=_Any)
    spec = importlib.util.spec_from_file_location("ref_color_fix_util", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import colorfix_ref as R

    ref = load_reference()
    rng = np.random.default_rng(20261016)
    data = {}
    for key, (n, h, w) in CASES.items():
        content, style = R.make_pair(rng, n, h, w)
        c, s = torch.from_numpy(content), torch.from_numpy(style)
        outs = {"wavelet": ref.wavelet_reconstruction(c, s).numpy(), "adain": ref.adaptive_instance_normalization(c, s).numpy()}
        data[f"{key}_content"], data[f"{key}_style"] = content, style
        for mode, got in outs.items():
            assert got.dtype == np.float32 and got.shape == content.shape
            want = R.fix(content, style, mode)
            e_ref = float(np.abs(got.astype(np.float64) - want).max())
            worst, share = R.u8_gate(R.to_u8(got.astype(np.float64)), R.to_u8(want))
            print(f"{key} {n}x3x{h}x{w} {mode}: e_ref {e_ref:.3e}, range {got.min():.3f} .. {got.max():.3f}, uint8 worst {worst} "
                  f"share {share:.2e}")
            assert e_ref < 1e-6 and worst <= 1 and share <= 1e-3
            data[f"{key}_{mode}"] = got
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
