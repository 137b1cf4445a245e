#!/usr/bin/env python3
"""sha256 digests of the metric networks' rule-generated state dicts and of the weights objects packed from them.

    tools/state_digests.py            writes tests/golden/state_digests.json

Run it at the revision whose draws and packing are to be kept; tests/test_netweights_cpu.py recomputes the digests and compares.  Only
public names are used (the ``random_*`` generators, ``from_state_dict(s)`` and the public dataclass fields of the weights objects), so
the same file runs before and after a change to how these are written.  A digest covers (path, dtype, shape, bytes) of every tensor or
array in sorted-path order, and the repr of every other leaf (floats, strings, configs); ``device`` is not a leaf.
"""
import dataclasses, hashlib, json, os, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leaves(obj, path=""):
    """(path, leaf) of everything reachable through dicts, lists, tuples and the public fields of dataclass instances."""
    if dataclasses.is_dataclass(obj) and not isinstance(obj, type) and not getattr(obj, "__dataclass_params__").frozen:
        obj = {f.name: getattr(obj, f.name) for f in dataclasses.fields(obj) if not f.name.startswith("_") and f.name != "device"}
    if isinstance(obj, dict):
        for k in obj:
            yield from leaves(obj[k], f"{path}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from leaves(v, f"{path}/{i}")
    else:
        yield path, obj


def digest(obj) -> str:
    h = hashlib.sha256()
    for path, v in sorted(leaves(obj), key=lambda pv: pv[0]):
        h.update(path.encode() + b"\0")
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().contiguous()
            h.update(f"{v.dtype}{tuple(v.shape)}".encode() + b"\0")
            h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes() if v.numel() else b"")
        elif isinstance(v, np.ndarray):
            h.update(f"numpy.{v.dtype}{tuple(v.shape)}".encode() + b"\0" + np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
        h.update(b"\1")
    return h.hexdigest()


def cases():
    """name -> (state, weights) thunks, in the order of the file."""
    from dove_amd import clipiqa, fastvqa, flow, musiq, percep
    out = {}
    for net in ("alex", "vgg"):
        out[f"lpips-{net}"] = (lambda net=net: percep.random_lpips_state(1, net),
                               lambda s, net=net: percep.LpipsWeights.from_state_dicts(s[0], s[1], net))
    out["dists"] = (lambda: percep.random_dists_state(1), lambda s: percep.DistsWeights.from_state_dicts(*s))
    out["raft"] = (lambda: flow.random_raft_state(7), flow.RaftWeights.from_state_dict)
    out["clipiqa"] = (lambda: clipiqa.random_clipiqa_state(31), lambda s: clipiqa.ClipIqaWeights.from_state_dict(*s))
    out["musiq"] = (lambda: musiq.random_musiq_state(3), musiq.MusiqWeights.from_state_dict)
    out["musiq-10"] = (lambda: musiq.random_musiq_state(3, 10), musiq.MusiqWeights.from_state_dict)
    for name in ("FasterVQA", "FAST-VQA"):
        cfg = fastvqa.preset(name)
        out[f"fastvqa-{name}"] = (lambda cfg=cfg: fastvqa.random_state(cfg, 5), lambda s, cfg=cfg: fastvqa.VqaWeights.from_state_dict(s, cfg))
    return out


def digests() -> dict:
    out = {}
    for name, (state, weights) in cases().items():
        s = state()
        out[name] = {"state": digest(s), "weights": digest(weights(s))}
    return out


def main():
    path = os.path.join(ROOT, "tests", "golden", "state_digests.json")
    with open(path, "w") as f:
        json.dump(digests(), f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
