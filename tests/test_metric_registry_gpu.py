"""Every metric of dove_amd.metrics.REGISTRY through the one metric object and the one group walk, on the device: the object gives the
bits of the module's own function, and a grouped metric gives the same bits whatever the grouping.

Input: three uint8 frames of 192 x 192 (the noise levels of tests/test_percep_gpu.py's ``_images``): NIQE has four blocks per frame, every
minimum side (96 for NIQE, 31 for CLIP-IQA and AlexNet, 16 for VGG16) is passed, and three frames leave a ragged last group at group=2."""
import gc

import pytest
import torch

import test_clipiqa_cpu as TC
import test_musiq_cpu as TM
from dove_amd import clipiqa, musiq, niqe, percep
from dove_amd import metrics as M
from test_percep_gpu import _images

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}
MODULE = {"lpips": percep, "lpips-vgg": percep, "dists": percep, "clipiqa": clipiqa, "musiq": musiq}      # the metrics walked in groups
DIRECT = {                                                      # the module's own function, on device tensors
    "psnr": lambda W, p, r: M.fr_metrics(p, r, ssim=False, layout="nchw")[0],
    "ssim": lambda W, p, r: M.fr_metrics(p, r, psnr=False, layout="nchw")[1],
    "lpips": lambda W, p, r, **kw: percep.lpips(W, p, r, **kw),
    "lpips-vgg": lambda W, p, r, **kw: percep.lpips(W, p, r, **kw),
    "dists": lambda W, p, r, **kw: percep.dists(W, p, r, **kw),
    "niqe": lambda W, p, r: niqe.niqe(W, p),
    "clipiqa": lambda W, p, r, **kw: clipiqa.clipiqa(W, p, **kw),
    "musiq": lambda W, p, r, **kw: musiq.musiq(W, p, **kw),
}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory():
    """As tests/test_musiq_gpu.py: the weights' device copies and the token tables are dropped and the blocks handed back, so that the
    streaming tool's peak-memory test sees nothing of this module."""
    live = torch.cuda.memory_allocated()
    yield
    _CACHE.clear()
    for geo in musiq._GEOMETRY.values():
        geo["device"].clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() <= live, "this module left tensors on the device"


def frames():
    """(pred, ref) uint8 [3,3,192,192] on the host."""
    if "frames" not in _CACHE:
        _CACHE["frames"] = tuple((t * 255).round().to(torch.uint8) for t in _images(192, 192))
    return _CACHE["frames"]


def weights(name):
    if name not in _CACHE:
        if name in ("lpips", "lpips-vgg"):
            net = "vgg" if name == "lpips-vgg" else "alex"
            _CACHE[name] = percep.LpipsWeights.from_state_dicts(*percep.random_lpips_state(21, net), net)
        elif name == "dists":
            _CACHE[name] = percep.DistsWeights.from_state_dicts(*percep.random_dists_state(21))
        elif name == "niqe":                                    # fitted on 45 blocks of other images: a full-rank model, distinct scores
            pristine = (_images(288, 480)[0] * 255).round().to(torch.uint8)
            _CACHE[name] = niqe.fit([pristine], sharpness=0.0)
        elif name == "clipiqa":
            _CACHE[name] = clipiqa.ClipIqaWeights.from_state_dict(*TC.state())
        elif name == "musiq":
            _CACHE[name] = musiq.MusiqWeights.from_state_dict(TM.state())
        else:
            _CACHE[name] = None
    return _CACHE[name]


def test_the_cases_are_the_registry():
    assert set(DIRECT) == set(M.REGISTRY) and set(MODULE) == set(M.NETWORK_METRICS + M.NR_METRICS) - {"niqe"}


@pytest.mark.parametrize("name", list(DIRECT))
def test_metric_object_and_group_walk(name, monkeypatch):
    pred, ref = frames()
    W, spec = weights(name), M.REGISTRY[name]                   # made before the stack is shortened: the state dict is shared with other modules
    monkeypatch.setattr(musiq, "NUM_LAYERS", 2)                 # as tests/test_musiq_gpu.py: two blocks walk every kernel of the stack
    metric = (M.create_metric(name) if W is None else M.create_metric(name, weights=W)).to(DEV)
    assert metric.metric_name == name and metric.lower_better is spec.lower_better and metric.device.type == "cuda"
    got = metric(pred) if spec.kind == M.NR else metric(pred, ref)               # host frames: the object uploads them
    want = DIRECT[name](W, pred.to(DEV), ref.to(DEV))
    print(f"{name}: {got.tolist()}")
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (3,)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert len(set(got.tolist())) == 3                          # three noise levels, three values: a swapped frame would show
    assert torch.equal(metric(pred[1], ref[1]), got[1:2])       # one [C,H,W] image; a no-reference metric ignores ``ref``
    if name in MODULE:
        counters = MODULE[name].COUNTERS
        for group, walked in ((1, 3), (2, 2)):
            before = counters["groups"]
            assert torch.equal(DIRECT[name](W, pred.to(DEV), ref.to(DEV), group=group), got), group
            assert counters["groups"] == before + walked


def test_weights_to_names_the_current_device_and_frees_with_its_owner():
    """dove_amd.netweights.Weights.to on the hand-made container of tests/test_netweights_cpu.py: ``cuda`` is the current index, one
    copy per device, every leaf there, and the copy's memory goes when the container goes."""
    import test_netweights_cpu as TN
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    c = TN.container(256)
    here = torch.device("cuda", torch.cuda.current_device())
    moved = c.to("cuda")
    assert moved is c.to(here) and moved is c.to(f"cuda:{here.index}") and moved.to("cuda") is moved and len(c._copies) == 1
    TN.check_copy(c, moved, here)
    for k, t in TN.tensor_leaves(moved).items():
        assert torch.equal(t.cpu(), TN.tensor_leaves(c)[k]), k
    assert torch.cuda.memory_allocated() > live
    del moved, t, c
    gc.collect()
    assert torch.cuda.memory_allocated() == live
