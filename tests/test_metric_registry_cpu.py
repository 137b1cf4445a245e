"""dove_amd.metrics.REGISTRY: every metric is declared once, and the lists, refusals, loaders, help texts and command-line checks are read
from it.  No GPU and no library: a dummy no-reference metric put into the registry is accepted everywhere with nothing else patched."""
import os
import subprocess
import sys

import pytest
import torch

from dove_amd import cli
from dove_amd import eval_metrics as E
from dove_amd import iqa
from dove_amd import metrics as M

ORDER = ("psnr", "ssim", "lpips", "lpips-vgg", "dists", "niqe", "clipiqa", "musiq")


def test_registry_order_and_derived_lists():
    assert tuple(M.REGISTRY) == ORDER == M.metric_names()
    assert M.FR_METRICS == ("psnr", "ssim")
    assert M.NETWORK_METRICS == ("lpips", "lpips-vgg", "dists")
    assert M.NR_METRICS == ("niqe", "clipiqa", "musiq")
    assert M.list_models() == M.list_models("FR") == ["psnr", "ssim"] and M.list_models("NR") == []
    assert M.name_list(["a"]) == "a" and M.name_list(["a", "b"]) == "a and b" and M.name_list(("a", "b", "c")) == "a, b and c"


def test_every_spec_is_filled():
    lower = {"psnr": False, "ssim": False, "lpips": True, "lpips-vgg": True, "dists": True, "niqe": True, "clipiqa": False, "musiq": False}
    for name, spec in M.REGISTRY.items():
        assert spec.name == name and spec.kind in (M.FR, M.NETWORK, M.NR) and spec.lower_better is lower[name] and callable(spec.build)
        if spec.kind == M.FR:
            assert spec.load is None and spec.probe is None and spec.patterns == ()
        else:
            assert callable(spec.load) and spec.patterns and all("*" in p for p in spec.patterns) and spec.section.startswith("1")
    assert [n for n, s in M.REGISTRY.items() if s.probe is not None] == ["clipiqa", "musiq"]


def test_patterns_are_the_modules_own():
    """The registry repeats the file patterns for the help texts and the probes, so that it can be read without the modules: they must be
    the ones the loaders search for."""
    from dove_amd import clipiqa, musiq, niqe, percep
    P = percep.FILE_PATTERNS
    assert M.REGISTRY["lpips"].patterns == (P["alex"], P["lpips-alex"])
    assert M.REGISTRY["lpips-vgg"].patterns == (P["vgg"], P["lpips-vgg"])
    assert M.REGISTRY["dists"].patterns == (P["vgg"], P["dists"])
    assert M.REGISTRY["niqe"].patterns == niqe.FILE_PATTERNS
    C = clipiqa.FILE_PATTERNS
    assert M.REGISTRY["clipiqa"].patterns == C["model"] + C["text"] + C["vocab"]
    assert M.REGISTRY["musiq"].patterns == (musiq.FILE_PATTERN,)
    assert percep.ACTIVATION_BUDGET == clipiqa.ACTIVATION_BUDGET == musiq.ACTIVATION_BUDGET == iqa.ACTIVATION_BUDGET == 4 << 30


def test_probes_look_for_the_main_file(tmp_path):
    assert M.REGISTRY["clipiqa"].probe(str(tmp_path)) is False and M.REGISTRY["musiq"].probe(str(tmp_path)) is False
    assert M.REGISTRY["musiq"].probe("") is False
    (tmp_path / "clipiqa_text.npz").touch()
    assert M.REGISTRY["clipiqa"].probe(str(tmp_path)) is False          # the text features alone are not the checkpoint
    (tmp_path / "RN50.pth").touch()
    (tmp_path / "musiq_koniq.pth").touch()
    assert M.REGISTRY["clipiqa"].probe(str(tmp_path)) is True and M.REGISTRY["musiq"].probe(str(tmp_path)) is True
    assert iqa.find_first(str(tmp_path), ("RN50*.pt", "RN50*.pth")).endswith("RN50.pth") and iqa.find_first(str(tmp_path), "x*") is None
    with pytest.raises(FileNotFoundError, match=r"no file matching a\*\.b or c\*\.d in "):
        iqa.find_file(str(tmp_path), ("a*.b", "c*.d"))


@pytest.mark.parametrize("name", ORDER)
def test_wrong_weights_are_refused_as_before(name):
    # psnr / ssim take no weights; every other metric names the class it wants
    with pytest.raises(NotImplementedError if name in ("psnr", "ssim") else TypeError):
        M.create_metric(name, weights=object())
    with pytest.raises(NotImplementedError, match="default options"):
        M.create_metric(name, **({} if name in ("psnr", "ssim") else {"weights": object()}), crop_border=4)
    if name not in ("psnr", "ssim"):
        with pytest.raises(NotImplementedError, match="pyiqa"):
            M.create_metric(name)


def test_importing_the_registry_imports_no_metric_module():
    code = ("import sys; import dove_amd.metrics as M; M.create_metric('psnr'); M.weights_help(); "
            "print(sorted(m for m in sys.modules if m in ('dove_amd.percep', 'dove_amd.niqe', 'dove_amd.clipiqa', 'dove_amd.musiq')))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.stdout.strip() == "[]"


def test_a_metric_is_declared_in_one_place(tmp_path, monkeypatch, capsys):
    """A dummy no-reference metric: one MetricSpec with stub load, probe and score functions, and nothing else patched."""
    calls = []

    def load(directory):
        calls.append(("load", directory))
        return {"offset": 0.5}

    def probe(directory):
        calls.append(("probe", directory))
        return directory.endswith("good")

    def score(weights, pred):
        calls.append(("score", tuple(pred.shape)))
        return pred.double().mean(dim=(1, 2, 3)) + weights["offset"]

    spec = M.MetricSpec("dummy", M.NR, False, lambda weights: iqa.GpuMetric("dummy", False, False, score, weights, dict), load, probe,
                        patterns=("dummy*.bin",), section="9z")
    monkeypatch.setitem(M.REGISTRY, "dummy", spec)
    good, bad = str(tmp_path / "good"), str(tmp_path / "bad")

    # create_metric and the generated messages
    with pytest.raises(NotImplementedError, match=r"pyiqa metrics \(lpips, lpips-vgg, dists, niqe, clipiqa, musiq, dummy, \.\.\.\)"):
        M.create_metric("dummy")
    with pytest.raises(NotImplementedError, match="weights belong to lpips, lpips-vgg, dists, niqe, clipiqa, musiq, dummy"):
        M.create_metric("psnr", weights={})
    with pytest.raises(TypeError, match=r"create_metric\('dummy'\): weights must be a builtins.dict"):
        M.create_metric("dummy", weights=object())
    m = M.create_metric(" Dummy ", weights={"offset": 0.5})
    assert isinstance(m, iqa.GpuMetric) and m.metric_name == "dummy" and m.lower_better is False
    assert "dummy: dummy*.bin (INTEGRATION.md 9z)" in M.weights_help()

    # eval_metrics: the loader, the models and the help texts
    assert E.load_weights(["psnr", "dummy"], good) == {"dummy": {"offset": 0.5}} and calls == [("load", good)]
    assert E.load_weights(["psnr", "dummy"], "") == {}
    models = E.init_models(["psnr", "dummy"], "cpu", {"dummy": {"offset": 0.5}})
    assert list(models) == ["psnr", "dummy"] and models["dummy"].weights == {"offset": 0.5}
    assert E.init_models(["dummy"], "cpu") == {} and "pyiqa" in capsys.readouterr().out
    for main in (E.main, cli.main):
        with pytest.raises(SystemExit):
            main(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert "dummy: dummy*.bin (INTEGRATION.md 9z)" in text and "niqe,clipiqa,musiq,dummy" in text

    # the command line's validation
    del calls[:]
    cli.check_eval_metrics(["dummy"], good, has_gt=False)                  # no-reference: no ground truth needed
    assert calls == [("probe", good)]
    with pytest.raises(NotImplementedError, match=r"holds none of the files of dummy \(dummy\*\.bin\).*INTEGRATION.md 9z"):
        cli.check_eval_metrics(["dummy"], bad, has_gt=False)
    with pytest.raises(NotImplementedError, match=r"only 'psnr' and 'ssim' are computed here.*adds lpips, lpips-vgg, dists, niqe, clipiqa, musiq and dummy\)"):
        cli.check_eval_metrics(["dummy"], "", has_gt=False)
    with pytest.raises(NotImplementedError, match="'musiq' and 'dummy' are computed here"):
        cli.check_eval_metrics(["dummy", "maniqa"], good, has_gt=False)
    with pytest.raises(ValueError, match="--eval_metrics ssim,dummy needs --gt_dir"):
        cli.check_eval_metrics(["ssim", "dummy"], good, has_gt=False)
    cli.check_eval_metrics(["ssim", "dummy"], good, has_gt=True)

    # the per-clip function, with the device moves stubbed out
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    del calls[:]
    frames = torch.full((3, 8, 10, 3), 51, dtype=torch.uint8)
    vals = M.nr_clip_metrics(frames, ["dummy"], {"dummy": {"offset": 0.5}})
    assert vals == {"dummy": 51.5} and calls == [("score", (3, 3, 8, 10))]
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.nr_clip_metrics(frames, ["dummy"], {})
    assert m(frames[0].permute(2, 0, 1), frames[0]).tolist() == [51.5]      # one [C,H,W] image; a no-reference metric ignores ``ref``
