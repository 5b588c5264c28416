"""bench.py's host side: the options of a plain run and what --dump-outputs writes (float32 .npy files, at most
bench.DUMP_BYTES in all, a larger output cut down to the same seeded sample in every run)."""
import os

import numpy as np
import torch

import bench


def _step():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4))
    model[2].bias.requires_grad_(False)  # a parameter without a gradient: no file
    total = model(torch.randn(8, 16)).square().mean()
    total.backward()
    return model, total.detach(), {"loss_a": total.detach() * 2, "loss_b": torch.tensor(0.5, dtype=torch.float64)}


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    opt = bench.parse()
    assert opt.steps == 7 and opt.warmup == 2 and not opt.full and opt.dump_outputs is None
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    opt = bench.parse()
    assert opt.full and opt.dump_outputs == "out"


def test_dump_writes_losses_and_the_gradient_as_float32(tmp_path):
    model, total, losses = _step()
    bench.dump_outputs(str(tmp_path), total, losses, model)
    names = sorted(os.listdir(tmp_path))
    assert names == ["grad.npy", "loss.loss_a.npy", "loss.loss_b.npy", "loss.npy"]
    for n in names:
        assert np.load(tmp_path / n).dtype == np.float32, n
    assert np.load(tmp_path / "loss.npy") == np.float32(total)
    # every parameter's gradient in named_parameters() order, zeros where there is none
    want = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in model.parameters()])
    assert np.array_equal(np.load(tmp_path / "grad.npy"), want.numpy())


def test_dump_of_a_larger_output_is_the_same_seeded_sample_within_the_cap(tmp_path, monkeypatch):
    model, total, losses = _step()
    monkeypatch.setattr(bench, "DUMP_BYTES", 2048)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), total, losses, model)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 2048
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    g = np.load(tmp_path / "a" / "grad.npy")
    full = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in model.parameters()])
    assert 0 < g.size < full.numel() and np.isin(g, full.numpy()).all()
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(total)  # a scalar stays whole
