"""bench.py --dump-outputs: what it writes, checked on a small CPU module (no GPU needed)."""
import os

import numpy as np
import torch

import bench
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LossResult


def _stepped_net():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.BatchNorm2d(16), torch.nn.Conv2d(16, 8, 1)).train()
    y = net(torch.randn(2, 3, 12, 12))
    parts = LossResult(localization=y.mean(), objectness=y.abs().mean(), classification=(y * y).mean())
    total = 2.0 * (parts.localization + parts.classification + parts.objectness)
    total.backward()
    return net, total, parts


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_the_step_outputs_in_full(tmp_path):
    net, total, parts = _stepped_net()
    written = bench.dump_outputs(str(tmp_path), net, total, parts)
    got = _load(tmp_path)
    assert set(got) == set(written) == {"loss_total", "loss_parts", "bn_buffers", "params", "grads"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["loss_total"].tolist() == [total.item()]
    assert got["loss_parts"].tolist() == [parts.localization.item(), parts.objectness.item(), parts.classification.item()]
    np.testing.assert_array_equal(got["params"], torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy())
    np.testing.assert_array_equal(got["grads"], torch.cat([p.grad.reshape(-1) for p in net.parameters()]).numpy())
    np.testing.assert_array_equal(got["bn_buffers"], torch.cat([b.reshape(-1).double() for b in net.buffers()]).numpy())


def test_dump_samples_large_arrays_within_the_budget(tmp_path, monkeypatch):
    net, total, parts = _stepped_net()
    full = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), net, total, parts)
        runs.append(_load(d))
        assert sum(os.path.getsize(d / f) - 128 for f in os.listdir(d)) <= 4000       # .npy payload (128 B headers)
    a, b = runs
    assert set(a) == {"loss_total", "loss_parts", "bn_buffers", "params", "params_index", "grads", "grads_index"}
    idx = a["params_index"].astype(np.int64)
    assert 0 < idx.size < full.size and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["params"], full[idx])
    for name in a:                                        # the same sample in every run
        np.testing.assert_array_equal(a[name], b[name])
