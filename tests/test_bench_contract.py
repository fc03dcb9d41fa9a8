"""Guard the bench.py driver contract: one JSON line on stdout with the
agreed keys, runnable with no flags on CPU, all three modes intact."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = [
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
]


def _run(*args):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *args],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    return json.loads(line)


def test_train_contract_cpu():
    d = _run("--steps", "2", "--warmup", "1", "--batch", "256")
    for k in REQUIRED:
        assert k in d, k
    assert d["metric"] == "samples_per_sec"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 256
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["model"].startswith("mnist_mlp")


def _load_dump(d):
    import numpy as np

    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_and_full_cpu(tmp_path):
    """--dump-outputs writes the last timed step's loss plus loss, gradients
    and weights of one untimed step of the rewound timed trainer (``ref.*``)
    as float32/float64 .npy; the same arguments reproduce all of it exactly on
    CPU.  --full is accepted and leaves the result line's meaning unchanged."""
    import numpy as np

    dumps = []
    for name, extra in (("a", ()), ("b", ("--full",))):
        d = str(tmp_path / name)
        out = _run("--device", "cpu", "--steps", "3", "--warmup", "1", "--batch", "256",
                   "--dump-outputs", d, *extra)
        assert out["metric"] == "samples_per_sec" and out["steps"] == 3
        assert out["unit"] == "samples/s" and out["higher_is_better"] is True
        assert out["ms_per_step"] > 0
        dumps.append(_load_dump(d))
    a, b = dumps
    grads = {k[len("ref.grad."):] for k in a if k.startswith("ref.grad.")}
    states = {k[len("ref.state."):] for k in a if k.startswith("ref.state.")}
    assert grads == states and len(states) == 6
    assert set(a) == {"loss", "ref.loss"} | {"ref.grad." + k for k in grads} | {"ref.state." + k for k in states}
    assert all(np.abs(a["ref.grad." + k]).max() > 0 for k in grads)
    assert sorted(a) == sorted(b)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    # 784*256 + 256 + 256*256 + 256 + 256*10 + 10 weights, unsampled
    assert sum(a["ref.state." + k].size for k in states) == 269322
    # loss is the 4th training step's, ref.loss the first step's: training moved it
    assert a["loss"][0] < a["ref.loss"][0]


def test_dump_outputs_match_independent_step_cpu(tmp_path):
    """With --warmup 0 --steps 1 the last timed step IS the first step from
    the seeded state, so the dumped timed loss must equal ref.loss, and both
    must equal a one-step recomputation done here with a trainer of our own
    (same seeds as bench.py: 1234 for the weights, 1234 + rank for the data)."""
    import numpy as np
    import torch
    import torch.nn as nn

    from sparktorch_amd.models.mnist import MnistMLP
    from sparktorch_amd.parallel.sync import SyncTrainer

    d = str(tmp_path / "one")
    _run("--device", "cpu", "--steps", "1", "--warmup", "0", "--batch", "256", "--dump-outputs", d)
    got = _load_dump(d)

    torch.manual_seed(1234)
    model = MnistMLP()
    trainer = SyncTrainer(model, nn.CrossEntropyLoss(), torch.optim.Adam(model.parameters(), lr=1e-3),
                          device="cpu", world_size=1)
    torch.manual_seed(1234)
    x = torch.randn(256, 784)
    y = torch.randint(0, 10, (256,))
    loss = trainer.train_step(x, y)

    assert got["loss"][0] == got["ref.loss"][0] == loss
    for k, p in trainer.model.named_parameters():
        assert np.array_equal(got["ref.grad." + k], p.grad.numpy()), k
    for k, v in trainer.model.state_dict().items():
        assert np.array_equal(got["ref.state." + k], v.detach().numpy()), k


def test_dump_outputs_sampling_over_budget(tmp_path, monkeypatch):
    """Over the byte budget every array is cut to the same fraction at fixed,
    seeded positions: two dumps keep the same elements, in order, and the
    total stays within the budget; small dumps are written whole."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    budget = 40_000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    big = torch.arange(50_000, dtype=torch.float32).reshape(100, 500)  # value == flat position
    ints = torch.arange(7_000, dtype=torch.int64)
    one = torch.tensor([3.5], dtype=torch.float64)
    tensors = {"big": big, "ints": ints, "one": one}
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), tensors)
    a, b = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))
    assert set(a) == set(tensors)
    on_disk = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert on_disk <= budget
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["big"].dtype == np.float32 and a["ints"].dtype == np.float64
    total = 50_000 * 4 + 7_000 * 8 + 8
    for k, n in (("big", 50_000), ("ints", 7_000)):
        v = a[k]
        assert v.ndim == 1 and 0 < v.size < n
        assert abs(v.size / n - budget / total) < 0.02, (k, v.size)  # same fraction of each
        assert np.all(np.diff(v) > 0) and v[0] >= 0 and v[-1] < n  # distinct positions, in order
        assert np.all(v == np.round(v))
    assert a["one"].shape == (1,) and a["one"][0] == 3.5

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 1000 * 1000)
    bench.dump_outputs(str(tmp_path / "whole"), tensors)
    w = _load_dump(str(tmp_path / "whole"))
    assert w["big"].shape == (100, 500) and np.array_equal(w["big"], big.numpy())


def test_infer_contract_cpu():
    d = _run("--mode", "infer", "--steps", "2", "--warmup", "1", "--batch", "128")
    assert d["metric"] == "inference_samples_per_sec"
    assert d["value"] > 0


def test_time_to_loss_contract_cpu():
    d = _run("--mode", "time_to_loss", "--steps", "2", "--warmup", "1",
             "--batch", "256", "--target-loss", "5.0", "--max-steps", "3")
    assert d["metric"] == "time_to_loss_s"
    assert d["higher_is_better"] is False
    assert d["scaling"] == "strong"
    assert "reached" in d["config"]


def test_graft_entry_contract():
    """__graft_entry__ must expose build() and smoke() (driver contract);
    build() must be idempotent-cheap when the extension is current."""
    sys.path.insert(0, REPO)
    try:
        import __graft_entry__ as g
    finally:
        sys.path.pop(0)
    assert callable(g.build) and callable(g.smoke)
    g.build()  # no-op rebuild when sources unchanged; must not raise on CPU
    from sparktorch_amd import ops
    assert ops.available()


def test_fit_contract_cpu():
    """--mode fit: estimator-path metric with ingest inside the timed region."""
    out = _run("--mode", "fit", "--steps", "2", "--warmup", "1", "--batch", "512")
    for k in REQUIRED:
        assert k in out, k
    assert out["metric"] == "fit_samples_per_sec"
    assert out["higher_is_better"] is True
    assert out["config"]["ingest_included_in_timed_region"] is True
    assert out["config"]["ingest_ms"] > 0
    assert out["value"] > 0
