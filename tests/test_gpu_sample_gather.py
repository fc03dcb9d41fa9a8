"""sample_gather (ops/csrc/sample_gather.hip): the kernel draws exactly the
rows of utils.sampling.permuted_indices and copies them bit for bit, a
captured call draws a new batch on every replay, and the trainer / estimator
minibatch paths run on it without any host draw."""

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import SparkTorch, ops, serialize_torch_obj
from sparktorch_amd.compat.local import LocalDataFrame, free_port
from sparktorch_amd.models.mnist import MnistMLP
from sparktorch_amd.ops.modules import MnistMLPFused
from sparktorch_amd.parallel.sync import SyncTrainer
from sparktorch_amd.utils.sampling import DeviceMinibatchSampler, permuted_indices

DEV = "cuda:0"
SEED = 20240607


def _bits(t):
    """Integer view for bit-exact comparison (NaN-safe, sign-of-zero-safe)."""
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _step_dev(step):
    return torch.tensor([step], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("n,k", [(5, 4), (33, 32), (1000, 100), (4099, 64), (65537, 256)])
def test_kernel_indices_equal_reference(n, k):
    ext = ops.ext()
    x = torch.arange(n, dtype=torch.float32, device=DEV).reshape(n, 1).contiguous()
    xb = torch.empty(k, 1, device=DEV)
    idx = torch.empty(k, dtype=torch.int32, device=DEV)
    for step in (0, 1, 7):
        sd = _step_dev(step)
        ext.sample_gather(x, None, xb, None, SEED, sd, idx)
        want = permuted_indices(n, k, SEED, step)
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), want), (n, k, step)
        assert np.array_equal(xb.cpu().numpy().reshape(-1).astype(np.int64), want)
        assert int(sd) == step  # the gather reads the counter, it does not advance it


def _gather_case(x, y, k, step=3):
    ext = ops.ext()
    n = x.shape[0]
    # canaries on both sides of the outputs: one allocation, outputs in the middle
    xb_all = torch.full((k + 2, x.shape[1]), 7, dtype=x.dtype, device=DEV)
    xb = xb_all[1:-1]
    yb = yb_all = None
    if y is not None:
        yb_all = torch.full((k + 2, y.shape[1]), 7, dtype=y.dtype, device=DEV)
        yb = yb_all[1:-1]
    ext.sample_gather(x, y, xb, yb, SEED, _step_dev(step), None)
    idx = torch.from_numpy(permuted_indices(n, k, SEED, step)).to(DEV)
    assert torch.equal(_bits(xb), _bits(x[idx]))
    assert (xb_all[0] == 7).all() and (xb_all[-1] == 7).all()
    if y is not None:
        assert torch.equal(_bits(yb), _bits(y[idx]))
        assert (yb_all[0] == 7).all() and (yb_all[-1] == 7).all()


@pytest.mark.parametrize("dtype,F", [(torch.bfloat16, 784), (torch.bfloat16, 10),
                                     (torch.float32, 20), (torch.bfloat16, 136)])
@pytest.mark.parametrize("labels", ["f32", "i64", None])
def test_gather_bit_equal(dtype, F, labels):
    """784 bf16: 98 granules of 16 B (two per lane, the second partial);
    136 bf16: 17 granules (one partial pass); 10 bf16: 20 B rows, the
    element path with rows that are not 16 B aligned; 20 fp32: 80 B = 5
    granules."""
    n, k = 1000, 300  # 300 rows > 4 waves per block: several blocks
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(n, F, device=DEV, generator=g).to(dtype).contiguous()
    y = {"f32": torch.randn(n, 1, device=DEV, generator=g),
         "i64": torch.randint(-2**40, 2**40, (n, 1), device=DEV, generator=g),
         None: None}[labels]
    _gather_case(x, y, k)


def test_gather_wide_labels_and_full_permutation():
    n = 257
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(n, 24, device=DEV, generator=g).to(torch.bfloat16)
    y = torch.randn(n, 70, device=DEV, generator=g)  # more label words than lanes
    _gather_case(x, y, n)


def test_gather_misaligned_base_takes_element_path():
    """x and xb start 2 bytes into an allocation: rows are whole granules but
    the base pointers are not 16 B aligned."""
    ext = ops.ext()
    n, k, F = 64, 16, 784
    g = torch.Generator(device=DEV).manual_seed(3)
    flat = torch.randn(n * F + 8, device=DEV, generator=g).to(torch.bfloat16)
    x = flat[1:1 + n * F].view(n, F)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    _gather_case(x, None, k)
    # aligned x, misaligned xb
    x2 = flat[:n * F].view(n, F)
    out = torch.zeros(k * F + 8, dtype=torch.bfloat16, device=DEV)
    xb = out[1:1 + k * F].view(k, F)
    ext.sample_gather(x2, None, xb, None, SEED, _step_dev(0), None)
    idx = torch.from_numpy(permuted_indices(n, k, SEED, 0)).to(DEV)
    assert torch.equal(_bits(xb), _bits(x2[idx]))
    assert out[0] == 0 and (out[1 + k * F:] == 0).all()


def test_binding_rejects_bad_arguments():
    ext = ops.ext()
    x = torch.zeros(8, 4, device=DEV)
    sd = _step_dev(0)
    with pytest.raises(RuntimeError):  # k > n
        ext.sample_gather(x, None, torch.zeros(9, 4, device=DEV), None, SEED, sd, None)
    with pytest.raises(RuntimeError):  # y without yb
        ext.sample_gather(x, torch.zeros(8, 1, device=DEV), torch.zeros(2, 4, device=DEV), None,
                          SEED, sd, None)
    with pytest.raises(RuntimeError):  # row width mismatch
        ext.sample_gather(x, None, torch.zeros(2, 5, device=DEV), None, SEED, sd, None)
    with pytest.raises(RuntimeError):  # fp64 rows
        ext.sample_gather(x.double(), None, torch.zeros(2, 4, device=DEV).double(), None, SEED,
                          sd, None)


def test_sampler_graph_capture_draws_new_batch_per_replay():
    n, k = 4099, 64
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(n, 784, device=DEV, generator=g).to(torch.bfloat16)
    y = torch.randint(0, 10, (n, 1), device=DEV, generator=g)
    s = DeviceMinibatchSampler(x, y, k, seed=SEED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.next()  # eager warmup consumes draw 0
    torch.cuda.current_stream().wait_stream(side)
    t0 = int(s.step_dev)
    assert t0 == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xb, yb = s.next()
    assert int(s.step_dev) == t0  # capture records, it does not run
    seen = []
    for r in range(3):
        graph.replay()
        idx = torch.from_numpy(s.indices(t0 + r)).to(DEV)
        assert torch.equal(_bits(xb), _bits(x[idx])), r
        assert torch.equal(yb, y[idx]), r
        seen.append(xb.clone())
    assert int(s.step_dev) == t0 + 3
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert not torch.equal(seen[0], seen[2])


def test_train_step_sampled_hipgraph_matches_eager():
    """Three replays of the captured draw + gather + step against three eager
    sampled steps from the same weights and seed.

    Tolerance: that of the existing hipgraph-vs-eager check on this model,
    tests/test_gpu_mlp_fusion.py::test_chain_sync_trainer_hipgraph_vs_eager,
    where two runs of the same step differ only by the order of fp32 atomics
    in the weight-gradient kernels: losses within 1e-3 relative.  The weights
    get the same figure relative to the largest weight of each tensor; a run
    on other batches than the eager one moves most weights by lr per step
    (Adam) and misses it by two orders of magnitude."""
    n, k, lr = 4096, 256, 1e-3
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(n, 784, device=DEV, generator=g).to(torch.bfloat16)
    y = torch.randint(0, 10, (n, 1), device=DEV, generator=g)
    torch.manual_seed(6)
    init = MnistMLPFused().state_dict()

    def run(mode):
        model = MnistMLPFused()
        model.load_state_dict(init)
        tr = SyncTrainer(model, nn.CrossEntropyLoss(), torch.optim.Adam(model.parameters(), lr=lr),
                         device=DEV, world_size=1, compile_mode=mode)
        s = DeviceMinibatchSampler(x, y, k, seed=SEED)
        losses = [tr.train_step_sampled(s)]
        after_first = int(s.step_dev)
        losses += [tr.train_step_sampled(s) for _ in range(2)]
        return tr, s, losses, after_first

    te, se, le, _ = run(None)
    tg, sg, lg, after_first = run("hipgraph")
    print("eager", le, "graph", lg)
    # warmup + capture consumed no draws: the first call ends on draw 1
    assert after_first == 1
    assert int(se.step_dev) == 3 and int(sg.step_dev) == 3
    assert tg._sampled_graph is not None and te._sampled_graph is None
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a), (le, lg)
    moved = False
    for (name, p), (_, q) in zip(tg.model.named_parameters(), te.model.named_parameters()):
        diff = (p.float() - q.float()).abs().max().item()
        ref = q.float().abs().max().item()
        print(name, "max|dw|", diff, "max|w|", ref)
        assert diff <= 1e-3 * ref, name
        moved = moved or not torch.equal(q.detach().cpu().float(), init[name].float())
    assert moved


def test_train_step_sampled_step_dev_restored_after_capture():
    """The sampler's counter right after the capture equals its value before
    the call, so warmup consumed no draws (checked before the first replay by
    building the graph from a sampler that is already at draw 5)."""
    n, k = 4096, 256
    x = torch.randn(n, 784, device=DEV).to(torch.bfloat16)
    y = torch.randint(0, 10, (n, 1), device=DEV)
    model = MnistMLPFused()
    tr = SyncTrainer(model, nn.CrossEntropyLoss(), torch.optim.Adam(model.parameters(), lr=1e-3),
                     device=DEV, world_size=1, compile_mode="hipgraph")
    s = DeviceMinibatchSampler(x, y, k, seed=SEED)
    s.step_dev.fill_(5)
    seen = {}
    replay = torch.cuda.CUDAGraph.replay

    def spy(graph):
        seen.setdefault("before_first_replay", int(s.step_dev))
        return replay(graph)

    torch.cuda.CUDAGraph.replay = spy
    try:
        tr.train_step_sampled(s)
    finally:
        torch.cuda.CUDAGraph.replay = replay
    assert seen["before_first_replay"] == 5
    assert int(s.step_dev) == 6


def _df(n=64, dim=20):
    rng = np.random.RandomState(0)
    feats = rng.normal(0, 1, (n, dim)).astype(np.float64)
    labels = (feats.sum(axis=1) > 0).astype(np.float64)
    return LocalDataFrame.from_arrays(feats, list(labels), num_partitions=1)


def _no_host_draw(*a, **kw):
    raise AssertionError("np.random.choice called on the GPU minibatch path")


@pytest.mark.parametrize("compile_mode", [None, "hipgraph"])
def test_estimator_minibatch_fit_makes_no_host_draw(monkeypatch, compile_mode):
    df = _df()
    obj = serialize_torch_obj(MnistMLP(in_dim=20, hidden=32, classes=2), nn.CrossEntropyLoss(),
                              torch.optim.Adam, lr=0.01)
    monkeypatch.setattr(np.random, "choice", _no_host_draw)
    model = SparkTorch(
        inputCol="features", labelCol="label", predictionCol="predicted", torchObj=obj,
        iters=5, miniBatch=8, validationPct=0.0, device="cuda:0", mode="synchronous",
        compileMode=compile_mode,
    ).fit(df)
    preds = {r["predicted"] for r in model.transform(df).collect()}
    assert preds.issubset({0.0, 1.0})


def test_hogwild_minibatch_fit_makes_no_host_draw(monkeypatch):
    df = _df()
    obj = serialize_torch_obj(MnistMLP(in_dim=20, hidden=16, classes=2), nn.MSELoss(),
                              torch.optim.Adam, lr=0.01)
    monkeypatch.setattr(np.random, "choice", _no_host_draw)
    model = SparkTorch(
        inputCol="features", labelCol="label", predictionCol="predicted", torchObj=obj,
        iters=3, miniBatch=8, validationPct=0.0, mode="hogwild", port=free_port(),
        device="cuda:0", acquireLock=True,
    ).fit(df)
    assert model.transform(df).count() == 64
