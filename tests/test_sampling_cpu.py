"""The minibatch sampling rule (utils/sampling.py) and its CPU surface: the
keyed bijection draws distinct, reproducible, uniformly spread rows, the
sampler gathers exactly those rows, and SyncTrainer trains on them."""

import numpy as np
import pytest
import torch
import torch.nn as nn

from sparktorch_amd.models.simple_net import Net
from sparktorch_amd.parallel.sync import SyncTrainer
from sparktorch_amd.utils import DeviceMinibatchSampler, permuted_indices

CASES = [(8, 3), (5, 4), (33, 32), (1000, 100), (4099, 64), (7, 7)]
SEED = 20240607  # fixed: the rule is deterministic, so nothing here can flake
T = 4096


@pytest.mark.parametrize("n,k", CASES)
def test_indices_in_range_distinct_reproducible(n, k):
    prev = None
    for step in (0, 1, 2, 7, 2**31 - 1):
        idx = permuted_indices(n, k, SEED, step)
        assert idx.dtype == np.int64 and idx.shape == (k,)
        assert idx.min() >= 0 and idx.max() < n
        assert len(set(idx.tolist())) == k
        if k == n:
            assert sorted(idx.tolist()) == list(range(n))
        assert np.array_equal(idx, permuted_indices(n, k, SEED, step))
        # a batch is a prefix of the step's permutation
        assert np.array_equal(idx, permuted_indices(n, n, SEED, step)[:k])
        if prev is not None:
            assert not np.array_equal(idx, prev)
        prev = idx


@pytest.mark.parametrize("n,k", CASES)
def test_consecutive_steps_and_seeds_differ(n, k):
    a = permuted_indices(n, k, SEED, 3)
    assert not np.array_equal(a, permuted_indices(n, k, SEED, 4))
    assert not np.array_equal(a, permuted_indices(n, k, SEED + 1, 3))


def test_argument_checks():
    with pytest.raises(ValueError):
        permuted_indices(4, 5, SEED, 0)
    with pytest.raises(ValueError):
        permuted_indices(0, 0, SEED, 0)
    with pytest.raises(ValueError):
        permuted_indices(1 << 31, 1, SEED, 0)
    assert permuted_indices(1, 1, SEED, 0).tolist() == [0]
    big = permuted_indices((1 << 31) - 1, 50, SEED, 0)  # the 2^32 domain
    assert len(set(big.tolist())) == 50 and big.max() < (1 << 31) - 1


@pytest.mark.parametrize("n,k", [(8, 3), (33, 32), (1000, 100)])
def test_uniformity(n, k):
    """Over T consecutive steps every row is included T*k/n times and sits in
    slot 0 T/n times, each within 5 binomial standard deviations."""
    incl = np.zeros(n)
    slot0 = np.zeros(n)
    for step in range(T):
        idx = permuted_indices(n, k, SEED, step)
        incl[idx] += 1
        slot0[idx[0]] += 1
    p = k / n
    z_incl = np.abs(incl - T * p).max() / np.sqrt(T * p * (1 - p))
    p0 = 1 / n
    z_slot0 = np.abs(slot0 - T * p0).max() / np.sqrt(T * p0 * (1 - p0))
    print("n=%d k=%d worst inclusion %.2f sigma, worst slot-0 %.2f sigma" % (n, k, z_incl, z_slot0))
    assert z_incl <= 5.0
    assert z_slot0 <= 5.0


@pytest.mark.parametrize("labels", ["float", "long", None])
def test_sampler_cpu_gathers_reference_rows(labels):
    n, k = 33, 8
    x = torch.arange(n * 5, dtype=torch.float32).reshape(n, 5)
    y = {"float": torch.arange(n, dtype=torch.float32).reshape(n, 1) * 0.5,
         "long": torch.arange(n).reshape(n, 1), None: None}[labels]
    s = DeviceMinibatchSampler(x, y, k, seed=SEED)
    assert not s.native
    for step in range(3):
        idx = torch.from_numpy(permuted_indices(n, k, SEED, step))
        assert np.array_equal(s.indices(step), idx.numpy())
        xb, yb = s.next()
        assert torch.equal(xb, x[idx])
        assert torch.equal(yb, y[idx] if y is not None else x[idx])
    assert int(s.step_dev) == 3


def test_sampler_unseeded_takes_one_numpy_draw():
    x = torch.zeros(16, 2)
    np.random.seed(5)
    a = DeviceMinibatchSampler(x, None, 4)
    np.random.seed(5)
    b = DeviceMinibatchSampler(x, None, 4)
    c = DeviceMinibatchSampler(x, None, 4)
    assert a.seed == b.seed and b.seed != c.seed
    with pytest.raises(ValueError):
        DeviceMinibatchSampler(x, None, 17)


def test_train_step_sampled_cpu_lowers_loss():
    torch.manual_seed(0)
    x = torch.randn(200, 10)
    y = x.sum(dim=1, keepdim=True) * 0.3
    model = Net()
    trainer = SyncTrainer(model, nn.MSELoss(), torch.optim.Adam(model.parameters(), lr=1e-2),
                          device="cpu", world_size=1)
    sampler = DeviceMinibatchSampler(x, y, 32, seed=SEED)
    before = trainer.validation_loss(x, y)
    losses = [trainer.train_step_sampled(sampler) for _ in range(20)]
    after = trainer.validation_loss(x, y)
    assert all(np.isfinite(losses)) and int(sampler.step_dev) == 20
    assert after < before, (before, after)
