"""hip_mlp_chain on CPU is plain F.linear / F.relu in sequence."""

import torch
import torch.nn.functional as F

from sparktorch_amd.ops.functional import hip_mlp_chain
from sparktorch_amd.ops.modules import MnistMLPFused


def _layers(seed, dims, relus, bias_last=True):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i, relu in enumerate(relus):
        w = torch.randn(dims[i + 1], dims[i], generator=g, requires_grad=True)
        last = i == len(relus) - 1
        b = None if (last and not bias_last) else torch.randn(dims[i + 1], generator=g,
                                                              requires_grad=True)
        layers.append((w, b, relu))
    return layers


def _sequential(x, layers):
    for w, b, relu in layers:
        x = F.linear(x, w, b)
        if relu:
            x = F.relu(x)
    return x


def test_chain_cpu_values_and_grads():
    for bias_last in (True, False):
        dims, relus = (12, 9, 7, 4), (True, True, False)
        a = _layers(3, dims, relus, bias_last)
        b = _layers(3, dims, relus, bias_last)
        xa = torch.randn(5, 12, generator=torch.Generator().manual_seed(4), requires_grad=True)
        xb = xa.detach().clone().requires_grad_(True)
        ya, yb = hip_mlp_chain(xa, a), _sequential(xb, b)
        assert torch.equal(ya, yb)
        ya.square().sum().backward()
        yb.square().sum().backward()
        assert torch.equal(xa.grad, xb.grad)
        for (wa, ba, _), (wb, bb, _) in zip(a, b):
            assert torch.equal(wa.grad, wb.grad)
            if ba is not None:
                assert torch.equal(ba.grad, bb.grad)


def test_mnist_mlp_fused_cpu_uses_chain():
    torch.manual_seed(0)
    m = MnistMLPFused(20, 16, 5)
    assert list(m.state_dict()) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
                                    "fc3.weight", "fc3.bias"]
    x = torch.randn(3, 20)
    want = m.fc3(m.fc2(m.fc1(x)))
    assert torch.equal(m(x), want)
