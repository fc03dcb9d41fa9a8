"""MLPAutoEncoderFused off the GPU: the F.linear / F.relu stack and the layer
names a plain torch module shares."""

import torch
import torch.nn.functional as F

from sparktorch_amd.ops.modules import MLPAutoEncoderFused


def test_autoencoder_cpu_forward_and_state_dict():
    torch.manual_seed(0)
    m = MLPAutoEncoderFused(24, (16, 8, 16))
    assert list(m.state_dict()) == ["fc%d.%s" % (i, n) for i in range(1, 5)
                                    for n in ("weight", "bias")]
    assert [tuple(m.state_dict()["fc%d.weight" % i].shape) for i in range(1, 5)] == [
        (16, 24), (8, 16), (16, 8), (24, 16)]
    x = torch.randn(5, 24)
    h = x
    for i in range(1, 5):
        fc = getattr(m, "fc%d" % i)
        h = F.linear(h, fc.weight, fc.bias)
        if i < 4:
            h = F.relu(h)
    assert torch.equal(m(x), h)
    plain = torch.nn.Module()
    for i, (a, b) in enumerate([(24, 16), (16, 8), (8, 16), (16, 24)], 1):
        setattr(plain, "fc%d" % i, torch.nn.Linear(a, b))
    plain.load_state_dict(m.state_dict())
