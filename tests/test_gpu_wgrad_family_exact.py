"""The three streaming wgrad kernels that share linear_wgrad_tile.h
(linear_wgrad.hip, linear_wgrad_wide.hip, hidden_bwd.hip) on inputs whose
result does not depend on the accumulation order.

dz, x and w are integer-valued bf16 from [-3, 3].  Every product and every
partial sum of dW / db is then an integer of magnitude <= 9 * 4099 < 2^24, an
exact fp32, so any tile walk, any grid, any number of atomics and the half-way
flush must give the float64 result bit for bit, and a second call into the same
buffers exactly twice it.  dz_in's fp32 sum (<= 9 * 256) is exact as well, so
its single bf16 rounding is determined.  A tile staged from the wrong rows or
slots, a tail row not zero-filled, a clamped column flushed or a block that
walks a tile twice or not at all changes an integer, which the error-bound
tests of each kernel may let pass.

The shapes take both fragment counts of a column tile (7 and 8), a clamped last
column tile (Ki = 200, No = 264, No = 1000), a one-row and a three-row partial
tile, the half-way flush on both ring periods (B = 4099, one row group: 128
full tiles) and the XCD deal (B = 4099, free grid: 8 row groups)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops

DEV = "cuda:0"
BATCHES = (33, 4099)
MAX_BLOCKS = (0, 1)
STREAM_SHAPES = [(64, 200), (128, 256), (256, 784)]
WIDE_SHAPES = [(264, 64), (1000, 128), (784, 256)]
HIDDEN_SHAPES = [(128, 200), (256, 256), (256, 784)]


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).to(torch.bfloat16).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(B, No, Ki):
    """Inputs and float64 references of one shape, shared by its tests."""
    g = torch.Generator().manual_seed(1000 * No + Ki + B)
    dz, x, w = _ints(g, B, No), _ints(g, B, Ki), _ints(g, No, Ki)
    assert (x <= 0).any() and (x < 0).any() and (x > 0).any()
    dw = (dz.double().t() @ x.double()).float()
    db = dz.double().sum(0).float()
    dzin = (dz.double() @ w.double()).float().bfloat16()
    dzin[x <= 0] = 0
    return dz, x, w, dw, db, dzin


def _twice(call, No, Ki, ref_dw, ref_db):
    dw = torch.zeros(No, Ki, device=DEV)
    db = torch.zeros(No, device=DEV)
    out = call(dw, db)
    assert torch.equal(dw, ref_dw) and torch.equal(db, ref_db)
    call(dw, db)
    assert torch.equal(dw, 2 * ref_dw) and torch.equal(db, 2 * ref_db)
    return out


@pytest.mark.parametrize("max_blocks", MAX_BLOCKS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("No,Ki", STREAM_SHAPES)
def test_linear_wgrad_stream_exact(No, Ki, B, max_blocks):
    dz, x, _, ref_dw, ref_db, _ = _case(B, No, Ki)
    _twice(lambda dw, db: ops.ext().linear_wgrad_stream(dz, x, dw, db, max_blocks),
           No, Ki, ref_dw, ref_db)


@pytest.mark.parametrize("max_blocks", MAX_BLOCKS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("No,Ki", WIDE_SHAPES)
def test_linear_wgrad_wide_exact(No, Ki, B, max_blocks):
    dz, x, _, ref_dw, ref_db, _ = _case(B, No, Ki)
    _twice(lambda dw, db: ops.ext().linear_wgrad_wide(dz, x, dw, db, max_blocks),
           No, Ki, ref_dw, ref_db)


@pytest.mark.parametrize("max_blocks", MAX_BLOCKS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("No,Ki", HIDDEN_SHAPES)
def test_linear_hidden_bwd_exact(No, Ki, B, max_blocks):
    dz, x, w, ref_dw, ref_db, ref_dzin = _case(B, No, Ki)
    dzin = _twice(lambda dw, db: ops.ext().linear_hidden_bwd(dz, w, x, dw, db, max_blocks),
                  No, Ki, ref_dw, ref_db)
    assert torch.equal(dzin, ref_dzin)
