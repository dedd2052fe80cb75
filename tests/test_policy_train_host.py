"""A masked RowDense under RowOptimizer.attach on the CPU (no GPU): whatever a launch, an attached copy or to_linear() reads of the layer is
masked_weight() (the invariant in RowDense's docstring).  The defect this holds off: a layer whose off-block weights are not zero -- nn.Linear's
initialisation under `mask=`, or a `load_state_dict` into a `stack_blocks` layer -- computed masked_weight() while unattached and the RAW weight once
attached, because `attach` copied the raw parameter into the bfloat16 copy; `to_linear()` copied the raw weight too.  tests/test_policy_train.py runs
the same layers through launches and optimiser steps on the GPU."""
import pytest


def _two_blocks():
    import torch
    mask = torch.zeros((64, 64))
    mask[:32, :32] = 1.0
    mask[32:, 32:] = 1.0
    return mask


def _layer(how):
    """-> a masked RowDense 64 -> 64, relu; "loaded" and "data" make its raw off-block weights non-zero."""
    import torch
    from balatro_gym_amd import RowDense, RowPolicy
    torch.manual_seed(7)
    if how == "constructed":   # RowDense(..., mask=...) at its nn.Linear initialisation
        return RowDense(64, 64, "relu", mask=_two_blocks())
    layer = RowPolicy.stack_blocks([torch.nn.Linear(32, 32), torch.nn.Linear(32, 32)], "relu")
    assert torch.equal(layer.block_mask, _two_blocks())
    if how == "loaded":        # a checkpoint whose off-block entries are not zero
        dense = torch.nn.Linear(64, 64)
        layer.load_state_dict({"weight": dense.weight.detach(), "bias": dense.bias.detach(), "block_mask": _two_blocks()})
    else:                      # "data": a write that the version does not see
        layer.weight.data.copy_(torch.nn.Linear(64, 64).weight.detach())
    assert int((layer.weight[layer.block_mask == 0] != 0).sum()) == 2048
    return layer


@pytest.mark.parametrize("how", ["constructed", "loaded", "data"])
def test_attach_and_to_linear_read_the_masked_weight(how):
    import torch
    from balatro_gym_amd import RowOptimizer
    from balatro_gym_amd.rows import _live_shadow
    layer = _layer(how)
    on = layer.block_mask != 0
    bits = lambda t: t.detach().contiguous().view(torch.int16)   # noqa: E731
    x = torch.randn((9, 64))
    want_w = layer.masked_weight().detach().to(torch.bfloat16)
    want_y = layer(x).detach()
    assert torch.equal(layer._w(), want_w), "unattached: the cast of masked_weight()"
    assert int((want_w[~on] != 0).sum()) == 0 and int((want_w[on] != 0).sum()) > 2000
    lin = layer.to_linear()
    assert torch.equal(torch.relu(lin(x)), want_y), "to_linear() computes forward()"
    assert int((lin.weight[~on] != 0).sum()) == 0
    opt = RowOptimizer(layer.parameters(), lr=1e-2, weight_decay=0.01)
    opt.attach(layer)
    assert _live_shadow(layer) is layer.weight_bf16, "attached, and current"
    assert torch.equal(layer._w(), want_w), "attached: _w() is what it was before attach, bfloat16(masked_weight())"
    assert torch.equal(layer._w(), layer.masked_weight().detach().to(torch.bfloat16))
    assert int((bits(layer.weight_bf16)[~on] != 0).sum()) == 0, "the copy's off-block entries are +0.0 bits"
    assert torch.equal(layer(x).detach(), want_y), "forward() did not change"
    assert torch.equal(torch.relu(layer.to_linear()(x)), want_y), "to_linear() behind attach"
    # the parameter itself obeys the mask from here on, so the update pass -- which writes bfloat16(p_new) of the raw parameter, and adds
    # weight_decay * p to the gradient -- keeps a zero at zero
    assert int((layer.weight[~on] != 0).sum()) == 0 and int((bits(layer.weight.detach().to(torch.bfloat16))[~on] != 0).sum()) == 0
    # a checkpoint loaded behind attach: the version moves, the launch casts masked_weight() again until refresh()
    dense = torch.nn.Linear(64, 64)
    layer.load_state_dict({"weight": dense.weight.detach(), "bias": dense.bias.detach(), "block_mask": _two_blocks()})
    assert _live_shadow(layer) is None and torch.equal(layer._w(), layer.masked_weight().detach().to(torch.bfloat16))
    assert torch.equal(torch.relu(layer.to_linear()(x)), layer(x).detach())
