"""ops.glu_activation on the CPU: the eager chain, unchanged."""

import pytest
import torch

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.hf_models.modeling import _activation
from dolomite_engine_amd.ops import hip

NAMES = ["swiglu", "geglu", "gelu_glu", "reglu"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", NAMES)
def test_cpu_branch_is_the_chain_bitwise(name, dtype):
    gen = torch.Generator().manual_seed(0)
    h = (torch.rand(2, 5, 24, generator=gen) * 16 - 8).to(dtype)
    g = torch.randn(2, 5, 12, generator=gen).to(dtype)
    act, is_glu = _activation(name)
    assert is_glu
    outs = []
    for fn in (lambda x: ops.glu_activation(x, name), lambda x: x.chunk(2, -1)[0] * act(x.chunk(2, -1)[1])):
        x = h.clone().requires_grad_(True)
        y = fn(x)
        y.backward(g)
        outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", NAMES)
def test_gradcheck_float64(name):
    h = torch.randn(3, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: ops.glu_activation(x, name), (h,))


@pytest.mark.parametrize("name", ["glu", "tanh_glu", "swiglux", "gelu"])
def test_unknown_name_raises(name):
    with pytest.raises(NotImplementedError):
        ops.glu_activation(torch.zeros(2, 4), name)


# (R, I, ld_h, act, dtype) -> code; all decided before any launch, so null
# pointers and no GPU. Listed in the order the entry points test them.
@pytest.mark.parametrize("args,code", [
    ((4, 8, 16, 4, hip.BF16), 9060), ((4, 8, 16, -1, hip.F32), 9060),
    ((4, 8, 16, 0, 2), 9061),
    ((-1, 8, 16, 0, hip.BF16), 9062), ((4, -8, 16, 0, hip.BF16), 9062),
    ((4, 8, 15, 0, hip.BF16), 9063),
    ((0, 8, 16, 3, hip.BF16), 0), ((4, 0, 0, 3, hip.F32), 0),
], ids=str)
def test_entry_point_codes(args, code):
    R, I, ld_h, act, dtype = args
    lib = hip.lib()
    assert lib.dolomite_glu_fwd(None, None, ld_h, None, R, I, act, dtype) == code
    assert lib.dolomite_glu_bwd(None, None, None, ld_h, None, R, I, act, dtype) == code
