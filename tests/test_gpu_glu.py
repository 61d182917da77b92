"""The fused GLU activation kernels (csrc/elementwise.hip, ops.glu_activation)
against the three formulas in float64, and the model paths that call them."""

import math

import pytest
import torch
import torch.nn.functional as F

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.hf_models.config import GPTDolomiteConfig
from dolomite_engine_amd.hf_models.modeling import MLP
from dolomite_engine_amd.hf_models.moe import MoEDolomiteConfig, SparseMoE
from dolomite_engine_amd.ops import hip

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
# name -> (DOLOMITE_ACT_* code, the torch activation of the eager chain)
ACTS = {
    "swiglu": (0, F.silu),
    "geglu": (1, lambda x: F.gelu(x, approximate="tanh")),
    "gelu_glu": (2, F.gelu),
    "reglu": (3, F.relu),
}


def _inputs(R, I, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    h = (torch.rand(R, 2 * I, generator=gen, dtype=torch.float64) * 16 - 8).to(dtype).cuda()
    g = (torch.rand(R, I, generator=gen, dtype=torch.float64) * 16 - 8).to(dtype).cuda()
    return h, g


def _ref64(h, g, name):
    """y = up*act(gate), dh = [g*act(gate) ; g*up*act'(gate)] in float64."""
    (up, x), g = h.double().chunk(2, -1), g.double()
    if name == "swiglu":
        s = torch.sigmoid(x)
        a, da = x * s, s * (1 + x * (1 - s))
    elif name == "geglu":
        t = torch.tanh(K0 * (x + K1 * x**3))
        a, da = 0.5 * x * (1 + t), 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * K0 * (1 + 3 * K1 * x * x)
    elif name == "gelu_glu":
        c = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
        a, da = x * c, c + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    else:
        a, da = x.clamp_min(0), (x > 0).double()
    return up * a, torch.cat([g * a, g * up * da], -1)


# (300, 264): 9900 bf16 / 19800 fp32 vectors against the 1024 a workgroup
# covers, so several workgroups and a partial last one; the chosen launch
# shape (one pass per workgroup, no grid stride) has no wrap to reach.
@pytest.mark.parametrize("shape", [(1, 8), (3, 40), (5, 72), (3, 7), (2, 12), (300, 264)], ids=str)
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ACTS))
def test_glu_vs_float64(name, dtype, shape):
    """fp32: |got - ref64| <= 4 E; bf16: <= 2^-8 |ref64| + 4 E per element (one
    rounding), E = the largest |chain32 - ref64| of the plain torch fp32 chain
    and its autograd gradients on the same inputs."""
    h, g = _inputs(*shape, dtype)
    ref_y, ref_dh = _ref64(h, g, name)

    h32 = h.detach().float().clone().requires_grad_(True)
    a, b = h32.chunk(2, -1)
    y32 = a * ACTS[name][1](b)
    y32.backward(g.float())
    E = max((y32.detach() - ref_y).abs().max().item(), (h32.grad - ref_dh).abs().max().item())

    hq = h.detach().clone().requires_grad_(True)
    y = ops.glu_activation(hq, name)
    y.backward(g)
    assert y.dtype == dtype and y.shape == g.shape and hq.grad.shape == h.shape
    for what, got, ref in (("y", y.detach(), ref_y), ("dh", hq.grad, ref_dh)):
        bound = 4 * E + (ref.abs() * 2.0**-8 if dtype == BF16 else 0)
        err = (got.double() - ref).abs()
        print(f"{name} {dtype} {shape} {what}: max err {err.max().item():.3e}, E {E:.3e}")
        assert bool((err <= bound).all()), f"{what}: {(err > bound).sum().item()} elements past the bound"


@pytest.mark.parametrize("offset", [8, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
def test_strided_rows_and_whole_dh_written(dtype, offset):
    """h as a column slice of a wider buffer (ld_h > 2I; at offset 4 the bf16
    slice is not 16-byte aligned) is bitwise the contiguous call, and the
    entry point writes every element of a NaN-filled dh."""
    R, I = 5, 72
    h, g = _inputs(R, I, dtype, seed=1)
    wide = torch.zeros(R, 2 * I + 24, dtype=dtype, device="cuda")
    view = wide[:, offset : offset + 2 * I]
    view.copy_(h)
    assert view.stride(0) > 2 * I
    outs = []
    for src in (h, view):
        x = src.detach().requires_grad_(True)
        y = ops.glu_activation(x, "swiglu")
        y.backward(g)
        outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])

    dh = torch.full((R, 2 * I), float("nan"), dtype=dtype, device="cuda")
    hip.check(
        hip.lib().dolomite_glu_bwd(hip.stream(), hip.ptr(g), hip.ptr(view), view.stride(0), hip.ptr(dh),
                                   R, I, 0, hip.dt(view)),
        "glu_bwd",
    )
    assert bool(torch.isfinite(dh).all()) and torch.equal(dh, outs[0][1])


@pytest.mark.parametrize("kind", ["mlp", "moe"])
def test_model_activation_is_the_fused_op(kind):
    """The input of c_proj is bitwise ops.glu_activation(output of c_fc): the
    module runs the kernels, not the torch chain (which rounds act(gate) to
    bf16 before the multiply and differs on many elements)."""
    torch.manual_seed(0)
    kw = dict(n_embd=64, n_head=4, n_inner=72, n_layer=2, activation_function="swiglu", resid_pdrop=0.0, add_bias=True,
              initializer_range=1.0)
    if kind == "mlp":
        layer = MLP(GPTDolomiteConfig(**kw))
    else:
        layer = SparseMoE(MoEDolomiteConfig(num_experts=4, num_experts_per_tok=2, **kw))
    layer = layer.to(BF16).cuda()
    seen = {}
    layer.c_fc.register_forward_hook(lambda m, args, out: seen.__setitem__("fc", out.detach().clone()))
    layer.c_proj.register_forward_pre_hook(lambda m, args: seen.__setitem__("proj_in", args[0].detach().clone()))
    layer(torch.randn(96, 64, dtype=BF16, device="cuda"))
    assert seen["fc"].shape[-1] == 144
    assert torch.equal(seen["proj_in"], ops.glu_activation(seen["fc"], "swiglu"))
