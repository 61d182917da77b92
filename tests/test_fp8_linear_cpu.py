"""fp8 weight-only linears without a GPU: the quantiser, Fp8Linear's
dequantised route and quantize_linears_fp8's module surgery."""

import pytest
import torch
import torch.nn.functional as F

from dolomite_engine_amd.hf_models import (
    Fp8Linear,
    GPTDolomiteConfig,
    GPTDolomiteForCausalLM,
    ParameterizedLinear,
    quantize_linears_fp8,
)
from dolomite_engine_amd.ops import fp8_linear, quantize_weight_e4m3


def _model(**kw):
    torch.manual_seed(0)
    cfg = GPTDolomiteConfig(
        vocab_size=64, n_positions=32, n_embd=32, n_layer=2, n_head=2, attention_head_type="mqa", n_inner=48,
        activation_function="swiglu", normalization_function="rmsnorm", position_embedding_type="rope",
        resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, tie_word_embeddings=True,
    )
    cfg._attn_implementation = "flash_attention_2" if kw else "sdpa"
    return GPTDolomiteForCausalLM(cfg, **kw)


def test_quantiser_round_trips_within_half_a_step():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(24, 80, generator=g) * 10.0 ** (torch.rand(24, 1, generator=g) * 6 - 3)
    w[5] = 0.0
    wq, scale = quantize_weight_e4m3(w.to(torch.bfloat16))
    w = w.to(torch.bfloat16).float()
    assert wq.dtype == torch.float8_e4m3fn and wq.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (24,)
    # e4m3's coarsest step, in the top binade [256, 448], is 32: half of it is 16 / 448 of the row amax
    amax = w.abs().amax(dim=1, keepdim=True)
    assert bool(((wq.float() * scale[:, None] - w).abs() <= amax * (16.0 / 448.0) * (1 + 2.0 ** -20)).all())
    assert bool((wq[5].float() == 0).all()) and bool(torch.isfinite(scale).all()) and float(scale[5]) > 0


@pytest.mark.parametrize("bias", [True, False])
def test_from_linear_matches_dequantised_f_linear(bias):
    torch.manual_seed(2)
    lin = torch.nn.Linear(40, 24, bias=bias)
    q = Fp8Linear.from_linear(lin)
    assert {n for n, _ in q.named_buffers()} == {"weight_q", "weight_scale"} | ({"bias"} if bias else set())
    assert not list(q.parameters())
    x = torch.randn(3, 5, 40)
    with torch.no_grad():
        want = F.linear(x, q.weight_q.float() * q.weight_scale[:, None], lin.bias)
        assert torch.equal(q(x), want)
    with pytest.raises(RuntimeError, match="inference only"):
        q(x.requires_grad_())
    with pytest.raises(ValueError, match=r"\(3, 39\)"):
        fp8_linear(torch.randn(3, 39), q.weight_q, q.weight_scale)


def test_quantize_linears_swaps_the_four_block_linears_only():
    model = _model().eval()
    ids = torch.arange(12).view(2, 6)
    with torch.no_grad():
        before = model(input_ids=ids).logits
    n_linear = sum(isinstance(m, ParameterizedLinear) for m in model.modules())
    assert not any(isinstance(m, Fp8Linear) for m in model.modules())  # importing the code changed nothing
    wte = model.transformer.wte.weight
    assert quantize_linears_fp8(model) is model
    swapped = sorted(n for n, m in model.named_modules() if isinstance(m, Fp8Linear))
    assert swapped == sorted(f"transformer.h.{i}.{p}" for i in range(2)
                             for p in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"))
    assert sum(isinstance(m, ParameterizedLinear) for m in model.modules()) == n_linear - 8
    assert model.transformer.wte.weight is wte and wte.dtype == torch.float32
    assert "transformer.h.0.attn.c_attn.weight_q" in model.state_dict()
    with torch.no_grad():
        after = model(input_ids=ids).logits
    # 3 mantissa bits per weight: close to, and not the same as, the unquantised model
    assert not torch.equal(after, before)
    torch.testing.assert_close(after, before, rtol=0, atol=0.1 * float(before.abs().max()))


def test_quantize_linears_refuses_training_and_padding_free_models():
    with pytest.raises(RuntimeError, match="training"):
        quantize_linears_fp8(_model().train())
    with pytest.raises(RuntimeError, match="padding-free"):
        quantize_linears_fp8(_model(use_padding_free_transformer=True).eval())
