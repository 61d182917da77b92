"""ops.moe_decode_mlp and the KV cache on MoEDolomite through the CPU lines
(fp32, tiny shapes): the op against its contract in float64, the cached
forward against one uncached forward over the whole sequence, generate()."""

import pytest
import torch

from dolomite_engine_amd import ops
from dolomite_engine_amd.hf_models import KVCache, MoEDolomiteConfig, MoEDolomiteForCausalLM
from dolomite_engine_amd.ops.functional import _moe_decode_act

VOCAB = 97


def contract64(x, selected, gates, w_fc, b_fc, w_proj, b_proj, activation):
    """out[t] = sum_j gates[t,j] (W_proj[e] act(W_fc[e] x[t] + b_fc[e]) + b_proj[e]) in float64."""
    _, fn, glu = _moe_decode_act(activation)
    d = lambda t: None if t is None else t.double()
    x, gates, w_fc, b_fc, w_proj, b_proj = map(d, (x, gates, w_fc, b_fc, w_proj, b_proj))
    out = torch.zeros_like(x)
    for t in range(x.shape[0]):
        for j, e in enumerate(selected[t].tolist()):
            h = w_fc[e] @ x[t] + (0 if b_fc is None else b_fc[e])
            if glu:
                a, b = h.chunk(2)
                h = a * fn(b)
            else:
                h = fn(h)
            out[t] += gates[t, j] * (w_proj[e] @ h + (0 if b_proj is None else b_proj[e]))
    return out


def make_case(T, E, k, H, I, activation, bias, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    F = 2 * I if activation.endswith("glu") else I
    r = lambda *s: torch.randn(*s, generator=g)
    selected = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    gates = torch.softmax(r(T, k), dim=-1)
    args = [r(T, H), selected, gates, r(E, F, H) / H**0.5, r(E, F) if bias else None,
            r(E, H, I) / I**0.5, r(E, H) if bias else None]
    return [a.to(dtype) if a is not None and a.is_floating_point() else a for a in args]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("activation", ["swiglu", "gelu_pytorch_tanh"])
def test_op_cpu_against_float64(activation, bias):
    args = make_case(5, 4, 2, 24, 16, activation, bias)
    out = ops.moe_decode_mlp(*args, activation)
    torch.testing.assert_close(out.double(), contract64(*args, activation), rtol=1e-5, atol=1e-5)


def test_op_refusals():
    assert ops.MOE_DECODE_MAX_TOKENS == 64
    with pytest.raises(ValueError, match="64 tokens"):
        ops.moe_decode_mlp(*make_case(65, 4, 2, 24, 16, "swiglu", False), "swiglu")
    args = make_case(3, 4, 2, 24, 16, "swiglu", False)
    with pytest.raises(ValueError, match="w_fc"):
        ops.moe_decode_mlp(*args, "gelu")                      # F = 2I under a non-GLU activation
    with pytest.raises(ValueError, match="int32"):
        ops.moe_decode_mlp(args[0], args[1].long(), *args[2:], "swiglu")
    with pytest.raises(ValueError, match="dtype"):
        ops.moe_decode_mlp(args[0], args[1], args[2].double(), *args[3:], "swiglu")


def _model(seed=0):
    torch.manual_seed(seed)
    cfg = MoEDolomiteConfig(
        vocab_size=VOCAB, n_positions=64, n_embd=64, n_layer=2, n_head=4, attention_head_type="gqa",
        num_key_value_heads=2, n_inner=48, activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type="rope", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
        tie_word_embeddings=False, initializer_range=0.2, num_experts=4, num_experts_per_tok=2,
    )
    cfg._attn_implementation = "flash_attention_2"
    return MoEDolomiteForCausalLM(cfg).eval()


def test_cached_logits_equal_uncached():
    """Prefill (7), three decode steps, one extend step (3) on a multi_token
    cache: every step's logits are the rows of one uncached forward over all
    13 tokens."""
    model = _model()
    ids = torch.randint(1, VOCAB, (3, 13), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(input_ids=ids).logits
        cache = KVCache(model.config, 3, 16, torch.float32, "cpu", multi_token=True)
        out = model(input_ids=ids[:, :7], past_key_values=cache, use_cache=True)
        assert out.past_key_values is cache and out.router_logits is None
        torch.testing.assert_close(out.logits, want[:, :7])
        for t in range(7, 10):
            got = model(input_ids=ids[:, t : t + 1], past_key_values=cache).logits
            torch.testing.assert_close(got[:, 0], want[:, t])
        got = model(input_ids=ids[:, 10:], past_key_values=cache).logits
        torch.testing.assert_close(got, want[:, 10:])
        assert cache.lengths.tolist() == [13, 13, 13]
        with pytest.raises(ValueError, match="router"):
            model(input_ids=ids[:, :1], use_cache=True, output_router_logits=True)


def test_generate():
    model = _model()
    ids = torch.randint(1, VOCAB, (2, 5), generator=torch.Generator().manual_seed(2))
    out = model.generate(ids, max_new_tokens=4)
    assert out.shape == (2, 9) and torch.equal(out[:, :5], ids)
