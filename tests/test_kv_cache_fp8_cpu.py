"""fp8 (e4m3) KV cache through the CPU branches: the quantisation rule's
edges, and the model path against the same steps on a plain cache that was
fed the dequantised K/V."""

import pytest
import torch

from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM, KVCache
from dolomite_engine_amd.hf_models import modeling
from dolomite_engine_amd.ops import QKVLayout, decode_attention, quantize_kv_e4m3

FP8 = torch.float8_e4m3fn


def _row(**at):
    x = torch.zeros(16)
    for i, val in at.items():
        x[int(i[1:])] = val
    return x.to(torch.bfloat16)


RULE_EDGES = {
    # name: (row, expected scale, expected q as floats)
    "all_zero": (_row(), 2.0 ** -64 / 448, torch.zeros(16)),
    # bf16 subnormals (2^-133 steps): amax clamps to 2^-64, x * 448 * 2^64 is far below e4m3's 2^-9
    "subnormals": (_row(_0=2.0 ** -130, _5=-(2.0 ** -133)), 2.0 ** -64 / 448, torch.zeros(16)),
    # one element carries the amax: it lands on +-448 exactly, the rest on 0
    "single_amax": (_row(_3=-3.0), 3.0 / 448, _row(_3=-448.0).float()),
    # 1.0 * (448 / 1.75) = 256, 0.0625 * 256 = 16
    "two_values": (_row(_0=1.75, _1=1.0, _2=0.0625), 1.75 / 448, _row(_0=448.0, _1=256.0, _2=16.0).float()),
}


@pytest.mark.parametrize("name", RULE_EDGES)
def test_rule_edges(name):
    x, want_scale, want_q = RULE_EDGES[name]
    q, scale = quantize_kv_e4m3(x[None])
    assert q.dtype == FP8 and q.shape == (1, 16) and scale.dtype == torch.float32 and scale.shape == (1,)
    assert float(scale[0]) == float(torch.tensor(want_scale, dtype=torch.float32))
    assert torch.equal(q[0].float(), want_q)
    assert not torch.isnan(q.float()).any()


def _model(head_type="mqa", Hkv=1):
    torch.manual_seed(0)
    cfg = GPTDolomiteConfig(
        vocab_size=97, n_positions=64, n_embd=64, n_layer=2, n_head=4,
        attention_head_type=head_type, num_key_value_heads=Hkv, n_inner=128,
        activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type="rope", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
        tie_word_embeddings=False, initializer_range=0.2,
    )
    cfg._attn_implementation = "flash_attention_2"
    return GPTDolomiteForCausalLM(cfg).eval()


def test_cache_allocation():
    cfg = _model("gqa", 2).config
    c = KVCache(cfg, 3, 10, torch.float32, "cpu", kv_dtype="fp8")
    assert len(c.k) == len(c.v) == len(c.k_scale) == len(c.v_scale) == 2
    assert c.k[0].dtype == c.v[1].dtype == FP8 and c.k[0].shape == (3, 10, 2, 16)
    assert c.k_scale[0].dtype == c.v_scale[1].dtype == torch.float32 and c.v_scale[1].shape == (3, 2, 10)
    plain = KVCache(cfg, 3, 10, torch.float32, "cpu")
    assert plain.k[0].dtype == torch.float32 and plain.k_scale == [None, None] and plain.kv_dtype is None
    with pytest.raises(NotImplementedError, match="extend"):
        KVCache(cfg, 3, 10, torch.float32, "cpu", multi_token=True, kv_dtype="fp8")
    with pytest.raises(ValueError):
        KVCache(cfg, 3, 10, torch.float32, "cpu", kv_dtype="int8")
    # the ops: scales are required with an fp8 cache, shape-checked, and refused without one
    lo, lens, qkv = QKVLayout.make(4, 2, 16, "gqa"), torch.ones(3, dtype=torch.int32), torch.zeros(3, 128)
    for bad, match in ((dict(), "needs k_scale"), (dict(k_scale=c.k_scale[0][..., :4], v_scale=c.v_scale[0]), "must be fp32")):
        with pytest.raises(ValueError, match=match):
            decode_attention(qkv, lo, c.k[0], c.v[0], lens, 0.25, 10, **bad)
    with pytest.raises(ValueError, match="go with"):
        decode_attention(qkv, lo, plain.k[0], plain.v[0], lens, 0.25, 10, k_scale=c.k_scale[0], v_scale=c.v_scale[0])


@pytest.mark.parametrize("head_type,Hkv", [("mqa", 1), ("gqa", 2)])
def test_model_steps_equal_dequantised_plain_cache(head_type, Hkv, monkeypatch):
    """Prefill + two decode steps on the fp8 cache against the same steps on
    a plain cache whose appends were fed dequant(quant(K)), dequant(quant(V)):
    the same numbers reach the same attention arithmetic, so the logits are
    equal, not close."""
    model = _model(head_type, Hkv)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 97, (3, 7), generator=g)
    mask = torch.ones(3, 7, dtype=torch.long)
    mask[1, :4] = 0          # left padding
    mask[2, :6] = 0
    feed = torch.randint(1, 97, (2, 3), generator=g)

    def steps(cache):
        with torch.no_grad():
            out = [model(input_ids=ids, attention_mask=mask, past_key_values=cache, use_cache=True).logits[:, -1]]
            for t in range(2):
                out.append(model(input_ids=feed[t][:, None], past_key_values=cache, use_cache=True).logits[:, 0])
        return torch.stack(out)

    got = steps(KVCache(model.config, 3, 12, torch.float32, "cpu", kv_dtype="fp8"))

    plain_append = modeling.kv_cache_append

    def dequantised_append(qkv, layout, *args, **kw):
        qkv = qkv.clone()
        for slot in layout.unpack_cpu(qkv)[1:]:     # views of the K and V slots
            q8, scale = quantize_kv_e4m3(slot)
            slot.copy_(q8.float() * scale[..., None])
        return plain_append(qkv, layout, *args, **kw)

    monkeypatch.setattr(modeling, "kv_cache_append", dequantised_append)
    want = steps(KVCache(model.config, 3, 12, torch.float32, "cpu"))
    monkeypatch.undo()
    unquantised = steps(KVCache(model.config, 3, 12, torch.float32, "cpu"))

    torch.testing.assert_close(got, want, rtol=0, atol=0)
    assert torch.equal(got[0], unquantised[0]), "the prefill attends the unquantised K/V"
    assert not torch.equal(got[1:], unquantised[1:]), "the decode steps never saw the quantised cache"


def test_generate_fp8_and_refusals():
    model = _model()
    ids = torch.randint(1, 97, (2, 5), generator=torch.Generator().manual_seed(2))
    out = model.generate(ids, max_new_tokens=4, kv_cache_dtype="fp8")
    assert out.shape == (2, 9) and torch.equal(out[:, :5], ids)
    with pytest.raises(NotImplementedError, match="extend"):
        model.generate(ids, max_new_tokens=4, kv_cache_dtype="fp8", prefill_chunk_size=2)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        model.generate(ids, max_new_tokens=4, kv_cache_dtype="fp8",
                       past_key_values=KVCache(model.config, 2, 16, torch.float32, "cpu"))
