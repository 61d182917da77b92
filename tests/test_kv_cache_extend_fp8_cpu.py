"""The extend step over an fp8 (e4m3) KV cache through the CPU branches: the
op dequantises exactly, and the model carries the scales into the extend step
(fp8 cache with multi_token set after construction)."""

import pytest
import torch

from dolomite_engine_amd.hf_models import KVCache, modeling
from dolomite_engine_amd.ops import QKVLayout, extend_attention, quantize_kv_e4m3
from tests.test_kv_cache_fp8_cpu import _model


def test_extend_fp8_equals_dequantised_float_cache():
    lo = QKVLayout.make(4, 2, 16, "gqa")
    g = torch.Generator().manual_seed(4)
    past_n = [(0, 5), (7, 3), (9, 0), (2, 1)]
    qkv = torch.randn(4 * 6, lo.row_len, generator=g)
    k8, ks = quantize_kv_e4m3(torch.randn(4, 13, 2, 16, generator=g) * 3)
    v8, vs = quantize_kv_e4m3(torch.randn(4, 13, 2, 16, generator=g) * 5)
    ks, vs = ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()   # (B, Hkv, S_cap)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    sb, se = i32([6 * b for b in range(4)]), i32([6 * b + n for b, (_, n) in enumerate(past_n)])
    lens = i32([p + n for p, n in past_n])
    with torch.no_grad():
        got = extend_attention(qkv, lo, sb, se, 5, k8, v8, lens, 0.25, 12, k_scale=ks, v_scale=vs)
        want = extend_attention(qkv, lo, sb, se, 5, k8.float() * ks.transpose(1, 2)[..., None],
                                v8.float() * vs.transpose(1, 2)[..., None], lens, 0.25, 12)
    assert got.abs().sum() > 0
    torch.testing.assert_close(got, want, rtol=0, atol=0)


@pytest.mark.parametrize("head_type,Hkv", [("mqa", 1), ("gqa", 2)])
def test_model_extend_step_equals_dequantised_plain_cache(head_type, Hkv, monkeypatch):
    """Prefill, one 3-token extend step, one decode step on an fp8 cache
    against the same steps on a plain multi_token cache whose appends were fed
    dequant(quant(K)), dequant(quant(V)): equal, not close. The extend step
    attends the quantised K/V of its own tokens, so it differs from the
    unquantised cache's."""
    model = _model(head_type, Hkv)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 97, (3, 7), generator=g)
    mask = torch.ones(3, 7, dtype=torch.long)
    mask[1, :4] = 0          # left padding
    mask[2, :6] = 0
    feed = torch.randint(1, 97, (3, 4), generator=g)

    def steps(cache):
        cache.multi_token = True   # the opt-in for an fp8 cache
        with torch.no_grad():
            model(input_ids=ids, attention_mask=mask, past_key_values=cache, use_cache=True)
            ext = model(input_ids=feed[:, :3], past_key_values=cache, use_cache=True).logits
            dec = model(input_ids=feed[:, 3:], past_key_values=cache, use_cache=True).logits
        assert cache.lengths.tolist() == [11, 7, 5]
        return torch.cat([ext, dec], dim=1)

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
    assert not torch.equal(got[:, :3], unquantised[:, :3]), "the extend step never saw the quantised cache"
