"""Dense flash_attention_2 on CPU: span_attention (the plain-torch branch of
the op the GPU runs) against a float64 reference written here, the dense
"flash_attention_2" model against dense "eager" on the same weights, the
mask-with-a-hole error, and dropout against the keep-mask restatement at the
global row indices b*S + pos."""

import math

import pytest
import torch

from dolomite_engine_amd.hf_models import (
    GPTDolomiteConfig,
    GPTDolomiteForCausalLM,
    MoEDolomiteConfig,
    MoEDolomiteForCausalLM,
)
from dolomite_engine_amd.ops import QKVLayout, attention_dropout_keep_mask, span_attention

LAYOUTS = [("mqa", 4, 1, 16), ("gqa", 4, 2, 8), ("mha", 2, 2, 16)]
# B = 4 rows of S = 12: a full row, a long one, length 1 and an empty span
S_ROW = 12
LENS = [12, 7, 1, 0]


def spans_for(lens, S, side):
    """(begin, end) int32 tensors of row b's span inside its S rows."""
    begin = [b * S + (0 if side == "right" else S - n) for b, n in enumerate(lens)]
    end = [s + n for s, n in zip(begin, lens)]
    return torch.tensor(begin, dtype=torch.int32), torch.tensor(end, dtype=torch.int32)


def _heads64(qkv, lo):
    """q (T,H,D), k/v (T,Hkv,D) float64 leaves-of-views of the packed buffer,
    by the address formula of include/dolomite_hip.h (no shared code)."""
    T = qkv.shape[0]
    x = qkv.double()
    q = torch.stack(
        [x[:, (h // lo.G) * lo.q_gstride + (h % lo.G) * lo.D:][:, : lo.D] for h in range(lo.H)], dim=1
    )
    k = torch.stack([x[:, lo.k_off + j * lo.kv_hstride:][:, : lo.D] for j in range(lo.Hkv)], dim=1)
    v = torch.stack([x[:, lo.v_off + j * lo.kv_hstride:][:, : lo.D] for j in range(lo.Hkv)], dim=1)
    assert q.shape == (T, lo.H, lo.D)
    return q, k, v


def reference_span_attention(qkv, begin, end, lo, scale, keep=None, rp=1.0):
    """Per-span causal softmax in float64. keep: {span index: (H, L, L) bool}."""
    q, k, v = _heads64(qkv, lo)
    o = torch.zeros(qkv.shape[0], lo.H * lo.D, dtype=torch.float64)
    for i, (s, e) in enumerate(zip(begin.tolist(), end.tolist())):
        L = e - s
        if L == 0:
            continue
        causal = torch.ones(L, L, dtype=torch.bool).tril()
        for h in range(lo.H):
            j = h // lo.G
            sc = (q[s:e, h] @ k[s:e, j].T) * scale
            p = torch.softmax(sc.masked_fill(~causal, float("-inf")), dim=-1)
            if keep is not None:
                p = p * keep[i][h] * rp
            o[s:e, h * lo.D : (h + 1) * lo.D] = p @ v[s:e, j]
    return o


def _gap_rows(begin, end, T):
    inside = torch.zeros(T, dtype=torch.bool)
    for s, e in zip(begin.tolist(), end.tolist()):
        inside[s:e] = True
    return ~inside


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS)
def test_span_attention_cpu_vs_float64_reference(head_type, H, Hkv, D, side):
    lo = QKVLayout.make(H, Hkv, D, head_type)
    begin, end = spans_for(LENS, S_ROW, side)
    T = len(LENS) * S_ROW
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(T, lo.row_len, generator=g)
    do = torch.randn(T, H * D, generator=g)
    scale = 1.0 / math.sqrt(D)

    x = qkv.clone().requires_grad_(True)
    o = span_attention(x, begin, end, max(LENS), lo, scale)
    o.backward(do)

    x64 = qkv.double().requires_grad_(True)
    o64 = reference_span_attention(x64, begin, end, lo, scale)
    o64.backward(do.double())

    # fp32 restatement vs float64: a few fp32 ulps on O(1) values
    torch.testing.assert_close(o.detach().double(), o64.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-5, atol=1e-5)

    gap = _gap_rows(begin, end, T)
    assert int(gap.sum()) == T - sum(LENS)
    assert torch.equal(o.detach()[gap], torch.zeros(int(gap.sum()), H * D))
    assert torch.equal(x.grad[gap], torch.zeros(int(gap.sum()), lo.row_len))
    # and the span rows did get a gradient in every slot class (q, k, v)
    assert bool((x.grad[~gap].abs().sum(0) > 0).all())


@pytest.mark.parametrize("side", ["right", "left"])
def test_span_attention_dropout_cpu_uses_global_row_indices(side):
    """keep(seed, h, t_q, t_k) is asked at the buffer's row indices b*S + pos."""
    head_type, H, Hkv, D = LAYOUTS[1]
    lo = QKVLayout.make(H, Hkv, D, head_type)
    begin, end = spans_for(LENS, S_ROW, side)
    T = len(LENS) * S_ROW
    p, seed = 0.25, (7 << 32) + 12345
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, lo.row_len, generator=g)
    scale = 1.0 / math.sqrt(D)

    keep = {}
    for i, (b, n) in enumerate(zip(range(len(LENS)), LENS)):
        first = 0 if side == "right" else S_ROW - n
        rows = b * S_ROW + first + torch.arange(n)
        keep[i] = attention_dropout_keep_mask(seed, H, rows, rows, p)
    rp = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)))

    o = span_attention(qkv, begin, end, max(LENS), lo, scale, dropout_p=p, seed=seed)
    ref = reference_span_attention(qkv, begin, end, lo, scale, keep=keep, rp=rp)
    torch.testing.assert_close(o.double(), ref, rtol=1e-5, atol=1e-5)
    undropped = span_attention(qkv, begin, end, max(LENS), lo, scale)
    assert not torch.allclose(o, undropped, atol=1e-3)  # the mask did bite
    gap = _gap_rows(begin, end, T)
    assert torch.equal(o[gap], torch.zeros(int(gap.sum()), H * D))


def test_span_attention_p0_draws_no_seed():
    lo = QKVLayout.make(*LAYOUTS[0][1:], LAYOUTS[0][0])
    begin, end = spans_for(LENS, S_ROW, "right")
    qkv = torch.randn(len(LENS) * S_ROW, lo.row_len)
    torch.manual_seed(5)
    before = torch.get_rng_state()
    span_attention(qkv, begin, end, max(LENS), lo, 0.25, dropout_p=0.0)
    assert torch.equal(before, torch.get_rng_state())
    span_attention(qkv, begin, end, max(LENS), lo, 0.25, dropout_p=0.1)
    assert not torch.equal(before, torch.get_rng_state())


# ---------------------------------------------------------------------------
# model: dense flash_attention_2 vs dense eager, fp32 on CPU
# ---------------------------------------------------------------------------

_KW = dict(
    vocab_size=97, n_positions=32, n_embd=32, n_layer=2, n_head=4, n_inner=64,
    attention_head_type="gqa", num_key_value_heads=2, activation_function="swiglu",
    normalization_function="rmsnorm", position_embedding_type="rope",
    resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, tie_word_embeddings=False,
)


def _pair(family):
    """(flash, eager) models of one family with the same weights."""
    models = []
    for impl in ("flash_attention_2", "eager"):
        torch.manual_seed(21)
        if family == "gpt_dolomite":
            cfg = GPTDolomiteConfig(**_KW)
            cls = GPTDolomiteForCausalLM
        else:
            cfg = MoEDolomiteConfig(num_experts=4, num_experts_per_tok=2, **_KW)
            cls = MoEDolomiteForCausalLM
        cfg._attn_implementation = impl
        models.append(cls(cfg).train())
    models[1].load_state_dict(models[0].state_dict())
    return models


def _batch(side):
    """B = 3, S = 10. side None: no mask. Labels are -100 on pads and, for
    left padding, on the first real token too: the shifted loss would
    otherwise read the logits of the last PAD position, which the two
    implementations compute differently by design."""
    B, S = 3, 10
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, _KW["vocab_size"], (B, S), generator=g)
    if side is None:
        return ids, None, ids.clone()
    lens = [10, 6, 1]
    mask = torch.zeros(B, S, dtype=torch.long)
    labels = ids.clone()
    for b, n in enumerate(lens):
        lo = 0 if side == "right" else S - n
        mask[b, lo : lo + n] = 1
        labels[b, lo] = -100 if side == "left" else labels[b, lo]
    labels[mask == 0] = -100
    return ids, mask, labels


@pytest.mark.parametrize("side", [None, "right", "left"], ids=["nomask", "right", "left"])
@pytest.mark.parametrize("family", ["gpt_dolomite", "moe_dolomite"])
def test_dense_flash_model_matches_dense_eager(family, side):
    flash, eager = _pair(family)
    ids, mask, labels = _batch(side)
    out_f = flash(input_ids=ids, attention_mask=mask, labels=labels)
    out_e = eager(input_ids=ids, attention_mask=mask, labels=labels)
    out_f.loss.backward()
    out_e.loss.backward()

    tol = dict(rtol=1e-4, atol=2e-5)  # sdpa-vs-golden tolerance of test_dense_matches_reference_golden
    real = torch.ones_like(ids, dtype=torch.bool) if mask is None else mask.bool()
    torch.testing.assert_close(out_f.logits[real], out_e.logits[real], **tol)
    torch.testing.assert_close(out_f.loss, out_e.loss, **tol)
    grads_e = dict(eager.named_parameters())
    for name, p in flash.named_parameters():
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad, grads_e[name].grad, msg=lambda m: f"{name}: {m}", **tol)


def test_dense_flash_model_with_gradient_checkpointing():
    from dolomite_engine_amd.hf_models.modeling import apply_gradient_checkpointing

    flash = _pair("gpt_dolomite")[0]
    plain = _pair("gpt_dolomite")[0]
    apply_gradient_checkpointing(flash, "block", checkpoint_every=1)
    ids, mask, labels = _batch("left")
    out_c = flash(input_ids=ids, attention_mask=mask, labels=labels)
    out_p = plain(input_ids=ids, attention_mask=mask, labels=labels)
    out_c.loss.backward()
    out_p.loss.backward()
    assert torch.equal(out_c.loss, out_p.loss)
    grads_p = dict(plain.named_parameters())
    for name, p in flash.named_parameters():
        assert torch.equal(p.grad, grads_p[name].grad), name


def test_dense_flash_empty_row_and_zero_fill():
    """An all-zero mask row is an empty span; the attention output of pad
    positions is zero, so a pad position's hidden state is what the residual
    stream and the MLPs alone make of its embedding."""
    flash, _ = _pair("gpt_dolomite")
    ids, mask, labels = _batch("right")
    mask[2] = 0
    labels[2] = -100
    out = flash(input_ids=ids, attention_mask=mask, labels=labels)
    assert torch.isfinite(out.logits).all() and torch.isfinite(out.loss)
    (begin, end, max_seqlen), _ = flash.transformer.dense_flash_inputs(
        mask, torch.arange(10).expand(3, -1), 3, 10, ids.device, torch.float32
    )
    assert begin.tolist() == [0, 10, 20] and end.tolist() == [10, 16, 20] and max_seqlen == 10
    assert begin.dtype == torch.int32 and end.dtype == torch.int32


def test_mask_with_a_hole_raises_value_error():
    flash, _ = _pair("gpt_dolomite")
    ids, mask, _ = _batch("right")
    mask[1, 2] = 0  # 1 1 0 1 1 1 0 0 0 0
    with pytest.raises(ValueError, match="contiguous"):
        flash(input_ids=ids, attention_mask=mask)


def test_alibi_with_flash_still_asserts():
    kw = dict(_KW, position_embedding_type="alibi")
    cfg = GPTDolomiteConfig(**kw)
    cfg._attn_implementation = "flash_attention_2"
    with pytest.raises(AssertionError, match="alibi"):
        GPTDolomiteForCausalLM(cfg)
