"""Pin the oracle (CPU restatement) to golden vectors generated from the
reference's own CPU eager path (oracle/gen_golden.py).

Tolerances mirror the reference's own suite
(tests/hf_models/single_gpu/hf_models/gpt_dolomite_test.py:59-80):
fp32 logits atol 3e-7, loss atol 1e-5.
"""

import math

import pytest
import torch

from oracle import (
    OracleConfig,
    OracleGPTDolomiteForCausalLM,
    adamw_step_ref,
    apply_rope_ref,
    attention_varlen_ref,
    cross_entropy_ref,
    layernorm_ref,
    lm_loss_padding_free_ref,
    rmsnorm_ref,
    rope_cos_sin_ref,
    softmax_cross_entropy_fwd_bwd_ref,
)

MODEL_CASES = [
    "mqa_rope_rmsnorm_gelu",
    "gqa_rope_rmsnorm_swiglu",
    "mha_abs_layernorm_gelu",
    "mqa_rope_rmsnorm_gelu_mup",
]


def _load(golden_dir, name):
    p = golden_dir / name
    if not p.exists():
        pytest.skip(f"golden fixture {name} missing")
    from oracle.golden import load_golden

    return load_golden(p)


def _oracle_from_fixture(fx):
    ckw = fx["config"]
    cfg = OracleConfig(
        vocab_size=ckw["vocab_size"],
        n_positions=ckw["n_positions"],
        n_embd=ckw["n_embd"],
        n_layer=ckw["n_layer"],
        n_head=ckw["n_head"],
        num_key_value_heads=ckw.get("num_key_value_heads"),
        n_inner=ckw.get("n_inner"),
        activation_function=ckw["activation_function"],
        attention_head_type=ckw["attention_head_type"],
        normalization_function=ckw["normalization_function"],
        layer_norm_epsilon=ckw["layer_norm_epsilon"],
        add_bias=ckw["add_bias"],
        position_embedding_type=ckw["position_embedding_type"],
        m_emb=ckw.get("m_emb"),
        m_width=ckw.get("m_width"),
        m_residual=ckw.get("m_residual"),
        attention_multiplier=ckw.get("attention_multiplier"),
        tie_word_embeddings=False,
    )
    model = OracleGPTDolomiteForCausalLM(cfg)
    missing, unexpected = model.load_state_dict(fx["state_dict"], strict=False)
    # rope caches / buffers in the reference state dict are recomputed here
    assert not missing, missing
    for k in unexpected:
        assert "rope" in k or "masked_bias" in k or "bias" in k.split(".")[-1], k
    return model, cfg


def _pack(input_ids):
    """Dense (B,S) -> packed (T,), position_ids, cu_seqlens, max_seqlen."""
    B, S = input_ids.shape
    packed = input_ids.reshape(-1)
    position_ids = torch.arange(S).repeat(B)
    cu_seqlens = torch.arange(0, B * S + 1, S, dtype=torch.int32)
    return packed, position_ids, cu_seqlens, S


@pytest.mark.parametrize("case", MODEL_CASES)
def test_oracle_model_matches_reference_golden(golden_dir, case):
    fx = _load(golden_dir, f"model_{case}.pt")
    model, cfg = _oracle_from_fixture(fx)
    model.eval()

    packed, position_ids, cu_seqlens, max_seqlen = _pack(fx["input_ids"])
    logits, _ = model(packed, position_ids, cu_seqlens, max_seqlen)
    B, S = fx["input_ids"].shape
    ref_logits = fx["logits"].reshape(B * S, -1)

    torch.testing.assert_close(logits, ref_logits, rtol=2e-5, atol=3e-6)

    # dense per-row shifted loss == packed loss with boundary drops
    labels = fx["labels"].reshape(-1)
    loss = lm_loss_padding_free_ref(logits, labels, cu_seqlens)
    torch.testing.assert_close(loss, fx["loss"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_oracle_model_backward_matches_reference_golden(golden_dir, case):
    fx = _load(golden_dir, f"model_{case}.pt")
    model, cfg = _oracle_from_fixture(fx)
    model.train()

    packed, position_ids, cu_seqlens, max_seqlen = _pack(fx["input_ids"])
    labels = fx["labels"].reshape(-1)
    logits, loss = model(packed, position_ids, cu_seqlens, max_seqlen, labels=labels)
    loss.backward()

    params = dict(model.named_parameters())
    for k, ref_grad in fx["grads"].items():
        g = params[k].grad
        assert g is not None, k
        torch.testing.assert_close(g, ref_grad, rtol=1e-4, atol=2e-6, msg=lambda m: f"{k}: {m}")


def test_rmsnorm_matches_reference(golden_dir):
    fx = _load(golden_dir, "ops.pt")
    for dtype in ("torch.float32", "torch.bfloat16"):
        c = fx[f"rmsnorm_{dtype}"]
        x = c["x"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        y = rmsnorm_ref(x, w, c["eps"])
        torch.testing.assert_close(y, c["y"], rtol=0, atol=0)  # same math graph -> bitwise
        y.backward(c["dy"])
        torch.testing.assert_close(x.grad, c["dx"], rtol=0, atol=0)
        torch.testing.assert_close(w.grad, c["dw"], rtol=0, atol=0)


def test_layernorm_matches_reference(golden_dir):
    fx = _load(golden_dir, "ops.pt")
    for dtype in ("torch.float32", "torch.bfloat16"):
        c = fx[f"layernorm_{dtype}"]
        x = c["x"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        b = c["b"].clone().requires_grad_(True)
        y = layernorm_ref(x, w, b, c["eps"])
        torch.testing.assert_close(y, c["y"], rtol=0, atol=0)
        y.backward(c["dy"])
        torch.testing.assert_close(x.grad, c["dx"], rtol=0, atol=0)
        torch.testing.assert_close(w.grad, c["dw"], rtol=0, atol=0)
        torch.testing.assert_close(b.grad, c["db"], rtol=0, atol=0)


def test_rope_matches_reference(golden_dir):
    fx = _load(golden_dir, "ops.pt")
    for d in (64, 80, 128):
        c = fx[f"rope_{d}"]
        cos, sin = rope_cos_sin_ref(d, c["cos"].shape[0], 10000.0)
        torch.testing.assert_close(cos, c["cos"], rtol=0, atol=0)
        torch.testing.assert_close(sin, c["sin"], rtol=0, atol=0)
        qr = apply_rope_ref(c["q"], cos[c["pos"]].unsqueeze(1), sin[c["pos"]].unsqueeze(1))
        torch.testing.assert_close(qr, c["q_rotated"], rtol=0, atol=0)


def test_cross_entropy_matches_reference(golden_dir):
    fx = _load(golden_dir, "ops.pt")
    c = fx["cross_entropy"]
    loss = cross_entropy_ref(c["logits"], c["labels"])
    torch.testing.assert_close(loss, c["loss"], rtol=1e-6, atol=1e-7)
    loss2, dlogits = softmax_cross_entropy_fwd_bwd_ref(c["logits"], c["labels"])
    torch.testing.assert_close(loss2, c["loss"], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(dlogits, c["dlogits"], rtol=1e-5, atol=1e-9)


def test_adamw_matches_torch(golden_dir):
    fx = _load(golden_dir, "ops.pt")
    c = fx["adamw"]
    p = c["p0"].clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for t, g in enumerate(c["grads"], start=1):
        adamw_step_ref(p, g, m, v, t, c["lr"], c["beta1"], c["beta2"], c["eps"], c["wd"])
    torch.testing.assert_close(p, c["p_final"], rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(m, c["exp_avg"], rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(v, c["exp_avg_sq"], rtol=1e-6, atol=1e-8)


def test_varlen_attention_equals_per_sequence_dense():
    """Size-independent property: packed varlen attention == independent
    dense causal attention per slice (ragged lengths, GQA)."""
    g = torch.Generator().manual_seed(3)
    H, Hkv, D = 8, 2, 16
    lens = [5, 1, 17, 0, 9]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    q = torch.randn(T, H, D, generator=g)
    k = torch.randn(T, Hkv, D, generator=g)
    v = torch.randn(T, Hkv, D, generator=g)
    out = attention_varlen_ref(q, k, v, cu, 1.0 / math.sqrt(D))
    # manual per-slice check with plain softmax loop
    for i, L in enumerate(lens):
        s = int(cu[i])
        for t in range(L):
            for h in range(H):
                scores = (q[s + t, h] @ k[s : s + t + 1, h * Hkv // H].T) / math.sqrt(D)
                p = torch.softmax(scores, dim=-1)
                o = p @ v[s : s + t + 1, h * Hkv // H]
                torch.testing.assert_close(out[s + t, h], o, rtol=1e-5, atol=1e-6)
