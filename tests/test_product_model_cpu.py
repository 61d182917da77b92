"""Product model (dolomite_engine_amd) CPU parity vs reference golden vectors
and vs the oracle:

  - dense eager path vs the reference's own logits/loss/grads (fp32)
  - padding-free packed path (the hot-path graph through the SAME autograd
    Functions the GPU uses, CPU branches) vs the goldens
  - list-input vs tensor-input equivalence (reference
    gpt_dolomite_test.py:203-245 — bit-exact)
"""

import pytest
import torch

from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

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


def build_model(fx, attn_implementation="eager", padding_free=False, dtype=torch.float32):
    ckw = dict(fx["config"])
    ckw.pop("tie_word_embeddings", None)
    cfg = GPTDolomiteConfig(**ckw, tie_word_embeddings=False)
    cfg._attn_implementation = attn_implementation
    model = GPTDolomiteForCausalLM(cfg, use_padding_free_transformer=padding_free)
    missing, unexpected = model.load_state_dict(fx["state_dict"], strict=False)
    assert not missing, missing
    for k in unexpected:
        assert "rope" in k or k.endswith("masked_bias") or k.endswith(".bias"), k
    return model.to(dtype)


@pytest.mark.parametrize("case", MODEL_CASES)
@pytest.mark.parametrize("impl", ["eager", "sdpa"])
def test_dense_matches_reference_golden(golden_dir, case, impl):
    fx = _load(golden_dir, f"model_{case}.pt")
    model = build_model(fx, impl)
    model.eval()
    out = model(input_ids=fx["input_ids"], labels=fx["labels"])
    tol = dict(rtol=2e-5, atol=3e-6) if impl == "eager" else dict(rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(out.logits, fx["logits"], **tol)
    torch.testing.assert_close(out.loss, fx["loss"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_dense_backward_matches_reference_golden(golden_dir, case):
    fx = _load(golden_dir, f"model_{case}.pt")
    model = build_model(fx, "eager")
    model.train()
    out = model(input_ids=fx["input_ids"], labels=fx["labels"])
    out.loss.backward()
    params = dict(model.named_parameters())
    for k, ref_grad in fx["grads"].items():
        torch.testing.assert_close(params[k].grad, ref_grad, rtol=1e-4, atol=2e-6, msg=lambda m: f"{k}: {m}")


@pytest.mark.parametrize("case", MODEL_CASES)
def test_padding_free_cpu_matches_reference_golden(golden_dir, case):
    """The hot-path graph (fused norms, packed rope, varlen attention, fused
    CE — CPU branches of the same autograd Functions the GPU runs)."""
    fx = _load(golden_dir, f"model_{case}.pt")
    model = build_model(fx, "flash_attention_2", padding_free=True)
    model.train()

    B, S = fx["input_ids"].shape
    input_ids = fx["input_ids"].reshape(-1)
    position_ids = torch.arange(S).repeat(B)
    cu_seqlens = torch.arange(0, B * S + 1, S, dtype=torch.int32)
    labels = fx["labels"].reshape(-1)

    out = model(
        input_ids=input_ids,
        position_ids=position_ids,
        cu_seqlens=cu_seqlens,
        max_seqlen=S,
        labels=labels,
    )
    ref_logits = fx["logits"].reshape(B * S, -1)
    torch.testing.assert_close(out.logits, ref_logits, rtol=2e-5, atol=5e-6)
    torch.testing.assert_close(out.loss, fx["loss"], rtol=0, atol=1e-5)

    out.loss.backward()
    params = dict(model.named_parameters())
    for k, ref_grad in fx["grads"].items():
        torch.testing.assert_close(params[k].grad, ref_grad, rtol=1e-4, atol=3e-6, msg=lambda m: f"{k}: {m}")


def test_list_inputs_equal_tensor_inputs(golden_dir):
    """Reference gpt_dolomite_test.py:203-245: list-of-lists inputs must be
    BIT-EXACT vs packed tensor inputs."""
    fx = _load(golden_dir, "model_mqa_rope_rmsnorm_gelu.pt")
    model = build_model(fx, "flash_attention_2", padding_free=True)
    model.eval()

    lists = [[5, 6, 7, 8, 9, 10], [3, 4, 5]]
    labels = [[-100, 6, 7, 8, 9, 10], [-100, 4, 5]]
    out_list = model(input_ids=lists, labels=labels)

    flat = [t for seq in lists for t in seq]
    input_ids = torch.tensor(flat)
    position_ids = torch.tensor([0, 1, 2, 3, 4, 5, 0, 1, 2])
    cu = torch.tensor([0, 6, 9], dtype=torch.int32)
    labels_t = torch.tensor([t for seq in labels for t in seq])
    out_tensor = model(input_ids=input_ids, position_ids=position_ids, cu_seqlens=cu, max_seqlen=6, labels=labels_t)

    torch.testing.assert_close(out_list.logits, out_tensor.logits, rtol=0, atol=0)
    torch.testing.assert_close(out_list.loss, out_tensor.loss, rtol=0, atol=0)


def test_label_ignore_positions_respected(golden_dir):
    """-100 labels and boundary drops: loss over valid targets only."""
    fx = _load(golden_dir, "model_mqa_rope_rmsnorm_gelu.pt")
    model = build_model(fx, "flash_attention_2", padding_free=True)
    model.eval()
    lists = [[5, 6, 7, 8], [3, 4, 5]]
    labels = [[-100, -100, 7, 8], [-100, 4, 5]]
    out = model(input_ids=lists, labels=labels)
    # manual: logits rows predicting labels[1:] per sequence minus drops
    logits = out.logits.float()
    import torch.nn.functional as F

    shift_logits = logits[:-1]
    flat_labels = torch.tensor([-100, -100, 7, 8, -100, 4, 5])
    shift_labels = flat_labels[1:].clone()
    shift_labels[torch.tensor([3]) - 0] = -100  # boundary: position cu[1]-1 = 3
    ref = F.cross_entropy(shift_logits, shift_labels)
    torch.testing.assert_close(out.loss, ref, rtol=1e-6, atol=1e-6)


def test_gradient_checkpointing_matches_plain(golden_dir):
    """Block activation checkpointing (reference gradient_checkpointing/
    block.py) must not change gradients — padding-free path, every block."""
    from dolomite_engine_amd.hf_models import apply_gradient_checkpointing

    fx = _load(golden_dir, "model_mqa_rope_rmsnorm_gelu.pt")

    def run(checkpointed):
        model = build_model(fx, "flash_attention_2", padding_free=True)
        if checkpointed:
            apply_gradient_checkpointing(model, "block", checkpoint_every=1)
        model.train()
        B, S = fx["input_ids"].shape
        out = model(
            input_ids=fx["input_ids"].reshape(-1),
            position_ids=torch.arange(S).repeat(B),
            cu_seqlens=torch.arange(0, B * S + 1, S, dtype=torch.int32),
            max_seqlen=S,
            labels=fx["labels"].reshape(-1),
        )
        out.loss.backward()
        return out.loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    loss_a, grads_a = run(False)
    loss_b, grads_b = run(True)
    torch.testing.assert_close(loss_a, loss_b, rtol=0, atol=0)
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        torch.testing.assert_close(grads_a[k], grads_b[k], rtol=1e-6, atol=1e-7, msg=lambda m: f"{k}: {m}")


def test_yarn_rope_tables_match_reference(golden_dir):
    """YaRNScaledRoPE cos/sin tables bit-match the recorded tables of the
    reference implementation (position_embedding/rope.py:59-142;
    oracle/gen_golden.py gen_yarn_rope) over scales and head dims."""
    import numpy

    from dolomite_engine_amd.hf_models.modeling import YaRNScaledRoPE

    ref = numpy.load(golden_dir / "yarn_rope.npz")
    for i, (head_dim, scale, orig) in enumerate([(64, 4.0, 2048), (128, 8.0, 4096), (80, 2.0, 1024), (64, 1.0, 2048)]):
        assert ref[f"case{i}_params"].tolist() == [head_dim, scale, orig]
        assert ref[f"case{i}_cos"].shape == (512, head_dim)
        ours = YaRNScaledRoPE(head_dim, 512, 10000.0, scale=scale, original_max_position_embeddings=orig)
        torch.testing.assert_close(ours.cos_cached, torch.from_numpy(ref[f"case{i}_cos"]), rtol=0, atol=0)
        torch.testing.assert_close(ours.sin_cached, torch.from_numpy(ref[f"case{i}_sin"]), rtol=0, atol=0)


def test_yarn_model_forward_runs():
    """A rope_scaling config builds YaRN tables and the padding-free CPU
    path runs end to end (previously raised NotImplementedError)."""
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM
    from dolomite_engine_amd.hf_models.modeling import YaRNScaledRoPE

    torch.manual_seed(0)
    cfg = GPTDolomiteConfig(
        vocab_size=128, n_positions=64, n_embd=64, n_layer=1, n_head=4,
        attention_head_type="mqa", n_inner=128, activation_function="gelu_pytorch_tanh",
        normalization_function="rmsnorm", position_embedding_type="rope",
        rope_scaling={"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 16},
        resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, tie_word_embeddings=False,
    )
    cfg._attn_implementation = "flash_attention_2"
    model = GPTDolomiteForCausalLM(cfg, use_padding_free_transformer=True)
    assert isinstance(model.transformer.rope, YaRNScaledRoPE)
    ids = torch.randint(0, 128, (32,))
    out = model(input_ids=ids, position_ids=torch.arange(32),
                cu_seqlens=torch.tensor([0, 32], dtype=torch.int32), max_seqlen=32, labels=ids)
    assert torch.isfinite(out.loss)


@pytest.mark.parametrize("impl", ["eager", "sdpa"])
def test_alibi_dense_matches_reference(golden_dir, impl):
    """position_embedding_type=alibi on the dense paths vs the recorded
    logits of the reference model run directly (base.py:261-287, alibi.py
    slopes; oracle/gen_golden.py gen_alibi), same weights and inputs."""
    fx = torch.load(golden_dir / "model_alibi_mqa.pt", weights_only=False)
    kw = fx["config"]
    assert kw["position_embedding_type"] == "alibi"

    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

    cfg = GPTDolomiteConfig(**kw)
    cfg._attn_implementation = impl
    model = GPTDolomiteForCausalLM(cfg)
    model.load_state_dict(fx[impl]["state_dict"])
    model.eval()

    ids = fx["input_ids"]
    mask = fx["attention_mask"]
    assert ids.shape == (2, 33) and int(mask[1, :7].sum()) == 0 and int(mask.sum()) == 2 * 33 - 7
    ref_full = fx[impl]["logits"]
    ref_mask = fx[impl]["logits_masked"]
    with torch.no_grad():
        our_full = model(input_ids=ids).logits
        our_mask = model(input_ids=ids, attention_mask=mask).logits
    torch.testing.assert_close(our_full, ref_full, rtol=1e-4, atol=1e-5)
    valid = mask.bool()
    torch.testing.assert_close(our_mask[valid], ref_mask[valid], rtol=1e-4, atol=1e-5)


def test_alibi_padding_free_raises():
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

    cfg = GPTDolomiteConfig(
        vocab_size=64, n_positions=32, n_embd=32, n_layer=1, n_head=4,
        attention_head_type="mqa", n_inner=64, position_embedding_type="alibi",
        normalization_function="rmsnorm", activation_function="gelu_pytorch_tanh",
        tie_word_embeddings=False,
    )
    cfg._attn_implementation = "flash_attention_2"
    with pytest.raises(AssertionError):
        GPTDolomiteForCausalLM(cfg, use_padding_free_transformer=True)
