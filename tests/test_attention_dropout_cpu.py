"""Attention dropout on the padding-free path, CPU side: the counter-based
keep mask's statistics, the CPU restatement of the dropped attention, the
model plumbing (default dropout fields train; eval unchanged; checkpoint
recompute sees the same masks), seed draws under RNG save/restore, and the
C-ABI surface."""

import copy
import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops.functional import QKVLayout, attention_dropout_keep_mask

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dolomite_hip.h"
NEW_SYMBOLS = [
    "dolomite_fa_varlen_fwd_dropout",
    "dolomite_fa_varlen_bwd_dropout",
    "dolomite_fa_dropout_mask_probe",
]


# ---------------------------------------------------------------------------
# 1. mask statistics
# ---------------------------------------------------------------------------


def _corr(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / (a.norm() * b.norm()))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed,t0", [(20240607, 0), ((911 << 32) + 5, 65536 - 100)])
def test_keep_mask_statistics(p, seed, t0):
    """H=4, 256x256 box: keep rate within 5 sigma of 1-p, and the mask is
    uncorrelated (|r| < 5/sqrt(N)) with its one-row, one-column, one-head,
    seed+1 and seed^(1<<32) shifted copies. The second case straddles
    T = 65536, where a naive t_q*c ^ t_k pre-mix makes rows share masks."""
    H, n = 4, 256
    N = H * n * n
    assert N == 262144
    tq = torch.arange(t0, t0 + n + 1)
    tk = torch.arange(t0, t0 + n + 1)
    big = attention_dropout_keep_mask(seed, H + 1, tq, tk, p)
    m = big[:H, :n, :n]

    sigma = math.sqrt(p * (1 - p) / N)
    rate = float(m.double().mean())
    print(f"keep rate {rate:.6f} (expect {1 - p}, sigma {sigma:.2e})")
    assert abs(rate - (1 - p)) < 5 * sigma

    shifted = {
        "row": big[:H, 1:, :n],
        "col": big[:H, :n, 1:],
        "head": big[1:, :n, :n],
        "seed+1": attention_dropout_keep_mask(seed + 1, H, tq[:n], tk[:n], p),
        "seed^(1<<32)": attention_dropout_keep_mask(seed ^ (1 << 32), H, tq[:n], tk[:n], p),
    }
    bound = 5 / math.sqrt(N)
    for name, other in shifted.items():
        r = _corr(m, other)
        print(f"corr[{name}] = {r:+.5f} (bound {bound:.5f})")
        assert abs(r) < bound, name


def test_keep_mask_p0_keeps_all_and_is_pure():
    tq = torch.arange(1000, 1100)
    tk = torch.arange(900, 1050)
    assert attention_dropout_keep_mask(77, 3, tq, tk, 0.0).all()
    a = attention_dropout_keep_mask((5 << 32) + 1, 3, tq, tk, 0.3)
    b = attention_dropout_keep_mask((5 << 32) + 1, 3, tq, tk, 0.3)
    assert a.shape == (3, 100, 150) and a.dtype == torch.bool
    assert torch.equal(a, b)
    # global indices: a sub-box of the mask is the mask of the sub-box
    sub = attention_dropout_keep_mask((5 << 32) + 1, 3, tq[10:20], tk[100:], 0.3)
    assert torch.equal(a[:, 10:20, 100:], sub)


# ---------------------------------------------------------------------------
# 2. CPU varlen_attention with dropout vs an explicit fp32 computation
# ---------------------------------------------------------------------------


def _explicit_dropped_attention(q, k, v, cu, scale, G, seed, p):
    """softmax(QK^T) * mask * 1/(1-p) @ V per sequence and head, fp32."""
    T, H, D = q.shape
    rp = 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32)))
    out = torch.zeros(T, H, D)
    cul = cu.tolist()
    rows = []
    for s, e in zip(cul[:-1], cul[1:]):
        if e == s:
            continue
        L = e - s
        tok = torch.arange(s, e)
        keep = attention_dropout_keep_mask(seed, H, tok, tok, p)
        causal = torch.ones(L, L, dtype=torch.bool).tril()
        heads = []
        for h in range(H):
            sc = (q[s:e, h] @ k[s:e, h // G].T) * scale
            pr = torch.softmax(sc.masked_fill(~causal, float("-inf")), dim=-1)
            heads.append((pr * keep[h] * rp) @ v[s:e, h // G])
        rows.append(torch.stack(heads, dim=1))
    return torch.cat(rows, dim=0)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_cpu_varlen_attention_dropout_matches_explicit(p):
    H, Hkv, D = 6, 2, 16  # gqa, G = 3
    lens = [7, 0, 9, 33]
    lo = QKVLayout.make(H, Hkv, D, "gqa")
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, lo.row_len, generator=g)
    do = torch.randn(T, H * D, generator=g)
    scale = 3.0 / math.sqrt(D)
    seed = (123 << 32) + 456

    x = qkv.clone().requires_grad_(True)
    o = Fx.varlen_attention(x, cu, max(lens), lo, scale, dropout_p=p, seed=seed)
    o.backward(do)

    y = qkv.clone().requires_grad_(True)
    q, k, v = lo.unpack_cpu(y)
    ref = _explicit_dropped_attention(q, k, v, cu, scale, lo.G, seed, p).reshape(T, H * D)
    ref.backward(do)

    torch.testing.assert_close(o.detach(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad, y.grad, rtol=1e-5, atol=1e-5)
    # dropout really happened: differs from the undropped op
    o0 = Fx.varlen_attention(qkv, cu, max(lens), lo, scale)
    assert not torch.allclose(o.detach(), o0, rtol=1e-3, atol=1e-3)


def test_varlen_attention_rejects_invalid_p():
    lo = QKVLayout.make(2, 1, 8, "mqa")
    cu = torch.tensor([0, 4], dtype=torch.int32)
    qkv = torch.zeros(4, lo.row_len)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Fx.varlen_attention(qkv, cu, 4, lo, 1.0, dropout_p=bad)


# ---------------------------------------------------------------------------
# 3. model
# ---------------------------------------------------------------------------


def _tiny_model(**over):
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

    kw = dict(
        vocab_size=128, n_positions=64, n_embd=64, n_layer=2, n_head=4,
        attention_head_type="mqa", n_inner=128, activation_function="gelu_pytorch_tanh",
        normalization_function="rmsnorm", position_embedding_type="rope",
        tie_word_embeddings=False,
    )
    kw.update(over)
    cfg = GPTDolomiteConfig(**kw)  # dropout fields left at their defaults unless overridden
    cfg._attn_implementation = "flash_attention_2"
    torch.manual_seed(0)
    return GPTDolomiteForCausalLM(cfg, use_padding_free_transformer=True)


def _batch():
    g = torch.Generator().manual_seed(11)
    lens = [20, 13, 31]
    T = sum(lens)
    ids = torch.randint(0, 128, (T,), generator=g)
    pos = torch.cat([torch.arange(n) for n in lens])
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    return dict(input_ids=ids, position_ids=pos, cu_seqlens=cu, max_seqlen=max(lens), labels=ids)


def _train_step(model, seed):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = model(**_batch())
    out.loss.backward()
    return out.loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_default_config_trains_on_padding_free_path():
    model = _tiny_model()
    assert model.config.attn_pdrop == 0.1 and model.config.resid_pdrop == 0.1 and model.config.embd_pdrop == 0.1
    model.train()
    loss_a, grads_a = _train_step(model, 5)
    assert torch.isfinite(loss_a)
    assert grads_a and all(torch.isfinite(g).all() for g in grads_a.values())
    loss_b, grads_b = _train_step(model, 5)
    assert torch.equal(loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
    loss_c, _ = _train_step(model, 6)
    assert not torch.equal(loss_a, loss_c)


def test_attention_dropout_alone_changes_training_loss_not_eval():
    drop = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.1)
    plain = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    plain.load_state_dict(drop.state_dict())
    drop.eval()
    plain.eval()
    with torch.no_grad():
        a = drop(**_batch())
        b = plain(**_batch())
    assert torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss)
    drop.train()
    plain.train()
    loss_d, _ = _train_step(drop, 5)
    loss_p, _ = _train_step(plain, 5)
    assert not torch.equal(loss_d, loss_p)


def test_block_checkpointing_recompute_sees_same_masks():
    from dolomite_engine_amd.hf_models import apply_gradient_checkpointing

    base = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.1)
    ckpt = copy.deepcopy(base)
    apply_gradient_checkpointing(ckpt, "block", checkpoint_every=1)
    base.train()
    ckpt.train()
    loss_a, grads_a = _train_step(base, 9)
    loss_b, grads_b = _train_step(ckpt, 9)
    assert torch.equal(loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


# ---------------------------------------------------------------------------
# 4. seed draws follow torch's CPU RNG state
# ---------------------------------------------------------------------------


def test_seed_draws_restore_with_rng_state():
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    first = [Fx.draw_attention_dropout_seed(), Fx.draw_attention_dropout_seed()]
    torch.set_rng_state(state)
    second = [Fx.draw_attention_dropout_seed(), Fx.draw_attention_dropout_seed()]
    assert first == second
    assert first[0] != first[1]  # successive layers get successive draws
    assert all(isinstance(s, int) and 0 <= s < 2**63 for s in first)


def test_p0_call_leaves_rng_stream_untouched():
    lo = QKVLayout.make(2, 1, 8, "mqa")
    cu = torch.tensor([0, 4], dtype=torch.int32)
    qkv = torch.randn(4, lo.row_len)
    state = torch.get_rng_state()
    Fx.varlen_attention(qkv, cu, 4, lo, 1.0, dropout_p=0.0)
    assert torch.equal(torch.get_rng_state(), state)


# ---------------------------------------------------------------------------
# 5. ABI
# ---------------------------------------------------------------------------


def test_header_declares_dropout_symbols():
    declared = set(re.findall(r"^int (dolomite_\w+)\(", HEADER.read_text(), flags=re.M))
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym


def test_library_exports_dropout_symbols():
    from dolomite_engine_amd.csrc.build import SO_PATH, build
    from dolomite_engine_amd.ops import hip

    so = SO_PATH if SO_PATH.exists() else build()
    lib = ctypes.CDLL(str(so))
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} not exported by {so.name}"
        assert sym in hip._SIGNATURES, sym
    fn = lib.dolomite_hip_abi_version
    fn.restype = ctypes.c_int32
    assert fn() == 2
