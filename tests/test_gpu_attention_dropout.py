"""Attention dropout fused into the gfx950 flash kernels: the device keep
mask equals the Python restatement bit for bit, fwd/dkv/dq agree with the
fp32 CPU restatement under the same seed (flat and sharp softmax scales, so
a lane->index mis-mapping in any kernel is visible), determinism, the
unchanged p = 0 path, and a tiny model end to end."""

import math

import pytest
import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout, attention_dropout_keep_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------
# 1. device mask == Python mask
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [12345, (9 << 32) + 77])
def test_device_mask_equals_python_mask(p, seed):
    H, nq, nk = 3, 200, 200
    tq0, tk0 = 70000, 65500
    out = torch.zeros(H, nq, nk, dtype=torch.uint8, device="cuda")
    hip.check(
        hip.lib().dolomite_fa_dropout_mask_probe(hip.stream(), hip.ptr(out), seed, p, H, tq0, nq, tk0, nk),
        "fa_dropout_mask_probe",
    )
    torch.cuda.synchronize()
    ref = attention_dropout_keep_mask(seed, H, torch.arange(tq0, tq0 + nq), torch.arange(tk0, tk0 + nk), p)
    got = out.cpu().bool()
    assert int((got != ref).sum()) == 0


def test_invalid_p_drop_is_a_host_side_error_code():
    """p_drop outside [0, 1) returns 9013 before anything is launched."""
    lo = QKVLayout.make(4, 1, 16, "mqa")
    T = 8
    cu = torch.tensor([0, T], dtype=torch.int32, device="cuda")
    qkv = torch.zeros(T, lo.row_len, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(T, lo.H * lo.D, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(lo.H, T, dtype=torch.float32, device="cuda")
    delta = torch.zeros_like(lse)
    dqkv = torch.zeros_like(qkv)
    acc = torch.zeros(T, lo.H, lo.D, dtype=torch.float32, device="cuda")
    mask = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    for bad in (1.0, -0.25, float("nan")):
        assert hip.lib().dolomite_fa_dropout_mask_probe(hip.stream(), hip.ptr(mask), 1, bad, 1, 0, 4, 0, 4) == 9013
        assert hip.lib().dolomite_fa_varlen_fwd_dropout(
            hip.stream(), *lo.operands(qkv),
            hip.ptr(o), hip.ptr(lse), hip.ptr(cu), 1, T, T, lo.H, lo.Hkv, lo.D, lo.G,
            *lo.strides(), 0.25, hip.BF16, bad, 1,
        ) == 9013
        assert hip.lib().dolomite_fa_varlen_bwd_dropout(
            hip.stream(), *lo.operands(qkv),
            hip.ptr(o), hip.ptr(lse), hip.ptr(delta), hip.ptr(dqkv), hip.ptr(acc), hip.ptr(acc),
            hip.ptr(cu), 1, T, T, lo.H, lo.Hkv, lo.D, lo.G,
            *lo.strides(), lo.H * lo.D, 0.25, hip.BF16, bad, 1,
        ) == 9013
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. fwd + bwd vs the fp32 CPU restatement with the same seed
# ---------------------------------------------------------------------------

_SHAPES = [
    ("mqa", 8, 1, 80, [128, 64, 200]),
    ("gqa", 8, 2, 128, [65, 63]),
    ("gqa", 6, 2, 64, [100, 60]),
    ("mqa", 4, 1, 16, [10, 5]),
    ("mha", 4, 4, 64, [7, 0, 9]),
    ("mqa", 4, 1, 96, [300]),      # multi-tile: the maskless full_tile paths run with dropout
]
_CASES = [
    (shape, p)
    for i, shape in enumerate(_SHAPES)
    for p in ([0.1, 0.5] if i in (0, len(_SHAPES) - 1) else [0.1])
]


@pytest.mark.parametrize("sharp", [1.0, 8.0], ids=["flat", "sharp"])
@pytest.mark.parametrize("shape,p", _CASES, ids=[f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-{s[4]}-p{p}" for s, p in _CASES])
def test_varlen_attention_dropout_fwd_bwd_vs_cpu_restatement(shape, p, sharp):
    """Tolerances of test_varlen_attention_fwd_bwd_vs_oracle (rtol 2e-2 for
    o, 3e-2 for dq/dk/dv) with atol multiplied by 1/(1-p): kept
    probabilities are scaled by exactly that factor."""
    head_type, H, Hkv, D, lens = shape
    g = torch.Generator().manual_seed(5)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    scale = sharp / math.sqrt(D)
    seed = (0x5EED << 32) + 1000 * D + H
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)

    qkv_g = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(qkv_g, cu.cuda(), max(lens), lo, scale, dropout_p=p, seed=seed)
    o.backward(do.cuda())
    torch.cuda.synchronize()

    qkv_c = qkv.float().requires_grad_(True)
    oc = Fx.varlen_attention(qkv_c, cu, max(lens), lo, scale, dropout_p=p, seed=seed)
    oc.backward(do.float())

    rp = 1.0 / (1.0 - p)
    dq_g, dk_g, dv_g = lo.unpack_cpu(qkv_g.grad.cpu())
    dq_c, dk_c, dv_c = lo.unpack_cpu(qkv_c.grad)
    got = {"o": o.detach().cpu().float(), "dq": dq_g.float(), "dk": dk_g.float(), "dv": dv_g.float()}
    ref = {"o": oc.detach(), "dq": dq_c, "dk": dk_c, "dv": dv_c}
    for name in got:
        err = (got[name] - ref[name]).abs()
        print(f"{name}: max|err| {float(err.max()):.4e}  max|ref| {float(ref[name].abs().max()):.4e}")
    torch.testing.assert_close(got["o"], ref["o"], rtol=2e-2, atol=2e-2 * rp)
    for name in ("dq", "dk", "dv"):
        torch.testing.assert_close(got[name], ref[name], rtol=3e-2, atol=3e-2 * rp, msg=lambda m: f"{name}: {m}")


# ---------------------------------------------------------------------------
# 3. determinism, 4. the p = 0 path
# ---------------------------------------------------------------------------


def _gqa_inputs():
    lo = QKVLayout.make(8, 2, 128, "gqa")
    cu = torch.tensor([0, 300, 428], dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(17)
    qkv = (torch.randn(428, lo.row_len, generator=g) * 0.5).to(torch.bfloat16).cuda()
    do = (torch.randn(428, 8 * 128, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return lo, cu, qkv, do


def _run(lo, cu, qkv, do, **kw):
    x = qkv.clone().requires_grad_(True)
    o = Fx.varlen_attention(x, cu, 300, lo, 1.0 / math.sqrt(lo.D), **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), x.grad


def test_dropout_is_deterministic_per_seed():
    lo, cu, qkv, do = _gqa_inputs()
    o1, g1 = _run(lo, cu, qkv, do, dropout_p=0.1, seed=(3 << 32) + 41)
    o2, g2 = _run(lo, cu, qkv, do, dropout_p=0.1, seed=(3 << 32) + 41)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    o3, _ = _run(lo, cu, qkv, do, dropout_p=0.1, seed=(3 << 32) + 42)
    assert not torch.equal(o1, o3)


def test_p0_through_new_signature_is_bitwise_unchanged():
    lo, cu, qkv, do = _gqa_inputs()
    o_old, g_old = _run(lo, cu, qkv, do)
    o_new, g_new = _run(lo, cu, qkv, do, dropout_p=0.0, seed=99)
    assert torch.equal(o_old, o_new) and torch.equal(g_old, g_new)


# ---------------------------------------------------------------------------
# 5. tiny bf16 padding-free model, one fwd + bwd
# ---------------------------------------------------------------------------


def test_tiny_model_with_attention_dropout_matches_cpu_fp32_copy():
    """Seeds come from torch's CPU generator, so the bf16 GPU model and its
    fp32 CPU copy see the same masks under the same torch.manual_seed; loss
    at the tolerance test_gpu_model.py uses for its tiny-model losses."""
    from tests.test_attention_dropout_cpu import _batch, _tiny_model

    gpu = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.1).to(torch.bfloat16)
    cpu = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.1)
    cpu.load_state_dict({k: v.float() for k, v in gpu.state_dict().items()})
    plain = _tiny_model(resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    plain.load_state_dict(cpu.state_dict())
    gpu = gpu.cuda().train()
    cpu.train()
    plain.train()
    batch = _batch()

    torch.manual_seed(77)
    out_g = gpu(**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})
    out_g.loss.backward()
    torch.cuda.synchronize()
    torch.manual_seed(77)
    out_c = cpu(**batch)
    out_p = plain(**batch)

    assert all(torch.isfinite(p.grad).all() for p in gpu.parameters() if p.grad is not None)
    lg, lc, lp = (float(x.loss.detach()) for x in (out_g, out_c, out_p))
    print(f"gpu loss {lg:.6f}  cpu loss {lc:.6f}  undropped {lp:.6f}")
    torch.testing.assert_close(out_g.loss.detach().float().cpu(), out_c.loss.detach(), rtol=1e-3, atol=1e-4)
    # same masks, not merely some masks: an independent mask draw would land
    # about as far from the CPU loss as dropping at all moves it
    assert abs(lg - lc) < 0.5 * abs(lc - lp)
    assert hip._lib is not None
