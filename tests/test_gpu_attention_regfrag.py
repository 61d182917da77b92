"""Register-resident P / dS in the gfx950 flash kernels: the forward and dq
kernels compute S^T = K*Q^T, keep one q row per lane and feed the packed
P^T / dS^T straight into the next MFMA, whose other operand (V^T / K^T) is a
transpose read of the row-major image in a PERMUTED key order. These tests
pin what that layout can get wrong:

- the key order of the second contraction (one-hot softmax that must return
  exactly one V row, and full fwd+bwd parity at sharp, flat and mild scales);
- the cross-lane-group row reductions and the lane that writes each LSE;
- the 8-byte transposed epilogue stores (no pad column, no row >= L);
- the dropout mask's lane -> (q, k) mapping (1 row word, 16 column words).
"""

import functools
import math

import pytest
import torch

import oracle
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def _pack(lo: QKVLayout, q, k, v):
    """Inverse of QKVLayout.unpack_cpu: q (T,H,D), k/v (T,Hkv,D) -> (T,row_len)."""
    T = q.shape[0]
    H, Hkv, D, G = lo.H, lo.Hkv, lo.D, lo.G
    if G == 1:
        return torch.cat([q, k, v], dim=-1).reshape(T, lo.row_len)
    if Hkv > 1:
        return torch.cat([q.reshape(T, Hkv, G * D), k, v], dim=-1).reshape(T, lo.row_len)
    return torch.cat([q.reshape(T, H * D), k.reshape(T, D), v.reshape(T, D)], dim=-1)


def _oracle_fwd_bwd(lo, qkv, cu, scale, do):
    q, k, v = lo.unpack_cpu(qkv)
    qc, kc, vc = (x.float().requires_grad_(True) for x in (q, k, v))
    oc = oracle.attention_varlen_ref(qc, kc, vc, cu, scale)
    oc.backward(do.float().reshape(oc.shape))
    return oc.detach(), qc.grad, kc.grad, vc.grad


# ---------------------------------------------------------------------------
# 1. key order of the second contraction
# ---------------------------------------------------------------------------

_KEY_LENS = [33, 65, 129, 200]  # both 32-key chunks, both halves, 2nd tile, ragged tails
_KEY_SHAPES = [("mha", 2, 2, 64), ("mqa", 4, 1, 80), ("gqa", 4, 2, 128)]  # DPAD 64 / 96 / 128


def _target(i: int) -> int:
    """Fixed key t(i) <= i that q row i points at."""
    return (29 * i + 7) % (i + 1)


@functools.lru_cache(maxsize=None)
def _key_order_case(head_type, H, Hkv, D, c):
    """K rows are +-1 vectors, q_i = c * K[t(i)], V[key][d] a small-integer
    pattern that is exact in bf16 and asymmetric in key and d. Returns the
    inputs, the target map and the fp32 oracle's fwd+bwd (computed once)."""
    g = torch.Generator().manual_seed(1234 + D)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = _cu(_KEY_LENS)
    T = int(cu[-1])
    k = (torch.randint(0, 2, (T, Hkv, D), generator=g) * 2 - 1).float()
    tgt = torch.empty(T, dtype=torch.int64)
    for s, L in zip(cu[:-1].tolist(), _KEY_LENS):
        for i in range(L):
            tgt[s + i] = s + _target(i)
    G = H // Hkv
    q = c * k[tgt][:, torch.arange(H) // G, :]                     # (T, H, D)
    key = torch.arange(T)[:, None, None]
    d = torch.arange(D)[None, None, :]
    j = torch.arange(Hkv)[None, :, None]
    v = ((7 * key + 3 * d + 5 * j) % 17 - 8).float()
    qkv = _pack(lo, q, k, v).to(torch.bfloat16)
    assert torch.equal(qkv.float(), _pack(lo, q, k, v))            # exact in bf16
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    return lo, cu, qkv, do, scale, tgt, v, _oracle_fwd_bwd(lo, qkv, cu, scale, do)


def test_targets_visit_every_key_slot():
    """The one-hot targets of the longest sequence hit every residue mod 64,
    i.e. every (chunk, half, lane group, register) slot of a key tile."""
    assert {_target(i) % 64 for i in range(max(_KEY_LENS))} == set(range(64))
    assert all(_target(i) <= i for i in range(max(_KEY_LENS)))


@pytest.mark.parametrize("c", [4.0, 0.0, 0.125], ids=["onehot", "flat", "mild"])
@pytest.mark.parametrize("head_type,H,Hkv,D", _KEY_SHAPES)
def test_key_order_fwd_bwd(head_type, H, Hkv, D, c):
    """c = 4: the score gap between the target key and any other is
    c*scale*(D - K_t.K_j) >= 15 here, so softmax is one-hot to far below
    bf16 and O[i] must equal V[t(i)] — a slot<->row mismatch in the V^T
    ladder returns another key's row, off by >= 1 on most elements.
    c = 0 (flat) makes dV carry every causal (q, key) pair and dQ every
    dS*K product; c = 0.125 (mild) adds a nonzero dK. All three against the
    fp32 oracle at the tolerances of test_varlen_attention_fwd_bwd_vs_oracle."""
    lo, cu, qkv, do, scale, tgt, v, (o_ref, dq_ref, dk_ref, dv_ref) = _key_order_case(head_type, H, Hkv, D, c)
    T = qkv.shape[0]
    x = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(x, cu.cuda(), max(_KEY_LENS), lo, scale)
    o.backward(do.cuda())
    torch.cuda.synchronize()
    o_g = o.detach().cpu().float().reshape(T, H, D)
    dq_g, dk_g, dv_g = (t.float() for t in lo.unpack_cpu(x.grad.cpu()))

    if c == 4.0:
        expect = v[tgt][:, torch.arange(H) // (H // Hkv), :]       # V[t(i)] per q head
        torch.testing.assert_close(o_ref, expect, rtol=0, atol=1e-3)   # the input does what it claims
        err = (o_g - expect).abs()
        print(f"one-hot: max|O - V[t]| {float(err.max()):.3e}, rows off {int((err.amax((1, 2)) > 2e-2).sum())}")
        torch.testing.assert_close(o_g, expect, rtol=2e-2, atol=2e-2)
    for name, got, ref, tol in (("o", o_g, o_ref, 2e-2), ("dq", dq_g, dq_ref, 3e-2),
                                ("dk", dk_g, dk_ref, 3e-2), ("dv", dv_g, dv_ref, 3e-2)):
        print(f"{name}: max|err| {float((got - ref).abs().max()):.3e}  max|ref| {float(ref.abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=tol, atol=tol, msg=lambda m, n=name: f"{n}: {m}")


# ---------------------------------------------------------------------------
# 2. LSE: cross-lane-group reductions, one value per q row from the right lane
# ---------------------------------------------------------------------------


def _fwd_abi(lo, qkv, cu, max_len, T, scale, o, lse, t_stride=None):
    hip.check(
        hip.lib().dolomite_fa_varlen_fwd(
            hip.stream(), *lo.operands(qkv),
            hip.ptr(o), hip.ptr(lse), hip.ptr(cu), cu.numel() - 1, max_len, T,
            lo.H, lo.Hkv, lo.D, lo.G, *lo.strides(t_stride), scale, hip.BF16,
        ),
        "fa_varlen_fwd",
    )


@pytest.mark.parametrize("head_type,H,Hkv,D", _KEY_SHAPES)
def test_lse_matches_fp32_logsumexp(head_type, H, Hkv, D):
    lens = _KEY_LENS + [1, 0]
    g = torch.Generator().manual_seed(77 + D)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = _cu(lens)
    T = int(cu[-1])
    scale = 1.0 / math.sqrt(D)
    qkv = (torch.randn(T, lo.row_len, generator=g)).to(torch.bfloat16)

    o = torch.empty(T, H * D, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((H, T), float("nan"), dtype=torch.float32, device="cuda")
    _fwd_abi(lo, qkv.cuda(), cu.cuda(), max(lens), T, scale, o, lse)
    torch.cuda.synchronize()

    q, k, _ = lo.unpack_cpu(qkv)
    ref = torch.empty(H, T)
    for s, L in zip(cu[:-1].tolist(), lens):
        if L == 0:
            continue
        mask = torch.ones(L, L, dtype=torch.bool).tril()
        for h in range(H):
            sc = (q[s:s + L, h].float() @ k[s:s + L, h // (H // Hkv)].float().T) * scale
            ref[h, s:s + L] = torch.logsumexp(sc.masked_fill(~mask, float("-inf")), dim=-1)
    got = lse.cpu()
    print(f"lse: max|err| {float((got - ref).abs().max()):.3e}")
    torch.testing.assert_close(got, ref, rtol=0, atol=2e-3)


# ---------------------------------------------------------------------------
# 3. store shape: the 8-byte transposed stores write no pad column, no row >= L
# ---------------------------------------------------------------------------

_SENT = -1024.0  # exact in bf16 and far outside every result


@pytest.mark.parametrize(
    "head_type,H,Hkv,D,lens",
    [
        ("gqa", 4, 2, 48, [77, 50]),   # DPAD 64: 16-col pad band, 4 store groups wide
        ("mqa", 4, 1, 16, [10, 5]),    # DPAD 32
        ("mha", 1, 1, 48, [70]),       # one head: row t's pad columns would land in row t+1
    ],
)
def test_epilogue_stores_stay_inside_rows_and_columns(head_type, H, Hkv, D, lens):
    """qkv / dqkv rows carry a sentinel band past row_len (the ABI takes the
    token stride) and sentinel rows past T; o and lse carry sentinel tails.
    The backward ABI is called without the finalize pass first, so the K/V
    columns of dqkv must still hold the sentinel after the dq kernel."""
    BAND, TAIL = 16, 4
    g = torch.Generator().manual_seed(9 + D)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = _cu(lens)
    T = int(cu[-1])
    ts = lo.row_len + BAND
    scale = 1.0 / math.sqrt(D)
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    o_ref, dq_ref, dk_ref, dv_ref = _oracle_fwd_bwd(lo, qkv, cu, scale, do)

    buf = torch.full((T + TAIL, ts), _SENT, dtype=torch.bfloat16)
    buf[:T, : lo.row_len] = qkv
    buf = buf.cuda()
    o = torch.full((T + TAIL, H * D), _SENT, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((H * T + TAIL,), _SENT, dtype=torch.float32, device="cuda")
    cu_g = cu.cuda()
    _fwd_abi(lo, buf, cu_g, max(lens), T, scale, o, lse, t_stride=ts)
    torch.cuda.synchronize()
    assert torch.all(o[T:] == _SENT) and torch.all(lse[H * T:] == _SENT)
    torch.testing.assert_close(o[:T].cpu().float().reshape(T, H, D), o_ref, rtol=2e-2, atol=2e-2)

    do_g = do.cuda()
    delta = torch.empty(H, T, dtype=torch.float32, device="cuda")
    hip.check(
        hip.lib().dolomite_fa_bwd_preprocess(
            hip.stream(), hip.ptr(o), hip.ptr(do_g), hip.ptr(delta), T, H, D, H * D, H * D, hip.BF16),
        "fa_bwd_preprocess",
    )
    dqkv = torch.full((T + TAIL, ts), _SENT, dtype=torch.bfloat16, device="cuda")
    dk_acc = torch.empty(T, H, D, dtype=torch.float32, device="cuda")
    dv_acc = torch.empty(T, H, D, dtype=torch.float32, device="cuda")
    hip.check(
        hip.lib().dolomite_fa_varlen_bwd(
            hip.stream(), *lo.operands(buf),
            hip.ptr(do_g), hip.ptr(lse), hip.ptr(delta), hip.ptr(dqkv), hip.ptr(dk_acc), hip.ptr(dv_acc),
            hip.ptr(cu_g), len(lens), max(lens), T, H, Hkv, D, lo.G,
            *lo.strides(ts), H * D, scale, hip.BF16,
        ),
        "fa_varlen_bwd",
    )
    torch.cuda.synchronize()
    after_dq = dqkv.cpu()
    assert torch.all(after_dq[T:] == _SENT) and torch.all(after_dq[:, lo.row_len:] == _SENT)
    # before finalize only the q columns may have been written
    is_q = _pack(lo, torch.ones(1, H, D), torch.zeros(1, Hkv, D), torch.zeros(1, Hkv, D))[0] == 1
    assert torch.all(after_dq[:T, : lo.row_len][:, ~is_q] == _SENT)

    hip.check(
        hip.lib().dolomite_fa_grad_finalize(
            hip.stream(), hip.ptr(dk_acc), hip.ptr(dv_acc), hip.ptr(dqkv), T, Hkv, D, lo.G, ts,
            lo.k_off, lo.kv_hstride, lo.v_off, hip.BF16),
        "fa_grad_finalize",
    )
    torch.cuda.synchronize()
    final = dqkv.cpu()
    assert torch.all(final[T:] == _SENT) and torch.all(final[:, lo.row_len:] == _SENT)
    dq_g, dk_g, dv_g = lo.unpack_cpu(final[:T, : lo.row_len].contiguous())
    torch.testing.assert_close(dq_g.float(), dq_ref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk_g.float(), dk_ref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv_g.float(), dv_ref, rtol=3e-2, atol=3e-2)


# ---------------------------------------------------------------------------
# 4. dropout: 1 row word + 16 column words per lane, at a tile edge
# ---------------------------------------------------------------------------


def test_dropout_mask_mapping_sharp_scale():
    """p = 0.3 at lens [129, 65] (a second q tile, a one-key tail tile),
    D = 80, softmax sharpened 8x so each row leans on a few keys and a
    lane -> (q, k) mis-mapping of the mask moves o and the gradients by
    far more than the tolerance. Reference: the fp32 CPU restatement built
    on attention_dropout_keep_mask with the same seed; tolerances of
    test_varlen_attention_dropout_fwd_bwd_vs_cpu_restatement."""
    H, D, p, lens = 4, 80, 0.3, [129, 65]
    lo = QKVLayout.make(H, 1, D, "mqa")
    g = torch.Generator().manual_seed(31)
    cu = _cu(lens)
    T = int(cu[-1])
    scale = 8.0 / math.sqrt(D)
    seed = (0xD0 << 32) + 4242
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)

    x = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(x, cu.cuda(), max(lens), lo, scale, dropout_p=p, seed=seed)
    o.backward(do.cuda())
    torch.cuda.synchronize()
    xc = qkv.float().requires_grad_(True)
    oc = Fx.varlen_attention(xc, cu, max(lens), lo, scale, dropout_p=p, seed=seed)
    oc.backward(do.float())

    rp = 1.0 / (1.0 - p)
    got = dict(zip(("dq", "dk", "dv"), (t.float() for t in lo.unpack_cpu(x.grad.cpu()))))
    ref = dict(zip(("dq", "dk", "dv"), lo.unpack_cpu(xc.grad)))
    got["o"], ref["o"] = o.detach().cpu().float(), oc.detach()
    for name in ("o", "dq", "dk", "dv"):
        print(f"{name}: max|err| {float((got[name] - ref[name]).abs().max()):.3e}")
    torch.testing.assert_close(got["o"], ref["o"], rtol=2e-2, atol=2e-2 * rp)
    for name in ("dq", "dk", "dv"):
        torch.testing.assert_close(got[name], ref[name], rtol=3e-2, atol=3e-2 * rp, msg=lambda m, n=name: f"{n}: {m}")
