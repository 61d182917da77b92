"""GPU parity tests: HIP kernels vs the oracle / CPU restatement, on a real
MI355X. Every test here calls through the C-ABI (include/dolomite_hip.h).

Tolerances follow the reference's own suite for bf16
(gpt_dolomite_test.py:128-136: rtol/atol 5e-3 bf16) and are tightened where
our kernels accumulate in fp32.
"""

import math

import pytest
import torch

import oracle
from dolomite_engine_amd.ops import QKVLayout, hip_extension_available
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hip_extension_available(), "libdolomite_hip.so missing — build() must run first"


def test_mfma_fragment_layout():
    """Empirical check of the assumed mfma_f32_16x16x32_bf16 A/B/C lane maps
    (attention.hip header). If this fails, every MFMA kernel is wrong."""
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(16, 32, generator=g) * 0.5).to(torch.bfloat16)
    B = (torch.randn(32, 16, generator=g) * 0.5).to(torch.bfloat16)
    # asymmetric inputs (guide §3: symmetric B hides transposed C writes)
    Ad, Bd = A.cuda(), B.cuda()
    Cd = torch.zeros(16, 16, dtype=torch.float32, device="cuda")
    hip.check(hip.lib().dolomite_mfma_probe(hip.stream(), hip.ptr(Ad), hip.ptr(Bd), hip.ptr(Cd)), "probe")
    torch.cuda.synchronize()
    ref = A.float() @ B.float()
    torch.testing.assert_close(Cd.cpu(), ref, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(33, 96), (128, 2560), (257, 4096)])
def test_rmsnorm_fwd_bwd(dtype, shape):
    g = torch.Generator().manual_seed(1)
    T, H = shape
    x = torch.randn(T, H, generator=g).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H, generator=g) * 0.1 + 1.0).to(dtype).cuda().requires_grad_(True)
    y, s = Fx.fused_rmsnorm(x, w, 1e-6)
    dy = torch.randn(T, H, generator=g).to(dtype).cuda()
    y.backward(dy)

    xc = x.detach().cpu().requires_grad_(True)
    wc = w.detach().cpu().requires_grad_(True)
    yc = oracle.rmsnorm_ref(xc, wc, 1e-6)
    yc.backward(dy.cpu())

    tol = dict(rtol=0, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(y.detach().cpu(), yc.detach(), **tol)
    torch.testing.assert_close(x.grad.cpu(), xc.grad, **tol)
    wtol = dict(rtol=1e-4, atol=1e-4 * T / 30) if dtype == torch.float32 else dict(rtol=1e-2, atol=3e-1)
    torch.testing.assert_close(w.grad.cpu().float(), wc.grad.float(), **wtol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rmsnorm_residual_fused(dtype):
    g = torch.Generator().manual_seed(2)
    T, H = 64, 512
    x = torch.randn(T, H, generator=g).to(dtype).cuda().requires_grad_(True)
    r = torch.randn(T, H, generator=g).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H, generator=g) * 0.1 + 1.0).to(dtype).cuda().requires_grad_(True)
    y, s = Fx.fused_rmsnorm(x, w, 1e-5, residual=r)
    (y.float().pow(2).sum() + s.float().sum()).backward()

    xc = x.detach().cpu().requires_grad_(True)
    rc = r.detach().cpu().requires_grad_(True)
    wc = w.detach().cpu().requires_grad_(True)
    sc = xc + rc
    yc = oracle.rmsnorm_ref(sc, wc, 1e-5)
    (yc.float().pow(2).sum() + sc.float().sum()).backward()

    # bf16: the kernel's fp32 dot-reduction order differs from torch's —
    # isolated one-ulp flips are expected (observed 10/32768 at 0.03)
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(y.detach().cpu(), yc.detach(), **tol)
    torch.testing.assert_close(s.detach().cpu(), sc.detach(), **tol)
    torch.testing.assert_close(x.grad.cpu(), xc.grad, **tol)
    torch.testing.assert_close(r.grad.cpu(), rc.grad, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_fwd_bwd(dtype):
    g = torch.Generator().manual_seed(3)
    T, H = 96, 768
    x = torch.randn(T, H, generator=g).to(dtype).cuda().requires_grad_(True)
    w = (torch.randn(H, generator=g) * 0.1 + 1.0).to(dtype).cuda().requires_grad_(True)
    b = (torch.randn(H, generator=g) * 0.1).to(dtype).cuda().requires_grad_(True)
    y, _ = Fx.fused_layernorm(x, w, b, 1e-5)
    dy = torch.randn(T, H, generator=g).to(dtype).cuda()
    y.backward(dy)

    xc = x.detach().cpu().float().requires_grad_(True)
    wc = w.detach().cpu().float().requires_grad_(True)
    bc = b.detach().cpu().float().requires_grad_(True)
    yc = torch.nn.functional.layer_norm(xc, (H,), wc, bc, 1e-5)
    yc.backward(dy.cpu().float())

    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(y.detach().cpu().float(), yc.detach(), **tol)
    torch.testing.assert_close(x.grad.cpu().float(), xc.grad, **tol)
    wtol = dict(rtol=1e-3, atol=1e-3) if dtype == torch.float32 else dict(rtol=1e-2, atol=2e-1)
    torch.testing.assert_close(w.grad.cpu().float(), wc.grad, **wtol)
    torch.testing.assert_close(b.grad.cpu().float(), bc.grad, **wtol)


@pytest.mark.parametrize("head_type,H,Hkv,D", [("mqa", 8, 1, 80), ("gqa", 8, 2, 128), ("mha", 4, 4, 64)])
def test_rope_packed_roundtrip_and_oracle(head_type, H, Hkv, D):
    g = torch.Generator().manual_seed(4)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    T = 48
    cos, sin = oracle.rope_cos_sin_ref(D, 64, 10000.0)
    pos = torch.arange(T) % 64
    cos_g = cos[pos].contiguous().cuda()
    sin_g = sin[pos].contiguous().cuda()
    qkv = torch.randn(T, lo.row_len, generator=g).to(torch.bfloat16)

    base = qkv.cuda().requires_grad_(True)
    qkv_g = base.clone()  # non-leaf: the Function rotates in place (mark_dirty)
    out = Fx.RoPEPackedQKV.apply(qkv_g, cos_g, sin_g, lo)
    torch.cuda.synchronize()

    # oracle comparison head by head
    out_cpu = out.detach().cpu()
    qf, kf, vf = lo.unpack_cpu(qkv)
    of_q, of_k, of_v = lo.unpack_cpu(out_cpu)
    cos_e = cos[pos]
    sin_e = sin[pos]
    for h in range(H):
        ref = oracle.apply_rope_ref(qf[:, h].float(), cos_e, sin_e).to(torch.bfloat16)
        torch.testing.assert_close(of_q[:, h], ref, rtol=2e-2, atol=2e-2)
    for j in range(Hkv):
        ref = oracle.apply_rope_ref(kf[:, j].float(), cos_e, sin_e).to(torch.bfloat16)
        torch.testing.assert_close(of_k[:, j], ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(of_v, vf, rtol=0, atol=0)  # v untouched

    # inverse rotation restores (within bf16 rounding)
    back = out_cpu.clone().cuda()
    hip.check(
        hip.lib().dolomite_rope_qkv(
            hip.stream(), hip.ptr(back), hip.ptr(back), hip.ptr(cos_g), hip.ptr(sin_g),
            T, lo.row_len, lo.H, lo.Hkv, lo.D, lo.G, lo.q_gstride, lo.k_off, lo.kv_hstride,
            -1, 0, hip.BF16,
        ),
        "rope inverse",
    )
    torch.cuda.synchronize()
    torch.testing.assert_close(back.cpu().float(), qkv.float(), rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize(
    "head_type,H,Hkv,D,lens",
    [
        ("mqa", 8, 1, 80, [128, 64, 200]),
        ("gqa", 8, 2, 128, [96, 1, 130]),
        ("mha", 4, 4, 64, [64, 64]),
        ("mqa", 4, 1, 16, [10, 5]),       # tiny-config shape (D=16 -> DPAD 32)
        ("mqa", 8, 1, 80, [4096]),        # one full-length 3B-shaped sequence
        ("mqa", 8, 1, 80, [7, 0, 9]),     # empty sequence in the packed batch
        ("gqa", 8, 2, 128, [65, 63]),     # edge tiles on both sides of 64
        ("gqa", 6, 2, 64, [100, 60]),     # odd G=3 grouping
        ("mqa", 4, 1, 96, [200, 56]),     # D == DPAD: pad-zero prologue skipped
        ("gqa", 4, 2, 48, [77]),          # D=48 -> DPAD 64, 16-col pad band
    ],
)
def test_varlen_attention_fwd_bwd_vs_oracle(head_type, H, Hkv, D, lens):
    g = torch.Generator().manual_seed(5)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    scale = 1.0 / math.sqrt(D)
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)

    qkv_g = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(qkv_g, cu.cuda(), max(lens), lo, scale)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    o.backward(do.cuda())
    torch.cuda.synchronize()

    # oracle (fp32)
    q, k, v = lo.unpack_cpu(qkv)
    qc = q.float().requires_grad_(True)
    kc = k.float().requires_grad_(True)
    vc = v.float().requires_grad_(True)
    oc = oracle.attention_varlen_ref(qc, kc, vc, cu, scale)
    oc.backward(do.float().reshape(T, H, D))

    torch.testing.assert_close(
        o.detach().cpu().float().reshape(T, H, D), oc.detach(), rtol=2e-2, atol=2e-2
    )
    dq_g, dk_g, dv_g = lo.unpack_cpu(qkv_g.grad.cpu())
    torch.testing.assert_close(dq_g.float(), qc.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk_g.float(), kc.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv_g.float(), vc.grad, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("seed", range(6))
def test_varlen_attention_random_sweep(seed):
    """Seeded random head geometry + ragged packing through fwd+bwd vs the
    fp32 oracle — shapes the fixed parametrization does not enumerate
    (random D multiples of 8, random G, empty/singleton sequences)."""
    import random as pyrandom

    r = pyrandom.Random(1000 + seed)
    Hkv = r.choice([1, 2, 4])
    G = r.choice([1, 2, 3, 4])
    H = Hkv * G
    D = 8 * r.randint(2, 16)  # 16..128
    n_seq = r.randint(1, 4)
    lens = [r.choice([0, 1, r.randint(2, 300)]) for _ in range(n_seq)]
    if sum(lens) == 0:
        lens.append(37)
    head_type = "mha" if Hkv == H else ("mqa" if Hkv == 1 else "gqa")
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(seed)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    scale = 1.0 / math.sqrt(D)
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)

    qkv_g = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(qkv_g, cu.cuda(), max(max(lens), 1), lo, scale)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    o.backward(do.cuda())
    torch.cuda.synchronize()

    q, k, v = lo.unpack_cpu(qkv)
    qc = q.float().requires_grad_(True)
    kc = k.float().requires_grad_(True)
    vc = v.float().requires_grad_(True)
    oc = oracle.attention_varlen_ref(qc, kc, vc, cu, scale)
    oc.backward(do.float().reshape(T, H, D))

    torch.testing.assert_close(
        o.detach().cpu().float().reshape(T, H, D), oc.detach(), rtol=2e-2, atol=2e-2
    )
    dq_g, dk_g, dv_g = lo.unpack_cpu(qkv_g.grad.cpu())
    torch.testing.assert_close(dq_g.float(), qc.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk_g.float(), kc.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv_g.float(), vc.grad, rtol=3e-2, atol=3e-2)


def test_varlen_attention_deterministic_list_vs_tensor_packing():
    """Same packed input twice -> bitwise-identical output (the list-input
    path reuses the tensor path; reference requires bit-exactness there)."""
    g = torch.Generator().manual_seed(6)
    lo = QKVLayout.make(8, 1, 80, "mqa")
    cu = torch.tensor([0, 100, 164], dtype=torch.int32).cuda()
    qkv = (torch.randn(164, lo.row_len, generator=g) * 0.5).to(torch.bfloat16).cuda()
    o1 = Fx.varlen_attention(qkv.clone(), cu, 100, lo, 0.1118)
    o2 = Fx.varlen_attention(qkv.clone(), cu, 100, lo, 0.1118)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("head_type,H,Hkv,D", [("mqa", 8, 1, 80), ("gqa", 8, 2, 128)])
def test_varlen_attention_backward_bitwise_deterministic(head_type, H, Hkv, D):
    """Backward twice on the same inputs -> bitwise-identical dqkv. Guards
    the whole deterministic-gradient chain (tiled preprocess LDS reduction,
    exclusive per-q-head dk/dv partial stores, fixed-order finalize) that
    bit-exact checkpoint resume depends on — the round-1 fp32 atomicAdd
    join failed exactly this."""
    g = torch.Generator().manual_seed(11)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = torch.tensor([0, 300, 428, 4524], dtype=torch.int32).cuda()
    qkv0 = (torch.randn(4524, lo.row_len, generator=g) * 0.5).to(torch.bfloat16).cuda()
    dout = (torch.randn(4524, H * D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    grads = []
    for _ in range(2):
        qkv = qkv0.clone().requires_grad_(True)
        o = Fx.varlen_attention(qkv, cu, 4096, lo, 1.0 / math.sqrt(D))
        o.backward(dout)
        torch.cuda.synchronize()
        grads.append(qkv.grad.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("TV", [(64, 512), (230, 49152)])
def test_fused_cross_entropy(dtype, TV):
    g = torch.Generator().manual_seed(7)
    T, V = TV
    logits = (torch.randn(T, V, generator=g) * 2).to(dtype)
    labels = torch.randint(0, V, (T,), generator=g)
    labels[::7] = -100

    lg = logits.cuda().requires_grad_(True)
    loss = Fx.fused_cross_entropy(lg, labels.cuda())
    loss.backward()
    torch.cuda.synchronize()

    lc = logits.clone().requires_grad_(True)
    loss_ref, dlogits_ref = oracle.softmax_cross_entropy_fwd_bwd_ref(lc.detach(), labels)

    torch.testing.assert_close(loss.detach().cpu(), loss_ref, rtol=1e-4, atol=1e-5)
    tol = dict(rtol=1e-3, atol=1e-6) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-4)
    torch.testing.assert_close(lg.grad.cpu().float(), dlogits_ref.float(), **tol)


def test_adamw_matches_torch_on_gpu(golden_dir):
    fx = torch.load(golden_dir / "ops.pt", weights_only=False)["adamw"]
    p = fx["p0"].clone().cuda()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    pout = torch.empty_like(p, dtype=torch.bfloat16)
    for t, grd in enumerate(fx["grads"], start=1):
        Fx.adamw_step_flat(p, grd.cuda(), m, v, t, fx["lr"], fx["beta1"], fx["beta2"], fx["eps"], fx["wd"], param_out=pout)
    torch.cuda.synchronize()
    torch.testing.assert_close(p.cpu(), fx["p_final"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(m.cpu(), fx["exp_avg"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(v.cpu(), fx["exp_avg_sq"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(pout.cpu(), fx["p_final"].to(torch.bfloat16), rtol=0, atol=0)


@pytest.mark.parametrize("dtype,n", [(torch.bfloat16, 1_000_003), (torch.float32, 257)])
def test_sqsum_matches_torch_and_is_bitwise_stable(dtype, n):
    """dolomite_sqsum (grad-norm input): matches torch fp32 within reduction
    -order tolerance AND is bitwise identical across repeated runs (the
    fixed-order property the clipped-step determinism relies on)."""
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(n, generator=g) * 0.1).to(dtype).cuda()
    partials = torch.empty(1024, dtype=torch.float32, device="cuda")
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    for i in range(2):
        hip.check(
            hip.lib().dolomite_sqsum(
                hip.stream(), hip.ptr(x), x.numel(), hip.ptr(partials), hip.ptr(out, i), hip.dt(x)
            ),
            "sqsum",
        )
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])  # fixed reduction order
    ref = x.float().pow(2).sum()
    torch.testing.assert_close(out[0], ref, rtol=1e-6, atol=1e-6)


def test_adamw_fused_clip_matches_explicit_scale():
    """grad_scale (device scalar fused into the AdamW kernel) must equal
    pre-scaling the grads explicitly — exactly the old clip mul pass."""
    g = torch.Generator().manual_seed(13)
    n = 100_001
    p0 = torch.randn(n, generator=g).float()
    grad = (torch.randn(n, generator=g) * 0.5).to(torch.bfloat16).cuda()
    coef = torch.tensor(0.3725, dtype=torch.float32).cuda()

    def run(fused):
        p = p0.clone().cuda()
        m = torch.zeros_like(p)
        v = torch.zeros_like(p)
        pout = torch.empty_like(p, dtype=torch.bfloat16)
        if fused:
            Fx.adamw_step_flat(p, grad, m, v, 1, 1e-3, 0.9, 0.95, 1e-10, 0.1,
                               param_out=pout, grad_scale=coef)
        else:
            scaled = (grad.float() * coef).to(torch.float32)
            Fx.adamw_step_flat(p, scaled, m, v, 1, 1e-3, 0.9, 0.95, 1e-10, 0.1, param_out=pout)
        torch.cuda.synchronize()
        return p, m, v, pout

    pa, ma, va, oa = run(True)
    pb, mb, vb, ob = run(False)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(oa, ob)


def test_moe_rows_combine_matches_index_add():
    """Deterministic top-k combine vs torch zeros+index_add (the reference
    scatter-back, moe/base.py:127) at a tolerance, plus bitwise run-to-run
    stability. The bitwise check against the ordered fp32 sum is
    tests/test_gpu_moe_kernels.py::test_rows_combine_bitwise."""
    from dolomite_engine_amd.ops.functional import _rows_combine

    g = torch.Generator().manual_seed(14)
    T, K, k_top, E = 1337, 1024, 2, 8
    selected = torch.randint(0, E, (T, k_top), generator=g).flatten()
    _, sorted_idx = selected.sort(0)
    batch_index = (sorted_idx // k_top).cuda()
    n = T * k_top
    inv = torch.empty(n, dtype=torch.int32)
    inv[sorted_idx] = torch.arange(n, dtype=torch.int32)
    inv = inv.cuda()
    h = (torch.randn(n, K, generator=g) * 0.5).to(torch.bfloat16).cuda()

    out1 = _rows_combine(h, inv, batch_index, T, k_top)
    out2 = _rows_combine(h, inv, batch_index, T, k_top)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)

    ref = torch.zeros(T, K, dtype=h.dtype, device=h.device).index_add(0, batch_index, h)
    # fp32-accumulated combine vs bf16 index_add: one rounding difference
    torch.testing.assert_close(out1, ref, rtol=1e-2, atol=1e-2)
    # and within one bf16 rounding (2^-8 relative) of the fp32 reference
    ref32 = torch.zeros(T, K, dtype=torch.float32, device=h.device).index_add(0, batch_index.cuda(), h.float())
    torch.testing.assert_close(out1.float(), ref32, rtol=4e-3, atol=4e-3)


class TestMoEGroupedGemm:
    """Grouped expert GEMM (csrc/moe_gemm.hip) vs the eager per-expert loop
    (reference moe/base.py:12-50 semantics) — ragged groups, empty groups,
    bias, fwd + both grads."""

    @pytest.mark.parametrize(
        "E,N,K,counts,bias",
        [
            (4, 128, 64, [37, 0, 91, 12], True),
            (8, 512, 256, [64, 128, 1, 0, 200, 17, 63, 39], False),
            (2, 72, 96, [130, 70], True),   # N not multiple of 64
            (4, 256, 520, [65, 64, 63, 8], False),  # K % 64 != 0 (tail chunk)
        ],
    )
    def test_matches_eager(self, E, N, K, counts, bias):
        torch.manual_seed(17)
        T = sum(counts)
        x = (torch.randn(T, K) * 0.5).bfloat16().cuda().requires_grad_(True)
        w = (torch.randn(E, N, K) * 0.05).bfloat16().cuda().requires_grad_(True)
        b = (torch.randn(E, N) * 0.1).bfloat16().cuda().requires_grad_(True) if bias else None
        num = torch.tensor(counts, device="cuda")

        from dolomite_engine_amd.ops import grouped_expert_gemm

        y = grouped_expert_gemm(x, w, b, num)
        assert y is not None, "HIP grouped path did not engage"
        dy = torch.randn_like(y) * 0.3
        y.backward(dy)

        # eager reference (fp32 accumulated per-expert linear)
        xr = x.detach().float().requires_grad_(True)
        wr = w.detach().float().requires_grad_(True)
        br = b.detach().float().requires_grad_(True) if bias else None
        pieces = xr.split(counts, dim=0)
        ref = torch.cat(
            [torch.nn.functional.linear(pieces[i], wr[i], None if br is None else br[i]) for i in range(E)]
        )
        ref.backward(dy.float())

        torch.testing.assert_close(y.float(), ref.detach(), rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(x.grad.float(), xr.grad, rtol=3e-2, atol=3e-2)
        torch.testing.assert_close(w.grad.float(), wr.grad, rtol=3e-2, atol=3e-2)
        if bias:
            torch.testing.assert_close(b.grad.float(), br.grad, rtol=3e-2, atol=3e-2)

    def test_moe_model_grouped_path_runs(self, golden_dir):
        """Full MoE model on GPU routes experts through the grouped kernel
        (moe_gemm_fwd appears in the op profile)."""
        from dolomite_engine_amd.ops import hip as hip_mod
        from tests.test_moe_cpu import FIXTURE, build_model as build_moe

        p = golden_dir / FIXTURE
        if not p.exists():
            pytest.skip("moe golden missing")
        from oracle.golden import load_golden

        fx = load_golden(p)
        model = build_moe(fx, "flash_attention_2", padding_free=True, dtype=torch.bfloat16).cuda()
        B, S = fx["input_ids"].shape
        hip_mod.enable_profiling()
        try:
            out = model(
                input_ids=fx["input_ids"].reshape(-1).cuda(),
                position_ids=torch.arange(S).repeat(B).cuda(),
                cu_seqlens=torch.arange(0, B * S + 1, S, dtype=torch.int32).cuda(),
                max_seqlen=S,
                labels=fx["labels"].reshape(-1).cuda(),
            )
            out.loss.backward()
            torch.cuda.synchronize()
            prof = hip_mod.collect_profile()
        finally:
            hip_mod.disable_profiling()
        assert any("moe_gemm_fwd" in k for k in prof), sorted(prof)
        torch.testing.assert_close(out.loss.float().cpu(), fx["loss"], rtol=2e-2, atol=2e-2)
