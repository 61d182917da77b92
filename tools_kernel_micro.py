"""Standalone micro-timing for the small bandwidth kernels (preprocess,
finalize, norm bwd) against their algorithmic byte counts. Event-timed,
K iterations back-to-back, no profiler. Pure analysis tool.

`python tools_kernel_micro.py decode` times the single-token decode
attention kernel instead (and `generate` end to end): see decode_case()."""
import math
import statistics
import sys
import time

import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip

T, H, Hkv, D = 65536, 32, 1, 80
dev = "cuda"
torch.manual_seed(0)
PEAK = 6.3e3  # GB/s measured


def timed(fn, k=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def timed_median(fn, n=20, warm=5):
    """Median and min / max of n individually event-timed calls after warm-up (ms)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


COPY_CEILING = 6.29e3  # GB/s: the measured device copy ceiling (MI355X_MICROARCH.md)


def decode_case():
    """decode_attention at the 3B attention shape (small: launch / latency
    bound) and at a bandwidth-sized GQA shape, beside
    F.scaled_dot_product_attention on the same cache (the path a user has
    without the kernel) and the copy ceiling. Bytes = the K/V the step must
    read, 2 * B * len * Hkv * D * 2; q, o and the split partials are not
    counted. Then greedy generate tokens/s on the 350M config."""
    import torch.nn.functional as F

    from dolomite_engine_amd.ops.functional import QKVLayout

    shapes = [
        ("3B attention shape", "mqa", 32, 1, 80, 16, 4096),
        ("bandwidth-sized   ", "gqa", 32, 8, 128, 32, 8192),
    ]
    for name, head_type, H, Hkv, D, B, n in shapes:
        lo = QKVLayout.make(H, Hkv, D, head_type)
        qkv = (torch.randn(B, lo.row_len, device=dev) * 0.5).to(torch.bfloat16)
        k = (torch.randn(B, n, Hkv, D, device=dev) * 0.5).to(torch.bfloat16)
        v = (torch.randn(B, n, Hkv, D, device=dev) * 0.5).to(torch.bfloat16)
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        scale = 1.0 / math.sqrt(D)
        gb = 2 * B * n * Hkv * D * 2 / 1e9
        # q as (B, H, 1, D) for SDPA; K/V as (B, Hkv, n, D) views of the same cache
        qh = torch.stack(
            [qkv[:, (h // lo.G) * lo.q_gstride + (h % lo.G) * D:][:, :D] for h in range(H)], dim=1
        ).unsqueeze(2).contiguous()
        kh, vh = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        print(f"--- {name}: {head_type} H={H} Hkv={Hkv} D={D} B={B} cache={n}  K/V {gb * 1e3:.1f} MB ---")
        with torch.no_grad():
            ref = F.scaled_dot_product_attention(qh, kh, vh, scale=scale, enable_gqa=True)
            ref = ref.squeeze(2).reshape(B, H * D).float()
            auto = Fx.decode_num_splits(B, lo, n)
            for ns in sorted({1, auto, 2 * auto, 4 * auto}):
                fn = lambda: Fx.decode_attention(qkv, lo, k, v, lens, scale, n, num_splits=ns)
                err = (fn().float() - ref).abs().max().item()
                med, lo_t, hi_t = timed_median(fn)
                tag = " (default)" if ns == auto else ""
                print(f"decode nsplit={ns:3d}{tag:10s}: {med * 1e3:8.1f} us [{lo_t * 1e3:.1f}..{hi_t * 1e3:.1f}]  "
                      f"{gb / med * 1e3:6.0f} GB/s ({gb / med * 1e3 / COPY_CEILING * 100:4.1f}% of the copy ceiling)  "
                      f"max|o - sdpa| {err:.2e}")
            med, lo_t, hi_t = timed_median(
                lambda: F.scaled_dot_product_attention(qh, kh, vh, scale=scale, enable_gqa=True))
            print(f"torch SDPA (enable_gqa)    : {med * 1e3:8.1f} us [{lo_t * 1e3:.1f}..{hi_t * 1e3:.1f}]  "
                  f"{gb / med * 1e3:6.0f} GB/s ({gb / med * 1e3 / COPY_CEILING * 100:4.1f}% of the copy ceiling)")
        del qkv, k, v, kh, vh

    # end to end: greedy generate, 128 new tokens, the 350M bench config
    import bench
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

    cfg = GPTDolomiteConfig(**bench.MODEL_350M)
    cfg._attn_implementation = "flash_attention_2"
    model = GPTDolomiteForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()
    for B, S in ((1, 512), (16, 512)):
        ids = torch.randint(0, cfg.vocab_size, (B, S), device=dev)
        model.generate(ids, max_new_tokens=8)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = model.generate(ids, max_new_tokens=128)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        print(f"generate 350M greedy B={B:2d} prompt={S} +128 tokens: {t * 1e3:7.1f} ms "
              f"(prefill included)  {B * 128 / t:7.0f} tokens/s  {128 / t:6.1f} steps/s")
        assert out.shape == (B, S + 128)


if len(sys.argv) > 1 and sys.argv[1] == "decode":
    decode_case()
    sys.exit(0)

# --- fa_bwd_preprocess: delta[h,t] = rowsum(dO*O) ---
o = torch.randn(T, H * D, dtype=torch.bfloat16, device=dev)
do = torch.randn(T, H * D, dtype=torch.bfloat16, device=dev)
delta = torch.empty(H, T, dtype=torch.float32, device=dev)


def pre():
    hip.check(
        hip.lib().dolomite_fa_bwd_preprocess(
            hip.stream(), hip.ptr(o), hip.ptr(do), hip.ptr(delta), T, H, D, H * D, H * D, hip.BF16
        ),
        "pre",
    )


ms = timed(pre)
gb = (2 * T * H * D * 2 + H * T * 4) / 1e9
print(f"preprocess : {ms:6.3f} ms  {gb/ms*1e3:6.0f} GB/s ({gb/ms*1e3/PEAK*100:4.1f}% of peak)")

# correctness vs torch
ref = (o.view(T, H, D).float() * do.view(T, H, D).float()).sum(-1).t().contiguous()
err = (delta - ref).abs().max().item()
print(f"             max|err| vs torch fp32: {err:.3e}")

# --- fa_grad_finalize: reduce (T, HG, D) fp32 pairs into packed bf16 ---
G = H // Hkv
dk_acc = torch.randn(T, H, D, dtype=torch.float32, device=dev)
dv_acc = torch.randn(T, H, D, dtype=torch.float32, device=dev)
row_len = (H + 2 * Hkv) * D
dqkv = torch.empty(T, row_len, dtype=torch.bfloat16, device=dev)


def fin():
    hip.check(
        hip.lib().dolomite_fa_grad_finalize(
            hip.stream(), hip.ptr(dk_acc), hip.ptr(dv_acc), hip.ptr(dqkv),
            T, Hkv, D, G, row_len, H * D, D, (H + Hkv) * D, hip.BF16,
        ),
        "fin",
    )


ms = timed(fin)
gb = (2 * T * H * D * 4 + 2 * T * Hkv * D * 2) / 1e9
print(f"finalize   : {ms:6.3f} ms  {gb/ms*1e3:6.0f} GB/s ({gb/ms*1e3/PEAK*100:4.1f}% of peak)")

# --- rmsnorm bwd (fused dres) ---
Hn = 2560
x = torch.randn(T, Hn, dtype=torch.bfloat16, device=dev).requires_grad_(True)
w = (torch.randn(Hn, dtype=torch.bfloat16, device=dev) * 0.1 + 1.0).requires_grad_(True)
r = torch.randn(T, Hn, dtype=torch.bfloat16, device=dev).requires_grad_(True)
y, s = Fx.fused_rmsnorm(x, w, 1e-5, residual=r)
dy = torch.randn_like(y)
ds = torch.randn_like(s)
g = torch.autograd.grad((y, s), (x, r, w), (dy, ds), retain_graph=True)


def nb():
    torch.autograd.grad((y, s), (x, r, w), (dy, ds), retain_graph=True)


ms = timed(nb)
gb = (5 * T * Hn * 2) / 1e9  # dy, ds, s reads + dx write (+ s_hat cast path) approx
print(f"norm_bwd   : {ms:6.3f} ms  {gb/ms*1e3:6.0f} GB/s ({gb/ms*1e3/PEAK*100:4.1f}% of peak)")
