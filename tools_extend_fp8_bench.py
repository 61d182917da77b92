"""Extend attention over the fp8 (e4m3) KV cache against the bf16 cache
(profiles/extend_fp8_bench.txt).

3B attention layout (H=32, MQA, D=80), bf16 qkv. HIP events around WINDOW
back-to-back calls, the fp8 and the bf16 cache interleaved in one session,
median / min / max of 10 windows per side, after a warm-up of each. Both
caches hold the same keys and values (the bf16 one unquantised), both calls
use the default split rule.

  verify: B=16, n=4 draft tokens on past in {4096, 32768}; GB/s of the cache
          bytes each side must read (K and V once per kv head, the fp8 side's
          two scale arrays included).
  chunk:  B=4, a 2048-token chunk on past=6144; TFLOP/s by the
          causal-algorithmic count 2*2*H*D*(visible (query, key) pairs).
"""

import math
import statistics

import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops.functional import QKVLayout

LO = QKVLayout.make(32, 1, 80, "mqa")
SCALE = 1.0 / math.sqrt(LO.D)
WINDOW, WINDOWS = 20, 10


def _time(sides):
    """{name: [ms per call] * WINDOWS}, the sides alternating window by window."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    out = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(WINDOW):
                fn()
            stop.record()
            stop.synchronize()
            out[name].append(start.elapsed_time(stop) / WINDOW)
    return out


def _line(label, ms, nbytes=None, flop=None):
    med = statistics.median(ms)
    rate = f"  {nbytes / med / 1e6:7.1f} GB/s" if nbytes else ""
    rate += f"  {flop / med / 1e9:7.1f} TFLOP/s" if flop else ""
    print(f"{label:<44s} median {med * 1e3:9.1f} us  min {min(ms) * 1e3:9.1f}  max {max(ms) * 1e3:9.1f}{rate}")


def _case(B, past, n):
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * n, LO.row_len, generator=g) * 0.7).to(torch.bfloat16).cuda()
    k = (torch.randn(B, past + n, 1, LO.D, generator=g) * 0.7).to(torch.bfloat16).cuda()
    v = (torch.randn(B, past + n, 1, LO.D, generator=g) * 0.7).to(torch.bfloat16).cuda()
    begin = torch.arange(B, dtype=torch.int32, device="cuda") * n
    lens = torch.full((B,), past + n, dtype=torch.int32, device="cuda")
    return qkv, k, v, begin, begin + n, lens


def _sides(B, past, n):
    qkv, k, v, sb, se, lens = _case(B, past, n)
    (k8, ks), (v8, vs) = Fx.quantize_kv_e4m3(k), Fx.quantize_kv_e4m3(v)
    ks, vs = ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()   # (B, Hkv, S_cap)
    o8 = Fx.extend_attention(qkv, LO, sb, se, n, k8, v8, lens, SCALE, past + n, k_scale=ks, v_scale=vs)
    o16 = Fx.extend_attention(qkv, LO, sb, se, n, k, v, lens, SCALE, past + n)
    print(f"B={B} past={past} n={n}: max|o_fp8 - o_bf16| {float((o8.float() - o16.float()).abs().max()):.3e} "
          f"(the quantisation; max|o_bf16| {float(o16.float().abs().max()):.3e})")
    return {
        "fp8": lambda: Fx.extend_attention(qkv, LO, sb, se, n, k8, v8, lens, SCALE, past + n, k_scale=ks, v_scale=vs),
        "bf16": lambda: Fx.extend_attention(qkv, LO, sb, se, n, k, v, lens, SCALE, past + n),
    }


@torch.no_grad()
def main():
    print(f"device: {torch.cuda.get_device_name(0)}; {WINDOWS} windows of {WINDOW} calls per side, interleaved")
    B, n = 16, 4
    for past in (4096, 32768):
        res = _time(_sides(B, past, n))
        ns = Fx.extend_num_splits(B, LO, n, past + n)
        keys = B * (past + n)
        _line(f"verify B={B} n={n} past={past}: fp8 (nsplit {ns})", res["fp8"], nbytes=keys * (2 * LO.D + 8))
        _line(f"verify B={B} n={n} past={past}: bf16 (nsplit {ns})", res["bf16"], nbytes=keys * 4 * LO.D)

    B, n, past = 4, 2048, 6144
    res = _time(_sides(B, past, n))
    flop = 4.0 * LO.H * LO.D * B * (n * past + n * (n + 1) / 2)
    _line(f"chunk B={B} n={n} past={past}: fp8", res["fp8"], flop=flop)
    _line(f"chunk B={B} n={n} past={past}: bf16", res["bf16"], flop=flop)


if __name__ == "__main__":
    main()
