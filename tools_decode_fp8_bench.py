"""Decode attention and the decode-step append on the fp8 KV cache against the
bf16 cache of the same build (profiles/decode_fp8_bench.txt).

3B attention layout (H=32, MQA, D=80), B=16, bf16 queries. HIP events around
WINDOW back-to-back calls, the two sides interleaved in one session, median /
min / max of 10 windows per side after a warm-up of each. Bytes are what the
step must read: the valid K and V of every sequence once — 2 bytes an element
in bf16, 1 byte an element plus one fp32 scale per (key, kv head) in fp8.
The append moves one row per sequence (launch-bound: no rate given).
"""

import math
import statistics

import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops.functional import QKVLayout

LO = QKVLayout.make(32, 1, 80, "mqa")
SCALE = 1.0 / math.sqrt(LO.D)
B = 16
WINDOW, WINDOWS = 50, 10


def _time(sides):
    """{name: [ms per call] * WINDOWS}, the sides alternating window by window."""
    for fn in sides.values():
        for _ in range(5):
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


def _line(label, ms, nbytes=None):
    med = statistics.median(ms)
    rate = f"  {nbytes / med / 1e9:6.2f} TB/s" if nbytes else ""
    print(f"{label:<40s} median {med * 1e3:8.1f} us  min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f}{rate}")


@torch.no_grad()
def main():
    print(f"device: {torch.cuda.get_device_name(0)}; {WINDOWS} windows of {WINDOW} calls per side, interleaved")
    g = torch.Generator().manual_seed(0)
    for length in (4096, 32768):
        cap = length + 8
        qkv = (torch.randn(B, LO.row_len, generator=g) * 0.7).to(torch.bfloat16).cuda()
        kv = (torch.randn(2, B, cap, 1, LO.D, generator=g) * 0.7).to(torch.bfloat16).cuda()
        (k8, ks), (v8, vs) = (Fx.quantize_kv_e4m3(x) for x in kv)
        ks, vs = ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()
        lens = torch.full((B,), length, dtype=torch.int32, device="cuda")
        res = _time({
            "bf16": lambda: Fx.decode_attention(qkv, LO, kv[0], kv[1], lens, SCALE, length),
            "fp8": lambda: Fx.decode_attention(qkv, LO, k8, v8, lens, SCALE, length, k_scale=ks, v_scale=vs),
        })
        ns = Fx.decode_num_splits(B, LO, length)
        keys = 2 * B * length * LO.Hkv
        _line(f"decode len={length} (nsplit {ns}): bf16", res["bf16"], keys * LO.D * 2)
        _line(f"decode len={length} (nsplit {ns}): fp8", res["fp8"], keys * (LO.D + 4))
        diff = (Fx.decode_attention(qkv, LO, k8, v8, lens, SCALE, length, k_scale=ks, v_scale=vs).float()
                - Fx.decode_attention(qkv, LO, kv[0], kv[1], lens, SCALE, length).float()).abs().max()
        print(f"decode len={length}: max|fp8 - bf16 output| {float(diff):.3e}")

        rows = torch.arange(B, dtype=torch.int32, device="cuda")
        pos = lens - 1
        res = _time({
            "bf16": lambda: Fx.kv_cache_append(qkv, LO, rows, rows + 1, kv[0], kv[1], pos, max_rows=1),
            "fp8": lambda: Fx.kv_cache_append(qkv, LO, rows, rows + 1, k8, v8, pos, max_rows=1,
                                              k_scale=ks, v_scale=vs),
        })
        _line(f"append 1 row/seq at len={length}: bf16", res["bf16"])
        _line(f"append 1 row/seq at len={length}: fp8", res["fp8"])


if __name__ == "__main__":
    main()
