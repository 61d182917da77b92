"""Extend attention against the existing kernels (profiles/extend_attention_bench.txt).

3B attention layout (H=32, MQA, D=80), bf16. HIP events around WINDOW
back-to-back calls, the two sides of a comparison interleaved in one
session, median / min / max of 10 windows per side, after a warm-up of each.

  verify: B=16, past=4096, n in {2, 4, 8}: one extend_attention call against
          n decode_attention calls over the same cache (key counts past+1 ..
          past+n), both with their default split rule.
  chunk:  B=4, a 2048-token chunk on past in {0, 6144}, against
          span_attention over a 2048-token prompt; TFLOP/s by the
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


def _line(label, ms, flop=None):
    med = statistics.median(ms)
    rate = f"  {flop / med / 1e9:7.1f} TFLOP/s" if flop else ""
    print(f"{label:<44s} median {med * 1e3:9.1f} us  min {min(ms) * 1e3:9.1f}  max {max(ms) * 1e3:9.1f}{rate}")


def _case(B, past, n):
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * n, LO.row_len, generator=g) * 0.7).to(torch.bfloat16).cuda()
    k = (torch.randn(B, past + n, 1, LO.D, generator=g) * 0.7).to(torch.bfloat16).cuda()
    v = (torch.randn(B, past + n, 1, LO.D, generator=g) * 0.7).to(torch.bfloat16).cuda()
    begin = torch.arange(B, dtype=torch.int32, device="cuda") * n
    lens = torch.full((B,), past + n, dtype=torch.int32, device="cuda")
    return qkv, k, v, begin, begin + n, lens


@torch.no_grad()
def main():
    print(f"device: {torch.cuda.get_device_name(0)}; {WINDOWS} windows of {WINDOW} calls per side, interleaved")
    B, past = 16, 4096
    for n in (2, 4, 8):
        qkv, k, v, sb, se, lens = _case(B, past, n)
        rows = [qkv[i::n].contiguous() for i in range(n)]          # token i of every sequence
        step_len = [lens - (n - 1 - i) for i in range(n)]

        def decode_n():
            for i in range(n):
                Fx.decode_attention(rows[i], LO, k, v, step_len[i], SCALE, past + i + 1)

        res = _time({
            "extend": lambda: Fx.extend_attention(qkv, LO, sb, se, n, k, v, lens, SCALE, past + n),
            "decode": decode_n,
        })
        ns = Fx.extend_num_splits(B, LO, n, past + n)
        _line(f"verify B={B} past={past} n={n}: extend (nsplit {ns})", res["extend"])
        _line(f"verify B={B} past={past} n={n}: {n} x decode", res["decode"])

    B, n = 4, 2048
    for past in (0, 6144):
        qkv, k, v, sb, se, lens = _case(B, past, n)
        flop = 4.0 * LO.H * LO.D * B * (n * past + n * (n + 1) / 2)
        sides = {"extend": lambda: Fx.extend_attention(qkv, LO, sb, se, n, k, v, lens, SCALE, past + n)}
        if past == 0:
            sides["span"] = lambda: Fx.span_attention(qkv, sb, se, n, LO, SCALE)
        res = _time(sides)
        _line(f"chunk B={B} n={n} past={past}: extend", res["extend"], flop)
        if past == 0:
            _line(f"chunk B={B} n={n} past=0: span_attention", res["span"], flop)


if __name__ == "__main__":
    main()
