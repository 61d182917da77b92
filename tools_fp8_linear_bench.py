"""A/B of ops.fp8_linear against F.linear on the bf16 weight, same process,
alternating, at the four linear shapes of the 3B config. Weights rotate over
enough copies to exceed the 256 MB last-level cache, so every call streams
its weight from HBM. The calls of one pass over the copies are captured into
a graph (no host launch gaps: the kernels take a few microseconds) and the
replay is timed with device events. `--sweep` also times half, twice and four
times the default split count. Appends the table to ./fp8_linear_ab.txt."""

import os
import sys


import torch
import torch.nn.functional as F

from dolomite_engine_amd.ops import functional as Fx

HBM_PEAK_GBS = 8000.0
SHAPES = [("attn.c_attn", 2720, 2560), ("attn.c_proj", 2560, 2560), ("mlp.c_fc", 10240, 2560), ("mlp.c_proj", 2560, 10240)]
MS = [1, 8, 32, 64]
ROTATE_BYTES = 640 << 20
sweep = "--sweep" in sys.argv


def emit(s):
    print(s, flush=True)
    with open("fp8_linear_ab.txt", "a") as f:
        f.write(s + "\n")


def capture(fn, n):
    for i in range(min(n, 3)):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    return g


def window(g, n, replays):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        g.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / (n * replays)  # us per call


def ab(graphs, n):
    """Alternate the graphs' windows, 5 rounds; (median, min, max) us per call each."""
    replays = 10
    ts = [[] for _ in graphs]
    for _ in range(5):
        for g, t in zip(graphs, ts):
            t.append(window(g, n, replays))
    return [(sorted(t)[2], min(t), max(t)) for t in ts]


emit(f"# fp8_linear vs bf16 F.linear, MI355X, HBM peak {HBM_PEAK_GBS:.0f} GB/s. us per call: median of 5 alternating "
     f"windows (min..max), each 10 replays of a captured pass over the weight copies (> {ROTATE_BYTES >> 20} MB)")
emit("# GB/s = weight bytes / time (fp8: N*K, bf16: 2*N*K); ratio = fp8 time / bf16 time (ideal 0.5)")
emit(f"{'linear':12s} {'N':>6s} {'K':>6s} {'M':>3s} {'nsplit':>6s} {'fp8 us':>24s} {'GB/s':>6s} {'%peak':>5s} "
     f"{'bf16 us':>24s} {'GB/s':>6s} {'ratio':>6s}")
torch.manual_seed(0)
for name, N, K in SHAPES:
    ncopy = -(-ROTATE_BYTES // (N * K))
    w = torch.randn(N, K, device="cuda") * 0.02
    wq1, sc1 = Fx.quantize_weight_e4m3(w)
    wq = wq1.unsqueeze(0).repeat(ncopy, 1, 1)
    wb = w.to(torch.bfloat16).unsqueeze(0).repeat(ncopy, 1, 1)
    wd = wq1.double() * sc1.double()[:, None]
    for M in MS:
        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        ns = Fx.fp8_linear_num_splits(M, N, K)
        y = Fx.fp8_linear(x, wq[ncopy - 1], sc1)
        ref, S = x.double() @ wd.T, x.double().abs() @ wd.abs().T
        assert bool(((y.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S).all()), (name, M)
        with torch.no_grad():
            g8 = capture(lambda i: Fx.fp8_linear(x, wq[i], sc1), ncopy)
            gb = capture(lambda i: F.linear(x, wb[i]), ncopy)
            (t8, tb) = ab([g8, gb], ncopy)
            g8s, gbs = N * K / t8[0] / 1e3, 2 * N * K / tb[0] / 1e3
            emit(f"{name:12s} {N:6d} {K:6d} {M:3d} {ns:6d} {t8[0]:8.2f} ({t8[1]:6.2f}..{t8[2]:6.2f}) {g8s:6.0f} "
                 f"{100 * g8s / HBM_PEAK_GBS:5.1f} {tb[0]:8.2f} ({tb[1]:6.2f}..{tb[2]:6.2f}) {gbs:6.0f} {t8[0] / tb[0]:6.2f}")
            if sweep:
                cand = [s for s in sorted({1, max(1, ns // 2), ns * 2, ns * 4} - {ns}) if s <= -(-K // 64)]
                gs = [capture(lambda i, s=s: Fx.fp8_linear(x, wq[i], sc1, num_splits=s), ncopy) for s in cand]
                for s, t in zip(cand, ab(gs, ncopy) if gs else []):
                    emit(f"#   sweep {name} M={M} num_splits={s}: {t[0]:8.2f} us ({t[1]:.2f}..{t[2]:.2f})")
                del gs
            del g8, gb
    del wq, wb
