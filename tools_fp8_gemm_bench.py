"""A/B/C of ops.fp8_linear's tiled GEMM kernel (more than 64 rows) against the
route it replaces and against bf16, same process, alternating, at the four
linear shapes of the 3B config and M = 128 .. 4096:
  (a) the kernel (csrc/fp8_gemm.hip), whatever FP8_GEMM_MAX_ROWS says;
  (b) the dequantised route, written out: F.linear on wq.to(bf16) * scale;
  (c) bf16 F.linear on the bf16 weight.
The method is tools_fp8_linear_bench.py's: weights rotate over enough copies
to exceed the 256 MB last-level cache, the calls of one pass over the copies
are captured into a graph and the replay is timed with device events, the
sides' windows alternate. `--sweep` also times half and twice the default
split count where it is above one. Appends the table to ./fp8_gemm_ab.txt."""

import sys

import torch
import torch.nn.functional as F

from dolomite_engine_amd.ops import functional as Fx

SHAPES = [("attn.c_attn", 2720, 2560), ("attn.c_proj", 2560, 2560), ("mlp.c_fc", 10240, 2560), ("mlp.c_proj", 2560, 10240)]
MS = [128, 256, 512, 1024, 2048, 4096]
ROTATE_BYTES = 640 << 20
sweep = "--sweep" in sys.argv
Fx.FP8_GEMM_MAX_ROWS = None  # (a) is the kernel at every M; the op's bound is what this table decides


def emit(s):
    print(s, flush=True)
    with open("fp8_gemm_ab.txt", "a") as f:
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


def ab(graphs, n, replays=10):
    """Alternate the graphs' windows, 5 rounds; (median, min, max) us per call each."""
    ts = [[] for _ in graphs]
    for _ in range(5):
        for g, t in zip(graphs, ts):
            t.append(window(g, n, replays))
    return [(sorted(t)[2], min(t), max(t)) for t in ts]


def cell(t):
    return f"{t[0]:9.2f} ({t[1]:8.2f}..{t[2]:8.2f})"


emit("# fp8 tiled GEMM kernel (a) vs the dequantised route (b) vs bf16 F.linear (c), MI355X. us per call: median of 5 "
     f"alternating windows (min..max), each 10 replays of a captured pass over the weight copies (> {ROTATE_BYTES >> 20} MB)")
emit("# a/b, a/c = ratios of the medians; TF/s = 2*M*N*K / (a)'s median")
emit(f"{'linear':12s} {'N':>6s} {'K':>6s} {'M':>5s} {'nsplit':>6s} {'(a) kernel us':>30s} {'TF/s':>6s} "
     f"{'(b) dequantised us':>30s} {'(c) bf16 us':>30s} {'a/b':>5s} {'a/c':>5s}")
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
        ns = Fx.fp8_gemm_num_splits(M, N, K)
        y = Fx.fp8_linear(x, wq[ncopy - 1], sc1)
        ref, S = x.double() @ wd.T, x.double().abs() @ wd.abs().T
        assert bool(((y.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S).all()), (name, M)
        del y, ref, S
        with torch.no_grad():
            ga = capture(lambda i: Fx.fp8_linear(x, wq[i], sc1), ncopy)
            gb = capture(lambda i: F.linear(x, wq[i].to(x.dtype) * sc1[:, None].to(x.dtype)), ncopy)
            gc = capture(lambda i: F.linear(x, wb[i]), ncopy)
            ta, tb, tc = ab([ga, gb, gc], ncopy)
            emit(f"{name:12s} {N:6d} {K:6d} {M:5d} {ns:6d} {cell(ta)} {2e-6 * M * N * K / ta[0]:6.0f} {cell(tb)} {cell(tc)} "
                 f"{ta[0] / tb[0]:5.2f} {ta[0] / tc[0]:5.2f}")
            if sweep and ns > 1:
                cand = sorted({max(1, ns // 2), ns * 2} - {ns})
                gs = [capture(lambda i, s=s: Fx.fp8_linear(x, wq[i], sc1, num_splits=s), ncopy) for s in cand]
                for s, t in zip(cand, ab(gs, ncopy)):
                    emit(f"#   sweep {name} M={M} num_splits={s}: {cell(t)}")
                del gs
            del ga, gb, gc
    del wq, wb
