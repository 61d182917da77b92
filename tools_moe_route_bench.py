"""MoE routing region, HIP op against the torch chain it replaces
(profiles/moe_route_bench.txt).

The MoE bench shape: T = 65536 tokens, E = 32, top_k = 2, bf16 router logits;
forward plus backward of the region between the gate GEMM and the first
expert GEMM (d_batch_gates in, d_logits out). HIP events around WINDOW
back-to-back calls, the two sides interleaved in one session, median / min /
max of 10 windows per side after a warm-up of each; then the GPU kernel
launches of one call of each side, counted by torch.profiler.
"""

import statistics

import torch
import torch.nn.functional as F

import dolomite_engine_amd.ops as ops

T, E, K = 65536, 32, 2
WINDOW, WINDOWS = 20, 10


def torch_chain(logits, dbg):
    lg = logits.detach().requires_grad_(True)
    w, sel = lg.topk(K, dim=-1)
    w = F.softmax(w.float(), dim=-1).type_as(lg)
    flat = sel.flatten()
    num = flat.bincount(minlength=E)
    _, order = flat.sort(0)
    batch_index = order // K
    batch_gates = w.flatten()[order]
    inv = torch.empty(flat.numel(), dtype=torch.int32, device=lg.device)
    inv[order] = torch.arange(flat.numel(), dtype=torch.int32, device=lg.device)
    batch_gates.backward(dbg)
    return lg.grad, batch_index, inv, num


def hip_route(logits, dbg):
    lg = logits.detach().requires_grad_(True)
    batch_gates, batch_index, inv, num, _ = ops.moe_route(lg, K)
    batch_gates.backward(dbg)
    return lg.grad, batch_index, inv, num


def _launches(fn, *args):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(*args)
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def main():
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(T, E, generator=g) * 2).to(torch.bfloat16).cuda()
    dbg = torch.randn(T * K, generator=g).to(torch.bfloat16).cuda()
    sides = {"hip moe_route": hip_route, "torch chain": torch_chain}
    print(f"device: {torch.cuda.get_device_name(0)}; T={T} E={E} top_k={K} bf16, fwd+bwd; "
          f"{WINDOWS} windows of {WINDOW} calls per side, interleaved", flush=True)
    for fn in sides.values():
        for _ in range(3):
            fn(logits, dbg)
    ms = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(WINDOW):
                fn(logits, dbg)
            stop.record()
            stop.synchronize()
            ms[name].append(start.elapsed_time(stop) / WINDOW)
    for name, v in ms.items():
        print(f"{name:<16s} median {statistics.median(v) * 1e3:9.1f} us  min {min(v) * 1e3:9.1f}  max {max(v) * 1e3:9.1f}",
              flush=True)
    for name, fn in sides.items():
        print(f"{name:<16s} GPU kernel launches per call (fwd+bwd): {_launches(fn, logits, dbg)}", flush=True)


if __name__ == "__main__":
    main()
