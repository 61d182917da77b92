"""GLU activation, the fused HIP op against the torch chain it replaces
(profiles/glu_bench.txt).

Shapes: the Llama-8B MLP of `bench.py --model llama8b` (16384 rows,
I = 14336) and the expert rows of `bench.py --model moe` (131072 pairs,
I = 1024), swiglu, bf16. HIP events around WINDOW back-to-back calls, the
sides interleaved in one session, median / min / max of 10 windows per side
after a warm-up of each. Effective TB/s is against the bytes the operation
needs: 3·R·I elements forward, 5·R·I backward (8·R·I for forward+backward).

`--lib NAME=PATH` (repeatable) adds the raw entry points of another build of
the library to the kernel-only table, e.g. one compiled with
-DDOLOMITE_GLU_GRID_CAP=2048 (grid-stride over 8 workgroups per CU) or
-DDOLOMITE_GLU_NT_DH=0 (plain dh stores). `--memory` adds the peak
memory of one forward+backward of the Llama-shape MLP, op against chain.
"""

import argparse
import ctypes
import statistics

import torch
import torch.nn.functional as F

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.ops import hip

SHAPES = [("llama8b mlp", 16384, 14336), ("moe experts", 131072, 1024)]
WINDOW, WINDOWS = 20, 10


def chain(h):
    a, b = h.chunk(2, dim=-1)
    return a * F.silu(b)


def fused(h):
    return ops.glu_activation(h, "swiglu")


def timed(sides, nbytes):
    """sides: {name: zero-argument callable}; prints one line per side."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    ms = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(WINDOW):
                fn()
            stop.record()
            stop.synchronize()
            ms[name].append(start.elapsed_time(stop) / WINDOW)
    for name, v in ms.items():
        med = statistics.median(v)
        print(f"  {name:<26s} median {med * 1e3:9.1f} us  min {min(v) * 1e3:9.1f}  max {max(v) * 1e3:9.1f}"
              f"  {nbytes / med / 1e9:6.2f} TB/s effective", flush=True)


def load(path):
    lib = ctypes.CDLL(path)
    for name in ("dolomite_glu_fwd", "dolomite_glu_bwd"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGNATURES[name]
    return lib


def peak_memory():
    from dolomite_engine_amd.hf_models.config import GPTDolomiteConfig
    from dolomite_engine_amd.hf_models import modeling

    cfg = GPTDolomiteConfig(n_embd=4096, n_head=32, n_inner=14336, n_layer=32, activation_function="swiglu",
                            add_bias=False, resid_pdrop=0.0)
    mlp = modeling.MLP(cfg).to(torch.bfloat16).cuda()
    x = torch.randn(16384, 4096, dtype=torch.bfloat16, device="cuda")
    real = modeling.glu_activation
    for name, fn in (("hip glu_activation", real), ("torch chain", lambda h, _: chain(h))):
        modeling.glu_activation = fn
        peaks = []
        for _ in range(2):
            mlp.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            xin = x.clone().requires_grad_(True)
            mlp(xin).sum().backward()
            torch.cuda.synchronize()
            peaks.append((torch.cuda.max_memory_allocated() - base) / 2**20)
            del xin
        print(f"  {name:<26s} peak over the resident weights and input: {peaks[-1]:9.1f} MiB", flush=True)
    modeling.glu_activation = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--memory", action="store_true")
    args = ap.parse_args()
    libs = {"in-tree library": hip.lib()}
    libs.update({name: load(path) for name, path in (spec.split("=", 1) for spec in args.lib)})

    print(f"device: {torch.cuda.get_device_name(0)}; swiglu bf16; {WINDOWS} windows of {WINDOW} calls per side, "
          f"interleaved", flush=True)
    for label, R, I in SHAPES:
        gen = torch.Generator().manual_seed(0)
        h = (torch.rand(R, 2 * I, generator=gen) * 16 - 8).to(torch.bfloat16).cuda()
        g = torch.randn(R, I, generator=gen).to(torch.bfloat16).cuda()
        hg = h.detach().requires_grad_(True)
        elem = R * I * h.element_size()
        print(f"{label}: R={R} I={I}", flush=True)
        print(" op, forward (no grad):", flush=True)
        with torch.no_grad():
            timed({"hip glu_activation": lambda: fused(h), "torch chain": lambda: chain(h)}, 3 * elem)
        print(" op, forward + backward:", flush=True)
        timed({"hip glu_activation": lambda: torch.autograd.grad(fused(hg), hg, g),
               "torch chain": lambda: torch.autograd.grad(chain(hg), hg, g)}, 8 * elem)
        y, dh = torch.empty_like(g), torch.empty_like(h)
        s, bf16 = hip.stream(), hip.BF16
        print(" entry points alone:", flush=True)
        timed({f"glu_fwd, {name}": (lambda L=L: L.dolomite_glu_fwd(s, hip.ptr(h), 2 * I, hip.ptr(y), R, I, 0, bf16))
               for name, L in libs.items()}, 3 * elem)
        timed({f"glu_bwd, {name}": (lambda L=L: L.dolomite_glu_bwd(s, hip.ptr(g), hip.ptr(h), 2 * I, hip.ptr(dh),
                                                                   R, I, 0, bf16))
               for name, L in libs.items()}, 5 * elem)
        del h, g, hg, y, dh
    if args.memory:
        print("peak memory, one forward+backward of the Llama-shape MLP (16384 x 4096 -> 2*14336 -> 4096):", flush=True)
        peak_memory()


if __name__ == "__main__":
    main()
