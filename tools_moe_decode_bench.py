"""A/B of the fused MoE decode MLP (ops.moe_decode_mlp + ops.moe_route_topk)
against the unfused SparseMoE.forward at the bench MoE shape, and generate()
tokens/s with and without it, on one MI355X.

    python tools_moe_decode_bench.py [OUT]     (default profiles/moe_decode_ab.txt)"""

import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench import MODEL_MOE  # noqa: E402
from dolomite_engine_amd import ops  # noqa: E402
from dolomite_engine_amd.hf_models import MoEDolomiteConfig, MoEDolomiteForCausalLM  # noqa: E402
from dolomite_engine_amd.hf_models.moe import MoEDolomiteBlock, SparseMoE  # noqa: E402

OUT = Path(sys.argv[1] if len(sys.argv) > 1 else "profiles/moe_decode_ab.txt")
OUT.parent.mkdir(parents=True, exist_ok=True)
assert torch.cuda.is_available(), "this measurement needs the GPU"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)
    OUT.write_text("\n".join(lines) + "\n")


kw = {k: v for k, v in MODEL_MOE.items() if k != "model_type"}
cfg = MoEDolomiteConfig(**kw)
cfg._attn_implementation = "flash_attention_2"
torch.manual_seed(0)
dev = "cuda"

# ---- 1. the MLP alone: 4 layers' experts (768 MB of weight: more than the 256 MB
# Infinity Cache), 8 inputs each, so no call finds its experts cached by the last
NL, NX, ITERS, WINDOWS = 4, 8, 50, 5
mlps = [SparseMoE(cfg).to(torch.bfloat16).to(dev).eval() for _ in range(NL)]
for m in mlps:
    torch.nn.init.normal_(m.gate.weight, std=1.0)


def window(fn, xs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    n = 0
    for _ in range(ITERS):
        for x in xs:
            for m in mlps:
                fn(m, x)
                n += 1
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000 / n  # us per call


def fused(m, x):
    return m(x, decode=True)


def unfused(m, x):
    return m(x)


def op_waves(w):
    def fn(m, x):
        sel, g = ops.moe_route_topk(m.gate(x), m.top_k)
        return ops.moe_decode_mlp(x, sel, g, m.c_fc.weight, None, m.c_proj.weight, None, m.act_name, _waves=w)
    return fn


say("MoE decode MLP, bench MoE shape: E = 32, top-2, H = 1024, I = 1024, swiglu, bf16, no bias")
say("us per call of one layer's MLP (gate linear + routing + experts), device events, median of "
    f"{WINDOWS} alternating windows of {ITERS * NX * NL} calls over {NL} layers x {NX} inputs [min .. max]")
say(f"{'T':>3} {'unfused':>22} {'fused (rule)':>22} {'speedup':>8}   forced waves 1 / 2 / 4 (median)")
with torch.no_grad():
    for T in (1, 4, 16, 64):
        xs = [torch.randn(T, cfg.n_embd, device=dev, dtype=torch.bfloat16) for _ in range(NX)]
        variants = {"unfused": unfused, "fused": fused, "w1": op_waves(1), "w2": op_waves(2), "w4": op_waves(4)}
        worst = max(float((fused(mlps[0], x)[0].float() - unfused(mlps[0], x)[0].float()).abs().max()) for x in xs)
        for fn in variants.values():  # warm-up of every variant at this shape
            window(fn, xs[:2])
        t = {k: [] for k in variants}
        for _ in range(WINDOWS):
            for k, fn in variants.items():
                t[k].append(window(fn, xs))
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = lambda k: f"{med[k]:7.1f} [{min(t[k]):5.1f}..{max(t[k]):5.1f}]"
        say(f"{T:>3} {fmt('unfused'):>22} {fmt('fused'):>22} {med['unfused'] / med['fused']:7.2f}x   "
            f"{med['w1']:.1f} / {med['w2']:.1f} / {med['w4']:.1f}   max|fused - unfused| {worst:.3e}")
del mlps
torch.cuda.empty_cache()

# ---- 2. generate() end to end, B = 16, 128-token prompts, 64 new tokens
model = MoEDolomiteForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()
ids = torch.randint(0, cfg.vocab_size, (16, 128), device=dev)


def gen_tps(rows):
    MoEDolomiteBlock.decode_max_rows = rows
    model.generate(ids, max_new_tokens=8)  # warm-up
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=64)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    assert out.shape == (16, 192)
    return 16 * 64 / statistics.median(ts), out


tps_f, out_f = gen_tps(ops.MOE_DECODE_MAX_TOKENS)
tps_u, out_u = gen_tps(0)
tps_f2, _ = gen_tps(ops.MOE_DECODE_MAX_TOKENS)
say()
say("generate() end to end (prefill of 16 x 128 + 64 greedy steps, host clock around a synchronise, median of 3): "
    f"MoEDolomite-1.6B bf16, B = 16: fused decode MLP {tps_f:.0f} / {tps_f2:.0f} tokens/s (two runs), "
    f"unfused SparseMoE path {tps_u:.0f} tokens/s; {float((out_f == out_u).float().mean()) * 100:.1f}% of the "
    "tokens equal (random weights: near-ties flip)")
