"""Benchmark — BASELINE.json metric: tokens/sec/node, GPTDolomite-3B bf16
seq4096 padding-free, at N GPUs of one node (config #3; at N=1 it is the
single-GPU leg of that config).

Contract: `python bench.py --gpus N --steps K --warmup W` (N>1 launched by
the driver via torch.distributed.run, one rank per GPU over RCCL). Rank 0
prints ONE JSON line with the whole-node throughput and the roofline of the
dominant hand-written kernel (measured live with HIP events inside the timed
steps). `--full` adds the oracle CPU baseline (kind "port") timed on the
host cores, which takes minutes; a plain run leaves `cpu_baseline` null.
`--dump-outputs DIR` writes what the last timed step computed (see
dump_outputs) so two builds can be compared output for output: with the
same arguments the initial weights and every batch are identical.

A "step" = one train_step: padding-free forward + backward + ZeRO-2
reduce-scatter/AdamW/all-gather on synthetic packed seq-4096 batches
(random tokens, random-init weights — no network for data/checkpoints).
"""

import argparse
import json
import os
import time

import torch

# GPTDolomite-3B (granite-3b-code-base shape; SURVEY.md §8 header)
MODEL_3B = dict(
    vocab_size=49152,
    n_positions=4096,
    n_embd=2560,
    n_layer=32,
    n_head=32,
    num_key_value_heads=None,
    attention_head_type="mqa",
    n_inner=10240,
    activation_function="gelu_pytorch_tanh",
    normalization_function="rmsnorm",
    position_embedding_type="rope",
    rope_theta=10000,
    resid_pdrop=0.0,
    embd_pdrop=0.0,
    attn_pdrop=0.0,
    layer_norm_epsilon=1e-5,
    tie_word_embeddings=True,
    bos_token_id=0,
    eos_token_id=0,
    pad_token_id=0,
)

# GPTDolomite-350M (config #2 shape: h=1024, L=24, seq 2048)
MODEL_350M = dict(
    vocab_size=49152,
    n_positions=2048,
    n_embd=1024,
    n_layer=24,
    n_head=16,
    num_key_value_heads=None,
    attention_head_type="mqa",
    n_inner=4096,
    activation_function="gelu_pytorch_tanh",
    normalization_function="rmsnorm",
    position_embedding_type="rope",
    rope_theta=10000,
    resid_pdrop=0.0,
    embd_pdrop=0.0,
    attn_pdrop=0.0,
    layer_norm_epsilon=1e-5,
    tie_word_embeddings=True,
    bos_token_id=0,
    eos_token_id=0,
    pad_token_id=0,
)

# MoE-1.6B (moe_dolomite family, §8f.3): 32 experts top-2, swiglu —
# exercises the grouped expert GEMM path end-to-end (~250M active params)
MODEL_MOE = dict(
    model_type="moe_dolomite",
    vocab_size=49152,
    n_positions=4096,
    n_embd=1024,
    n_layer=24,
    n_head=16,
    num_key_value_heads=None,
    attention_head_type="mqa",
    n_inner=1024,
    activation_function="swiglu",
    normalization_function="rmsnorm",
    position_embedding_type="rope",
    rope_theta=10000,
    resid_pdrop=0.0,
    embd_pdrop=0.0,
    attn_pdrop=0.0,
    layer_norm_epsilon=1e-5,
    tie_word_embeddings=True,
    add_bias=False,
    num_experts=32,
    num_experts_per_tok=2,
    # train the reference's actual MoE pretraining objective: CLM + the
    # mixtral load-balancing aux loss on the packed router logits
    output_router_logits=True,
    router_aux_loss_coef=0.001,
    bos_token_id=0,
    eos_token_id=0,
    pad_token_id=0,
)

# Llama-3-8B shape (config #4 class: GQA d_head=128, swiglu, seq 8192 —
# the import_from_huggingface finetune target measured at micro-batch 1)
MODEL_LLAMA8B = dict(
    vocab_size=128256,
    n_positions=8192,
    n_embd=4096,
    n_layer=32,
    n_head=32,
    num_key_value_heads=8,
    attention_head_type="gqa",
    n_inner=14336,
    activation_function="swiglu",
    normalization_function="rmsnorm",
    position_embedding_type="rope",
    rope_theta=500000,
    resid_pdrop=0.0,
    embd_pdrop=0.0,
    attn_pdrop=0.0,
    layer_norm_epsilon=1e-5,
    add_bias=False,
    tie_word_embeddings=False,
    bos_token_id=0,
    eos_token_id=0,
    pad_token_id=0,
)

MODELS = {"3b": MODEL_3B, "350m": MODEL_350M, "moe": MODEL_MOE, "llama8b": MODEL_LLAMA8B}

SEQ_LEN = 4096
MICRO_BATCH = 16  # tokens per rank per step = 16 * 4096 = 65536 (fills HBM better; +5% vs B=8)


def build(args, device):
    from dolomite_engine_amd.model_wrapper import ModelWrapperForPretraining
    from dolomite_engine_amd.zero import ZeRO2Engine

    wrapper = ModelWrapperForPretraining(
        micro_batch_size=args.micro_batch,
        sequence_length=args.seq_len,
        model_name=None,
        pretrained_config=dict(MODELS[args.model]),
        dtype="bf16" if device.type == "cuda" else "fp32",
        attention_implementation="flash_attention_2" if device.type == "cuda" else "eager",
        use_padding_free_transformer=device.type == "cuda",
        device=device,  # construct + init directly on the GPU
    )
    wrapper.model.to(device)
    engine = ZeRO2Engine(wrapper.model, lr=1e-5, betas=(0.9, 0.95), eps=1e-10, weight_decay=0.1)
    return wrapper, engine


def synth_batch(rank, step, mbs, seq_len, vocab):
    g = torch.Generator().manual_seed(1234 + 100003 * rank + step)
    return {"text": torch.randint(0, vocab, (mbs, seq_len + 1), generator=g, dtype=torch.int64)}


def run_steps(wrapper, engine, scheduler, rank, mbs, seq_len, vocab, n_steps, step0=0, clip=1.0):
    from dolomite_engine_amd.train_utils import train_step

    class _It:
        def __init__(self):
            self.i = step0

        def __next__(self):
            b = synth_batch(rank, self.i, mbs, seq_len, vocab)
            self.i += 1
            return b

    it = _It()
    results = []
    for _ in range(n_steps):
        results.append(train_step(wrapper, engine, scheduler, it, 1, clip))
    return results


DUMP_SAMPLE_PER_BUCKET = 65536  # elements sampled from each optimizer bucket
DUMP_SEED = 20240229
WEIGHT_SEED = 1234  # torch seed set before the model is built


def dump_outputs(out_dir, step_results, engine):
    """Write what the last timed train_step handed back to its caller, as
    float64/float32 .npy files: the (loss, grad_norm) it returned, the loss
    of every timed step, and the parameters it left behind. The parameters
    are read from the optimizer's fp32 master shards, not from the bf16
    model copies: at lr 1e-5 a few AdamW steps move almost no bf16 value,
    while every master value moves. They are a fixed seeded sample
    (DUMP_SAMPLE_PER_BUCKET elements per bucket of this rank's shard, same
    indices every run) so the dump stays far below 64 MB at 3B/8B."""
    import numpy

    os.makedirs(out_dir, exist_ok=True)
    last_loss, last_grad_norm = step_results[-1]
    numpy.save(os.path.join(out_dir, "loss.npy"), numpy.array([last_loss], dtype=numpy.float64))
    numpy.save(os.path.join(out_dir, "grad_norm.npy"), numpy.array([last_grad_norm], dtype=numpy.float64))
    numpy.save(
        os.path.join(out_dir, "loss_per_step.npy"),
        numpy.array([r[0] for r in step_results], dtype=numpy.float64),
    )

    g = torch.Generator().manual_seed(DUMP_SEED)
    chunks = []
    for b in engine.buckets:
        flat = b.master.detach()
        if flat.numel() > DUMP_SAMPLE_PER_BUCKET:
            idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE_PER_BUCKET,), generator=g)
            flat = flat[idx.to(flat.device)]
        chunks.append(flat.float().cpu())
    numpy.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(chunks).numpy())


def cpu_baseline(args):
    """Oracle (CPU fp32 restatement, kind='port') on a bounded sample of the
    same 3B workload, with the superlinear attention term measured AT the
    bench sequence length instead of extrapolated (round-1 weakness: pure
    512-token scaling flattered the CPU):

      t_seq(S) = (t_512 - L*t_attn1(512)) * S/512  +  L*t_attn1(S)
      t_step   = n_seqs * t_seq(S) + t_adamw

    where t_512 is one full fwd+bwd on a packed 512-token sequence, and
    t_attn1(s) times ONE layer's varlen attention fwd+bwd at length s
    directly (the only superlinear component; everything else is per-token
    linear by construction). AdamW is measured on a 1/8 param sample and
    scaled. All components measured live on this host; composition stated
    in the sample string."""
    import oracle

    torch.manual_seed(0)
    cfg = oracle.OracleConfig(
        vocab_size=MODEL_3B["vocab_size"],
        n_positions=MODEL_3B["n_positions"],
        n_embd=MODEL_3B["n_embd"],
        n_layer=MODEL_3B["n_layer"],
        n_head=MODEL_3B["n_head"],
        n_inner=MODEL_3B["n_inner"],
        attention_head_type="mqa",
        position_embedding_type="rope",
        normalization_function="rmsnorm",
        activation_function="gelu_pytorch_tanh",
        tie_word_embeddings=True,
    )
    model = oracle.OracleGPTDolomiteForCausalLM(cfg)
    with torch.no_grad():
        for p in model.parameters():
            p.uniform_(-0.02, 0.02)

    S = 512
    ids = torch.randint(0, cfg.vocab_size, (S,))
    pos = torch.arange(S)
    cu = torch.tensor([0, S], dtype=torch.int32)

    t0 = time.perf_counter()
    logits, loss = model(ids, pos, cu, S, labels=ids)
    loss.backward()
    t_fwd_bwd = time.perf_counter() - t0

    # one layer's varlen attention fwd+bwd at 512 and at the bench seq len
    H, Hkv, D = cfg.n_head, 1, cfg.n_embd // cfg.n_head
    scale = 1.0 / (D ** 0.5)

    def t_attn1(s):
        q = torch.randn(s, H, D, requires_grad=True)
        kk = torch.randn(s, Hkv, D, requires_grad=True)
        vv = torch.randn(s, Hkv, D, requires_grad=True)
        cu_s = torch.tensor([0, s], dtype=torch.int32)
        t = time.perf_counter()
        out = oracle.attention_varlen_ref(q, kk, vv, cu_s, scale)
        out.backward(torch.ones_like(out))
        return time.perf_counter() - t

    L = cfg.n_layer
    t_attn1(256)  # warm up the autograd/GEMM paths before timing
    ta_S = t_attn1(args.seq_len)
    # measure the 512 leg fully warm (thread-pool spin-up was inflating it)
    ta_512 = min(t_attn1(512), t_attn1(512))

    # AdamW on a 1/8 sample of the params, scaled up
    n_sample = 0
    t0 = time.perf_counter()
    for i, p in enumerate(model.parameters()):
        if i % 8 != 0 or p.grad is None:
            continue
        m = torch.zeros_like(p, dtype=torch.float32)
        v = torch.zeros_like(p, dtype=torch.float32)
        oracle.adamw_step_ref(p.data, p.grad, m, v, 1, 1e-5, 0.9, 0.95, 1e-10, 0.1)
        n_sample += p.numel()
    t_adamw = (time.perf_counter() - t0) * (sum(p.numel() for p in model.parameters()) / max(n_sample, 1))

    tokens_per_step = args.micro_batch * args.seq_len
    t_linear_512 = max(t_fwd_bwd - L * ta_512, 0.0)
    t_seq = t_linear_512 * (args.seq_len / S) + L * ta_S
    t_step = args.micro_batch * t_seq + t_adamw
    return {
        "value": tokens_per_step / t_step,
        "unit": "tokens/s",
        "cores": torch.get_num_threads(),
        "kind": "port",
        "sample": (
            f"oracle fp32: 1x{S}-tok seq fwd+bwd {t_fwd_bwd:.1f}s; per-layer attention "
            f"fwd+bwd measured at S=512 ({ta_512:.2f}s) and S={args.seq_len} ({ta_S:.2f}s); "
            f"linear part scaled x{args.seq_len // S}, attention taken at shape "
            f"(t_seq={t_seq:.1f}s x{args.micro_batch} seqs) + AdamW over all 3.0e9 fp32 "
            f"params (1/8 sampled, {t_adamw:.1f}s scaled)"
        ),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--micro-batch", type=int, default=None)
    ap.add_argument("--seq-len", type=int, default=None)
    ap.add_argument("--model", choices=sorted(MODELS), default="3b",
                    help="3b = BASELINE config #3 (the headline metric); 350m = config #2")
    ap.add_argument("--skip-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also time the oracle CPU baseline (minutes of host time); a plain run "
                         "only sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy")
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"
    if args.seq_len is None:
        args.seq_len = {"350m": 2048, "llama8b": 8192}.get(args.model, SEQ_LEN)
    if args.micro_batch is None:
        args.micro_batch = {"3b": MICRO_BATCH, "350m": 64, "moe": 16, "llama8b": 2}[args.model]
    fam = "moedolomite" if args.model == "moe" else "gptdolomite"

    import torch.distributed as dist

    from dolomite_engine_amd.ops import hip
    from dolomite_engine_amd.optimization import LRScheduler
    from dolomite_engine_amd.utils import init_distributed

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    init_distributed()
    assert torch.cuda.is_available(), "bench.py measures the MI355X hot path"
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)

    # same arguments -> same initial weights (the batches are seeded per step)
    torch.manual_seed(WEIGHT_SEED)
    wrapper, engine = build(args, device)
    scheduler = LRScheduler(1e-5, 0, 0, None, 10**9, "constant", 0.1)
    vocab = MODELS[args.model]["vocab_size"]

    # warmup
    run_steps(wrapper, engine, scheduler, rank, args.micro_batch, args.seq_len, vocab, args.warmup)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()

    # timed region (per-op HIP events enabled for the roofline evidence)
    hip.enable_profiling()
    t0 = time.perf_counter()
    step_results = run_steps(
        wrapper, engine, scheduler, rank, args.micro_batch, args.seq_len, vocab, args.steps, step0=args.warmup
    )
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    profile = hip.collect_profile()
    hip.disable_profiling()

    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)

    if rank != 0:
        return

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, step_results, engine)

    tokens_total = args.micro_batch * args.seq_len * args.steps * world
    value = tokens_total / elapsed
    ms_per_step = elapsed / args.steps * 1000

    # roofline of the dominant hand-written kernel (per launch, algorithmic)
    MC = MODELS[args.model]
    B, S, L = args.micro_batch, args.seq_len, MC["n_layer"]
    H, D, h = MC["n_head"], MC["n_embd"] // MC["n_head"], MC["n_embd"]
    fa_fwd_flops = 2.0 * H * D * B * S * S  # QK^T + PV, causal half x2 matmuls, per layer-launch
    fa_bwd_flops = 2.5 * fa_fwd_flops  # 5 contractions vs 2 in fwd
    flops_per_launch = {"fa_varlen_fwd": fa_fwd_flops, "fa_varlen_bwd": fa_bwd_flops}
    # per-launch HBM traffic measured in a separate rocprofv3 --pmc pass
    # (profiles/pmc_traffic.json, corrections documented there); null when
    # no calibration exists for the dominant kernel
    traffic_cal = {}
    try:
        import pathlib

        cal = json.load(open(pathlib.Path(__file__).parent / "profiles" / "pmc_traffic.json"))
        traffic_cal = cal.get("kernels", {})
    except Exception:
        pass
    roofline = None
    if profile:
        dom = max(profile, key=lambda k: profile[k]["total_ms"])
        p = profile[dom]
        if dom in flops_per_launch:
            achieved = flops_per_launch[dom] / (p["avg_ms"] / 1e3)
            tr = traffic_cal.get("fa_bwd_dkv" if dom == "fa_varlen_bwd" else dom)
            roofline = {
                "kernel": dom,
                "bound": "mfma",
                "achieved": achieved / 1e12,
                "peak": 2500.0,
                "unit": "TFLOP/s",
                "frac": achieved / 1e12 / 2500.0,
                "traffic": tr["hbm_read_bytes_per_launch"] if tr else None,
                "avg_launch_ms": p["avg_ms"],
                "launches": p["count"],
            }
        else:  # HBM-bound elementwise kernel
            bytes_map = {
                "rmsnorm_fwd": 3 * B * S * h * 2,
                "rmsnorm_bwd": 3 * B * S * h * 2,
                "ce_fwd": B * S * vocab * 2,
                "ce_bwd": 2 * B * S * vocab * 2,
            }
            bl = bytes_map.get(dom)
            achieved = bl / (p["avg_ms"] / 1e3) if bl else None
            roofline = {
                "kernel": dom,
                "bound": "hbm",
                "achieved": achieved / 1e12 if achieved else None,
                "peak": 8.0,
                "unit": "TB/s",
                "frac": achieved / 8e12 if achieved else None,
                "traffic": None,
                "avg_launch_ms": p["avg_ms"],
                "launches": p["count"],
            }

    # secondary roofline: fa_fwd alongside the dominant kernel (the bwd
    # region usually dominates; VERDICT r01 asked for both to be visible)
    roofline_fwd = None
    if profile and "fa_varlen_fwd" in profile and (roofline is None or roofline["kernel"] != "fa_varlen_fwd"):
        p = profile["fa_varlen_fwd"]
        achieved = fa_fwd_flops / (p["avg_ms"] / 1e3)
        roofline_fwd = {
            "kernel": "fa_varlen_fwd",
            "bound": "mfma",
            "achieved": achieved / 1e12,
            "peak": 2500.0,
            "unit": "TFLOP/s",
            "frac": achieved / 1e12 / 2500.0,
            "traffic": (traffic_cal.get("fa_varlen_fwd") or {}).get("hbm_read_bytes_per_launch"),
            "avg_launch_ms": p["avg_ms"],
            "launches": p["count"],
        }

    cpu = None
    if args.full and not args.skip_cpu_baseline and world == 1 and args.model == "3b":
        cpu = cpu_baseline(args)

    result = {
        "metric": (
            f"tokens/sec/node "
            f"{ {'3b': 'GPTDolomite-3B', '350m': 'GPTDolomite-350M', 'moe': 'MoEDolomite-1.6B', 'llama8b': 'Llama-3-8B-shape'}[args.model] } "
            f"bf16 seq{args.seq_len} padding-free"
        ),
        "value": value,
        "unit": "tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic",
        "config": {
            "workload": f"{fam}-{args.model}-bf16-seq{args.seq_len}-paddingfree-pretrain",
            "model": {"3b": "GPTDolomite-3B", "350m": "GPTDolomite-350M",
                      "moe": "MoEDolomite-1.6B-A0.25B", "llama8b": "Llama-3-8B-shape"}[args.model],
            "global_batch": args.micro_batch * world,
            "seq_len": args.seq_len,
            "parallelism": f"dp{world}",
        },
        "roofline": roofline,
        "roofline_fwd": roofline_fwd,
        "cpu_baseline": cpu,
        "kernel_profile": {k: {kk: round(vv, 3) if isinstance(vv, float) else vv for kk, vv in v.items()} for k, v in profile.items()},
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
