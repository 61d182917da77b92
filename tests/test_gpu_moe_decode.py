"""ops.moe_decode_mlp, the pair-order routing helper and the KV cache on
MoEDolomite, on hardware.

The op is checked in bf16 against its contract in float64 from the same bf16
inputs. Its bound is not fixed in advance: on the same inputs the unfused path
(the gather, grouped GEMM, activation, grouped GEMM, gate multiply and combine
lines of SparseMoE.forward) is measured against the same reference, and the
fused op, which rounds fewer times, is allowed twice that (the factor covers
its different fp32 summation order). Shapes sit on the kernel's edges: T = 1
and T on both sides of the 16-row MFMA block, 64 rows in one expert's list,
(H, I) = (136, 88) with a partial 128-wide k tile and a partial last slab,
E = 64 with k = 8 (512 pairs: eight scan passes), idle experts.

Measured on an MI355X (printed by the tests): see DESIGN.md §7.
"""

import itertools

import pytest
import torch

from dolomite_engine_amd import ops
from dolomite_engine_amd.ops import functional as Fx
from tests.test_moe_decode_cpu import contract64, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


SHAPES = [(64, 64), (136, 88)]
ACTS = ["swiglu", "gelu_pytorch_tanh"]
PATTERNS = ["random", "same", "idle"]
# 4 x 3 (T, (E, k)) pairs, each at both shapes; activation, bias and routing pattern rotate
CASES = [
    (T, E, k, *SHAPES[j], ACTS[i % 2], bool((i // 2) % 2), PATTERNS[(2 * i + j) % 3])
    for i, (T, (E, k)) in enumerate(itertools.product([1, 3, 17, 64], [(2, 1), (8, 2), (64, 8)]))
    for j in range(2)
]


def gpu_case(T, E, k, H, I, activation, bias, pattern, seed=0):
    args = make_case(T, E, k, H, I, activation, bias, seed=seed, dtype=torch.bfloat16)
    if pattern == "same":  # every token to the same k experts: T rows in each list
        args[1] = args[1][:1].expand(T, k).contiguous()
    elif pattern == "idle":  # only the lower half of the experts is ever chosen
        g = torch.Generator().manual_seed(seed + 1)
        args[1] = torch.stack([torch.randperm(E // 2, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    return [a.cuda() if a is not None else None for a in args]


def unfused(x, selected, gates, w_fc, b_fc, w_proj, b_proj, activation):
    """The expert lines of SparseMoE.forward from a given (selected, gates)."""
    T, k = selected.shape
    flat = selected.flatten().long()
    counts = flat.bincount(minlength=w_fc.shape[0])
    _, order = flat.sort(stable=True)
    inv = torch.empty(T * k, dtype=torch.int32, device=x.device)
    inv[order] = torch.arange(T * k, dtype=torch.int32, device=x.device)
    batch_index = order // k
    h = Fx.grouped_expert_gemm(x[batch_index], w_fc, b_fc, counts)
    _, fn, glu = Fx._moe_decode_act(activation)
    h = ops.glu_activation(h, activation) if glu else fn(h)
    h = Fx.grouped_expert_gemm(h, w_proj, b_proj, counts)
    h = h * gates.flatten()[order].unsqueeze(-1)
    return Fx._rows_combine(h, inv, batch_index, T, k)


@pytest.mark.parametrize("T,E,k,H,I,activation,bias,pattern", CASES)
def test_op_matches_float64(T, E, k, H, I, activation, bias, pattern):
    args = gpu_case(T, E, k, H, I, activation, bias, pattern)
    ref = contract64(*[a.cpu() if a is not None else None for a in args], activation)
    with torch.no_grad():
        got = ops.moe_decode_mlp(*args, activation)
        again = ops.moe_decode_mlp(*args, activation)
        base = unfused(*args, activation)
    err = float((got.cpu().double() - ref).abs().max())
    err_unfused = float((base.cpu().double() - ref).abs().max())
    print(f"max|fused - f64| {err:.4e}  max|unfused - f64| {err_unfused:.4e}  bound {2 * err_unfused:.4e}")
    assert torch.equal(got, again), "two calls with the same arguments differ"
    assert err <= 2 * err_unfused


@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (17, 64, 8)])
def test_idle_experts_are_not_read(T, E, k):
    args = gpu_case(T, E, k, 136, 88, "swiglu", True, "idle")
    with torch.no_grad():
        want = ops.moe_decode_mlp(*args, "swiglu")
        idle = torch.ones(E, dtype=torch.bool, device="cuda")
        idle[args[1].flatten().long()] = False
        assert bool(idle.any())
        for i in (3, 4, 5, 6):  # w_fc, b_fc, w_proj, b_proj
            args[i] = args[i].clone()
            args[i][idle] = float("nan")
        got = ops.moe_decode_mlp(*args, "swiglu")
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_route_topk_matches_reference(dtype):
    logits = torch.randn(17, 8, generator=torch.Generator().manual_seed(3)).to(dtype)
    logits[5] = 0.25            # all tied: experts 0, 1, 2
    logits[6, [1, 4, 7]] = 3.0  # a three-way tie for the top 3
    batch_gates, _, inv, _, selected = Fx._moe_route_ref(logits, 3)
    got_selected, got_gates = ops.moe_route_topk(logits.cuda(), 3)
    assert got_selected.dtype == torch.int32 and got_gates.dtype == dtype
    assert torch.equal(got_selected.cpu(), selected)
    torch.testing.assert_close(got_gates.cpu().flatten(), batch_gates[inv.long()], rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_model_cached_logits_match_uncached(kv_dtype):
    """Prefill (70 tokens: the SparseMoE path), three decode steps and one
    4-token extend step (the fused MLP) against one uncached forward, at the
    dense model's cache tests' bf16 logits gate (rtol 1e-2 / atol 2e-2)."""
    from dolomite_engine_amd.hf_models import KVCache, MoEDolomiteConfig, MoEDolomiteForCausalLM

    torch.manual_seed(5)
    cfg = MoEDolomiteConfig(
        vocab_size=512, n_positions=256, n_embd=128, n_layer=2, n_head=2, attention_head_type="mqa",
        num_key_value_heads=1, n_inner=88, activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type="rope", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
        tie_word_embeddings=False, num_experts=8, num_experts_per_tok=2,
    )
    cfg._attn_implementation = "flash_attention_2"
    model = MoEDolomiteForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
    ids = torch.randint(0, 512, (3, 77), generator=torch.Generator().manual_seed(9)).cuda()
    worst = 0.0
    with torch.no_grad():
        want = model(input_ids=ids).logits.float()
        cache = KVCache(model.config, 3, 80, torch.bfloat16, "cuda", kv_dtype=kv_dtype)
        cache.multi_token = True  # an fp8 cache takes the flag after construction only (KVCache)
        for a, e in [(0, 70), (70, 71), (71, 72), (72, 73), (73, 77)]:
            got = model(input_ids=ids[:, a:e], past_key_values=cache, use_cache=True).logits.float()
            worst = max(worst, float((got - want[:, a:e]).abs().max()))
            torch.testing.assert_close(got, want[:, a:e], rtol=1e-2, atol=2e-2)
        out = model.generate(ids[:, :9], max_new_tokens=4, kv_cache_dtype=kv_dtype)
    print(f"max|cached - uncached logits| {worst:.4e}")
    assert cache.lengths.tolist() == [77, 77, 77] and out.shape == (3, 13)
