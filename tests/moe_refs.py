"""References and input builders for the MoE kernels (csrc/moe_gemm.hip),
shared by tests/test_gpu_moe_kernels.py (HIP kernels on hardware) and
tests/test_moe_refs_cpu.py (which pins these references against a second,
independent statement). Pure CPU torch; nothing here touches a GPU, and no
reference uses project code (build_sparse_moe, at the end, only builds the
module under test from the same parameters).

Three references:

* grouped GEMM on small-integer inputs — every fp32 partial sum is an exactly
  representable integer in any accumulation order, so the kernel's only
  rounding is the final fp32 -> bf16 store and the float64 matmul cast to
  bf16 is the bitwise expectation;
* rows combine — an fp32 sum over j = 0..k_top-1 in that order, cast to bf16
  once, which is what the kernel states it does;
* the SparseMoE layer — per token, out[t] = sum over the top-k experts of
  softmax_k(logits[t])[e] * MLP_e(h[t]) in float64, without the expert sort.
"""

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16

# ---------------------------------------------------------------------------
# grouped GEMM, integer-exact
# ---------------------------------------------------------------------------

# (E, N, K, counts)
GEMM_CASES = [
    (3, 8, 8, [1, 129, 63]),            # minimal dims, a one-row expert
    (4, 72, 520, [65, 0, 300, 64]),     # N tail 8, K tail 8 after 8 chunks, empty middle, 5 wgrad row chunks
    (5, 136, 72, [0, 64, 0, 191, 0]),   # leading, trailing, consecutive empty experts
    (2, 192, 128, [257, 255]),          # second expert starts one row past a 64-row tile
    (33, 64, 64, [i % 3 for i in range(33)]),  # E > 32, many one- and zero-row experts
]
GEMM_IDS = ["min8", "tails-empty-mid", "empty-ends", "tile-plus-1", "e33"]


def int_gemm_inputs(E, N, K, counts, bias, seed=0):
    """x, w, dy integers in [-3, 3], bias in [-8, 8], all bf16 (exact)."""
    g = torch.Generator().manual_seed(1000 + seed)
    T = sum(counts)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).to(BF16)
    return dict(
        x=ri(-3, 3, (T, K)),
        w=ri(-3, 3, (E, N, K)),
        b=ri(-8, 8, (E, N)) if bias else None,
        dy=ri(-3, 3, (T, N)),
    )


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def gemm_expected(inp, counts, acc=torch.float64):
    """Per-expert matmuls accumulated in `acc`, each result cast to bf16 once.
    float64 is the reference; float32 is the second statement (the integers
    make both exact before the cast)."""
    x, w, b, dy = (None if inp[k] is None else inp[k].to(acc) for k in ("x", "w", "b", "dy"))
    off = _offsets(counts)
    E, N, K = w.shape
    y, dx = torch.zeros(x.shape[0], N, dtype=acc), torch.zeros(x.shape[0], K, dtype=acc)
    dw, db = torch.zeros(E, N, K, dtype=acc), torch.zeros(E, N, dtype=acc)
    for e in range(E):
        s = slice(off[e], off[e + 1])
        y[s] = x[s] @ w[e].T
        if b is not None:
            y[s] += b[e]
        dx[s] = dy[s] @ w[e]
        dw[e] = dy[s].T @ x[s]
        db[e] = dy[s].sum(0)
    # A sum that comes to zero is +0: an accumulator starts at +0, and in
    # round-to-nearest +0 + (-0) and x + (-x) are both +0. A lone product
    # such as (-1) * 0 is -0 in the matmuls above (the one-row experts), so
    # add +0 as an accumulator would.
    out = dict(y=(y + 0.0).to(BF16), dx=(dx + 0.0).to(BF16), dw=(dw + 0.0).to(BF16))
    out["db"] = (db + 0.0).to(BF16) if b is not None else None
    return out


def gemm_sum_bounds(inp, counts):
    """Largest possible |partial sum| of each product, in any accumulation
    order: the sum of the |terms|. (y, dx, dw, db)"""
    x, w, dy = (inp[k].double().abs() for k in ("x", "w", "dy"))
    b = None if inp["b"] is None else inp["b"].double().abs()
    off = _offsets(counts)
    ymax = dxmax = dwmax = dbmax = 0.0
    for e in range(w.shape[0]):
        s = slice(off[e], off[e + 1])
        if off[e] == off[e + 1]:
            continue
        ye = x[s] @ w[e].T + (0 if b is None else b[e])
        ymax = max(ymax, float(ye.max()))
        dxmax = max(dxmax, float((dy[s] @ w[e]).max()))
        dwmax = max(dwmax, float((dy[s].T @ x[s]).max()))
        dbmax = max(dbmax, float(dy[s].sum(0).max()))
    return ymax, dxmax, dwmax, dbmax


def bits(t):
    """bf16 tensor -> its int16 bit patterns (so +0 != -0 and NaN == NaN)."""
    assert t.dtype == BF16
    return t.detach().cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# rows combine
# ---------------------------------------------------------------------------

# (T, K, k_top)
COMBINE_CASES = [(1, 8, 1), (31, 72, 3), (257, 1024, 2), (1337, 64, 8)]


def combine_inputs(T, K, k_top, seed=0, E=8):
    """Random bf16 h over the T*k_top expert-sorted slots; inv/batch_index
    from a random expert selection, as SparseMoE builds them."""
    g = torch.Generator().manual_seed(2000 + seed)
    selected = torch.randint(0, E, (T, k_top), generator=g).flatten()
    _, sorted_idx = selected.sort(0)
    n = T * k_top
    inv = torch.empty(n, dtype=torch.int32)
    inv[sorted_idx] = torch.arange(n, dtype=torch.int32)
    h = (torch.randn(n, K, generator=g) * 0.5).to(BF16)
    return dict(h=h, inv=inv, batch_index=sorted_idx // k_top)


def combine_expected(h, inv, T, k_top):
    """out[t] = bf16(fp32 sum over j = 0..k_top-1, in that order, of
    h[inv[t*k_top + j]])."""
    acc = torch.zeros(T, h.shape[1], dtype=torch.float32)
    slots = inv.long().view(T, k_top)
    for j in range(k_top):
        acc = acc + h[slots[:, j]].float()
    return acc.to(BF16)


# ---------------------------------------------------------------------------
# SparseMoE layer
# ---------------------------------------------------------------------------

# (E, top_k, n_embd, n_inner, activation, bias, dead expert or None)
LAYER_CONFIGS = [
    (8, 2, 64, 72, "swiglu", False, 5),
    (4, 1, 64, 72, "gelu", True, None),
    (5, 3, 128, 40, "swiglu", True, None),
]
LAYER_IDS = ["e8k2-swiglu-dead5", "e4k1-gelu-bias", "e5k3-swiglu-bias"]
LAYER_T = 300
LAYER_CANDIDATES = 512
MIN_GAP = 0.125     # k-th minus (k+1)-th logit, float64
MAX_LOGIT = 8.0
DEAD_LOGIT = -6.0


def _act(name):
    # restated here on purpose (no project code): swiglu gates with silu,
    # gelu is the erf form
    return {"swiglu": (F.silu, True), "gelu": (F.gelu, False)}[name]


def layer_inputs(E, top_k, n_embd, n_inner, act, bias, dead, seed=0):
    """bf16-rounded parameters, tokens and output gradient for one SparseMoE
    layer, all CPU bf16. Tokens are the first LAYER_T of LAYER_CANDIDATES
    draws whose float64 routing is safe from bf16 near-tie flips; `n_kept`
    says how many candidates passed.

    With `dead` set, feature 0 of every token is 1 and that expert's gate row
    is DEAD_LOGIT on feature 0 and zero elsewhere: its logit is DEAD_LOGIT
    for every token, 3 sigma below the others', so it is never chosen."""
    g = torch.Generator().manual_seed(3000 + seed)
    rn = lambda shape, std: (torch.randn(*shape, generator=g) * std).to(BF16)
    _, glu = _act(act)
    n_fc = 2 * n_inner if glu else n_inner
    p = dict(
        gate=rn((E, n_embd), 0.25),
        fc_w=rn((E, n_fc, n_embd), n_embd**-0.5),
        fc_b=rn((E, n_fc), 0.1) if bias else None,
        proj_w=rn((E, n_embd, n_inner), n_inner**-0.5),
        proj_b=rn((E, n_embd), 0.1) if bias else None,
    )
    cand = rn((LAYER_CANDIDATES, n_embd), 1.0)
    if dead is not None:
        cand[:, 0] = 1.0
        p["gate"][dead] = 0.0
        p["gate"][dead, 0] = DEAD_LOGIT
    logits = cand.double() @ p["gate"].double().T
    top = logits.sort(dim=-1, descending=True).values
    ok = (logits.abs().amax(-1) <= MAX_LOGIT)
    if top_k < E:
        ok &= (top[:, top_k - 1] - top[:, top_k]) >= MIN_GAP
    kept = ok.nonzero().flatten()
    h = cand[kept[:LAYER_T]].clone()
    dout = rn((h.shape[0], n_embd), 1.0)
    return dict(params=p, h=h, dout=dout, n_kept=int(kept.numel()), logits64=logits[kept[:LAYER_T]])


def expert_sets(logits, top_k):
    """(T, E) bool membership of each token's top-k set."""
    idx = logits.double().topk(top_k, dim=-1).indices
    return torch.zeros_like(logits, dtype=torch.bool).scatter_(1, idx.cpu(), True)


def layer_ref64(inp, top_k, act):
    """float64 SparseMoE forward + autograd backward of sum(out * dout).
    Returns out and the gradients, keyed like layer_inputs' params."""
    fn, glu = _act(act)
    p = {k: (None if v is None else v.double().requires_grad_(True)) for k, v in inp["params"].items()}
    h = inp["h"].double().requires_grad_(True)
    E = p["gate"].shape[0]
    logits = h @ p["gate"].T
    vals, idx = logits.topk(top_k, dim=-1)
    gates = torch.softmax(vals, dim=-1)
    out = torch.zeros_like(h)
    for e in range(E):
        hit = idx == e                       # (T, k): at most one True per row
        tok = hit.any(-1).nonzero().flatten()
        if tok.numel() == 0:
            continue
        ge = (gates * hit).sum(-1)[tok]
        z = h[tok] @ p["fc_w"][e].T
        if p["fc_b"] is not None:
            z = z + p["fc_b"][e]
        if glu:
            a, b = z.chunk(2, dim=-1)
            z = a * fn(b)
        else:
            z = fn(z)
        y = z @ p["proj_w"][e].T
        if p["proj_b"] is not None:
            y = y + p["proj_b"][e]
        out = out.index_add(0, tok, ge.unsqueeze(-1) * y)
    (out * inp["dout"].double()).sum().backward()
    res = dict(out=out.detach(), h=h.grad, logits=logits.detach())
    for k, v in p.items():
        if v is not None:
            res[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return res


def rel_err(got, ref):
    """max|got - ref| / max|ref| (NaN in got -> inf). A reference that is
    identically zero (d gate.weight for top_k = 1: a softmax over one logit
    is the constant 1) gives max|got|, so only an exact zero scores 0."""
    d = (got.detach().cpu().double() - ref).abs()
    d = torch.nan_to_num(d, nan=float("inf"))
    scale = float(ref.abs().max())
    return float(d.max()) / (scale if scale > 0 else 1.0)


def build_sparse_moe(inp, E, top_k, n_embd, n_inner, act, bias, dtype, device="cpu"):
    """The project's SparseMoE (the module under test, not a reference) with
    layer_inputs' parameters."""
    from dolomite_engine_amd.hf_models.moe import MoEDolomiteConfig, SparseMoE

    cfg = MoEDolomiteConfig(
        num_experts=E, num_experts_per_tok=top_k, n_embd=n_embd, n_inner=n_inner, n_layer=1, n_head=1,
        activation_function=act, add_bias=bias, resid_pdrop=0.0,
    )
    layer = SparseMoE(cfg)
    p = inp["params"]
    with torch.no_grad():
        layer.gate.weight.copy_(p["gate"])
        layer.c_fc.weight.copy_(p["fc_w"])
        layer.c_proj.weight.copy_(p["proj_w"])
        if bias:
            layer.c_fc.bias.copy_(p["fc_b"])
            layer.c_proj.bias.copy_(p["proj_b"])
    return layer.to(dtype=dtype, device=device)


def layer_grads(layer, h):
    """Gradients of a built layer, keyed like layer_ref64's result."""
    g = dict(h=h.grad, gate=layer.gate.weight.grad, fc_w=layer.c_fc.weight.grad, proj_w=layer.c_proj.weight.grad)
    if layer.c_fc.bias is not None:
        g.update(fc_b=layer.c_fc.bias.grad, proj_b=layer.c_proj.bias.grad)
    return g
