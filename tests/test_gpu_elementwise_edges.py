"""GPU edge-path tests for csrc/elementwise.hip: every kernel instantiation,
tail, bucket and rejection the friendly shapes of test_gpu_kernels.py never
reach, each against a float64 CPU computation of the same operation.

The float64 references start from the same dtype-rounded inputs and apply
the intermediate roundings include/dolomite_hip.h specifies (tensor-dtype
residual sum, RMSNorm's cast before the weight). Bounds are derived from the
roundings involved (u = one rounding of the dtype), never fitted to the
kernel (tests/elementwise_refs.py holds both, shared with the CPU tests);
each assertion prints `MAXRATIO <name> <error/bound>` first, and DESIGN.md's
test section records the measured maxima.
"""

import math

import pytest
import torch

import oracle
from dolomite_engine_amd.ops import QKVLayout, hip_extension_available
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip

from tests.elementwise_refs import (
    ADAM_HP, BF16, F32, SENTINEL, _ce_labels, _norm_inputs, _rand, _rope_bound, _rope_ref64, _rope_rounded,
    _rope_tables, _within, adamw_ref64, ce_bounds, ce_ref64, check_norm_against_ref, norm_ref64,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hip_extension_available(), "libdolomite_hip.so missing — build() must run first"


# ===========================================================================
# RMSNorm / LayerNorm
# ===========================================================================

NORM_SHAPES = [
    (8195, 64),   # grid-stride row loop: 2-3 rows per wave slot + ragged last pass
    (37, 100),    # bf16 scalar path (100 % 8 != 0)
    (37, 50),     # fp32 scalar path (50 % 4 != 0)
    (5, 1023),    # scalar path at the top bucket
    (9, 1536),    # bf16 bucket 4
    (9, 8192),    # bf16 bucket 16 (fp32 H=8192 is out of range: rejected, see below)
    (1, 8),       # partial workgroup, most lanes idle
    (2, 64),
    (3, 64),
]
NORM_CASES = [(s, d) for s in NORM_SHAPES for d in (BF16, F32) if not (d == F32 and s[1] > 4096)]


def _norm_gpu(kind, inp, eps):
    """fwd + bwd + both partial reduces straight through the C ABI (the
    autograd Functions always pass a materialized ds, so MODE 0/1 of
    norm_bwd_kernel are reachable only here)."""
    lib = hip.lib()
    dev = {k: (v.cuda() if v is not None else None) for k, v in inp.items()}
    x, w, b, dy, res, ds = (dev[k] for k in ("x", "w", "b", "dy", "res", "ds"))
    T, H = x.shape
    y = torch.empty_like(x)
    s_out = torch.empty_like(x) if res is not None else None
    rstd = torch.empty(T, dtype=F32, device="cuda")
    mean = torch.empty(T, dtype=F32, device="cuda")
    if kind == "rms":
        hip.check(lib.dolomite_rmsnorm_fwd(hip.stream(), hip.ptr(x), hip.ptr(res), hip.ptr(w), hip.ptr(y),
                                           hip.ptr(s_out), hip.ptr(rstd), T, H, eps, hip.dt(x)), "rmsnorm_fwd")
    else:
        hip.check(lib.dolomite_layernorm_fwd(hip.stream(), hip.ptr(x), hip.ptr(res), hip.ptr(w), hip.ptr(b),
                                             hip.ptr(y), hip.ptr(s_out), hip.ptr(mean), hip.ptr(rstd),
                                             T, H, eps, hip.dt(x)), "layernorm_fwd")
    s = s_out if res is not None else x
    nb = lib.dolomite_rmsnorm_bwd_nblocks(T)
    dx = torch.empty_like(x)
    partial = torch.empty((2 if kind == "ln" else 1) * nb, H, dtype=F32, device="cuda")
    if kind == "rms":
        hip.check(lib.dolomite_rmsnorm_bwd(hip.stream(), hip.ptr(dy), hip.ptr(s), hip.ptr(w), hip.ptr(rstd),
                                           hip.ptr(dx), hip.ptr(partial), hip.ptr(ds), T, H, hip.dt(x)), "rmsnorm_bwd")
    else:
        hip.check(lib.dolomite_layernorm_bwd(hip.stream(), hip.ptr(dy), hip.ptr(s), hip.ptr(w), hip.ptr(mean),
                                             hip.ptr(rstd), hip.ptr(dx), hip.ptr(partial), hip.ptr(ds),
                                             T, H, hip.dt(x)), "layernorm_bwd")
    dw = torch.full((H,), float("nan"), dtype=F32, device="cuda")  # out need not be zeroed
    hip.check(lib.dolomite_reduce_partials(hip.stream(), hip.ptr(partial), hip.ptr(dw), nb, H), "reduce")
    db = None
    if kind == "ln":
        db = torch.full((H,), float("nan"), dtype=F32, device="cuda")
        hip.check(lib.dolomite_reduce_partials(hip.stream(), hip.ptr(partial, nb * H), hip.ptr(db), nb, H), "reduce")
    torch.cuda.synchronize()
    return dict(y=y, s=s_out, rstd=rstd, mean=mean if kind == "ln" else None, dx=dx, dw=dw, db=db)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "res+ds"])
@pytest.mark.parametrize("kind", ["rms", "ln"])
@pytest.mark.parametrize("shape,dtype", NORM_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_norm_edge_shapes_vs_float64(kind, shape, dtype, fused):
    T, H = shape
    eps = 1e-5
    inp = _norm_inputs(kind, T, H, dtype, fused, seed=100 + H)
    got = _norm_gpu(kind, inp, eps)
    ref = norm_ref64(kind, inp, eps, dtype)
    tag = f"{kind}[{T}x{H},{str(dtype)[6:]},{'res' if fused else 'plain'}]"
    check_norm_against_ref(tag, kind, got, ref, dtype)
    if fused:
        assert torch.equal(got["s"].cpu(), ref["s"]), "res_out is the tensor-dtype sum x + res"


@pytest.mark.parametrize("dtype,H", [(BF16, 8200), (BF16, 1025), (F32, 1025)])
def test_norm_rejects_unsupported_width_without_launching(dtype, H):
    """Every norm entry point returns 9002 for a width beyond its largest
    ITMAX bucket, before launching anything: outputs keep their sentinel."""
    lib = hip.lib()
    T = 3
    x = torch.ones(T, H, dtype=dtype, device="cuda")
    w = torch.ones(H, dtype=dtype, device="cuda")
    stat = torch.ones(T, dtype=F32, device="cuda")
    outs = [torch.full((T, H), SENTINEL, dtype=dtype, device="cuda") for _ in range(2)]
    stats = [torch.full((T,), SENTINEL, dtype=F32, device="cuda") for _ in range(2)]
    nb = lib.dolomite_rmsnorm_bwd_nblocks(T)
    partial = torch.full((2 * nb, H), SENTINEL, dtype=F32, device="cuda")
    S, P, d = hip.stream, hip.ptr, hip.dt(x)
    calls = {
        "rmsnorm_fwd": lambda r: lib.dolomite_rmsnorm_fwd(
            S(), P(x), P(r), P(w), P(outs[0]), P(outs[1] if r is not None else None), P(stats[0]), T, H, 1e-5, d),
        "layernorm_fwd": lambda r: lib.dolomite_layernorm_fwd(
            S(), P(x), P(r), P(w), P(w), P(outs[0]), P(outs[1] if r is not None else None),
            P(stats[0]), P(stats[1]), T, H, 1e-5, d),
        "rmsnorm_bwd": lambda r: lib.dolomite_rmsnorm_bwd(
            S(), P(x), P(x), P(w), P(stat), P(outs[0]), P(partial), P(r), T, H, d),
        "layernorm_bwd": lambda r: lib.dolomite_layernorm_bwd(
            S(), P(x), P(x), P(w), P(stat), P(stat), P(outs[0]), P(partial), P(r), T, H, d),
    }
    for name, call in calls.items():
        for r in (None, x):  # without / with the residual (fwd) or dres (bwd) operand
            with pytest.raises(RuntimeError, match="9002"):
                hip.check(call(r), name)
    torch.cuda.synchronize()
    for t in outs + stats + [partial]:
        assert bool((t == SENTINEL).all())


# --- fixed-order partial reduce --------------------------------------------


@pytest.mark.parametrize("H", [64, 320])
@pytest.mark.parametrize("nblocks", [1, 128, 129, 4096])
def test_reduce_partials_fixed_order(nblocks, H):
    """dolomite_reduce_partials: bitwise run-to-run, bitwise equal to the
    CPU restatement of the documented order, close to float64, and `out`
    need not be zeroed. partial is scratch (chunk heads are overwritten), so
    every call gets a fresh upload."""
    g = torch.Generator().manual_seed(500 + nblocks + H)
    p = torch.randn(nblocks, H, generator=g) * 3.0 + 0.25
    outs = []
    for fill in (float("nan"), 0.0, 123.0):
        pd = p.cuda()
        out = torch.full((H + 3,), fill, dtype=F32, device="cuda")
        hip.check(hip.lib().dolomite_reduce_partials(hip.stream(), hip.ptr(pd), hip.ptr(out), nblocks, H), "reduce")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[1][H:], torch.zeros(3)) and torch.equal(outs[2][H:], torch.full((3,), 123.0))
    res = [o[:H] for o in outs]
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2])
    assert torch.equal(res[0], Fx.reduce_partials_ref(p)), "kernel order != documented order"
    # sequential fp32 summation: |err| <= (n-1) * 2^-24 * sum|p| (first order)
    p64 = p.double()
    _within(f"reduce[{nblocks}x{H}]", res[0], p64.sum(0), max(nblocks - 1, 1) * 2.0**-24 * p64.abs().sum(0))
    # the header's scratch contract: only chunk-head rows change
    nsplit = max(1, min(32, -(-nblocks // 128)))
    chunk = -(-nblocks // nsplit)
    keep = torch.ones(nblocks, dtype=torch.bool)
    if nsplit > 1:
        keep[::chunk] = False
    assert torch.equal(pd.cpu()[keep], p[keep])


@pytest.mark.parametrize("kind", ["rms", "ln"])
@pytest.mark.parametrize("shape", [(8195, 64), (4100, 2560)])
def test_norm_backward_bitwise_deterministic(kind, shape):
    """Norm backward twice on the same inputs -> bitwise-identical dx, dw, db
    (bit-exact resume depends on it; the atomicAdd chunk join failed this)."""
    T, H = shape
    inp = _norm_inputs(kind, T, H, BF16, True, seed=77)
    runs = []
    for _ in range(2):
        x, r, w = (inp[k].cuda().requires_grad_(True) for k in ("x", "res", "w"))
        if kind == "rms":
            params = [x, r, w]
            y, s = Fx.fused_rmsnorm(x, w, 1e-5, residual=r)
        else:
            b = inp["b"].cuda().requires_grad_(True)
            params = [x, r, w, b]
            y, s = Fx.fused_layernorm(x, w, b, 1e-5, residual=r)
        torch.autograd.backward([y, s], [inp["dy"].cuda(), inp["ds"].cuda()])
        torch.cuda.synchronize()
        runs.append([p.grad.clone() for p in params])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


# ===========================================================================
# RoPE on the packed layout
# ===========================================================================

ROPE_LAYOUTS = [("mha", 2, 2, 24), ("gqa", 4, 2, 40), ("mqa", 3, 1, 8)]  # scalar kernel: (D/2) % 8 != 0
ROPE_CASES = [(lo, d) for lo in ROPE_LAYOUTS for d in (BF16, F32)] + [(("gqa", 4, 2, 64), F32)]  # + fp32 vec8
ROPE_T = 19


def _rope_call(qin, qout, cos_g, sin_g, lo, direction, D=None):
    return hip.lib().dolomite_rope_qkv(
        hip.stream(), hip.ptr(qin), hip.ptr(qout), hip.ptr(cos_g), hip.ptr(sin_g),
        qin.shape[0], lo.row_len, lo.H, lo.Hkv, lo.D if D is None else D, lo.G,
        lo.q_gstride, lo.k_off, lo.kv_hstride, direction, 0, hip.dt(qin))


@pytest.mark.parametrize("layout,dtype", ROPE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_rope_scalar_and_fp32_paths_vs_float64(layout, dtype):
    head_type, H, Hkv, D = layout
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(40 + D)
    T = ROPE_T
    cos, sin = _rope_tables(D, T)
    cos_g, sin_g = cos.cuda(), sin.cuda()
    qkv = _rand(g, (T, lo.row_len), dtype, 1.0, 0.2)
    ref64, mag = _rope_ref64(qkv, cos, sin, lo, +1.0)
    bound = _rope_bound(ref64, mag, dtype)
    tag = f"rope[{head_type},D={D},{str(dtype)[6:]}]"

    inplace = qkv.cuda()
    hip.check(_rope_call(inplace, inplace, cos_g, sin_g, lo, +1), "rope in place")
    torch.cuda.synchronize()
    _within(f"{tag}.inplace", inplace, _rope_rounded(ref64, dtype), bound)

    # out of place: q,k slots rotated; v slots of qkv_out are NOT written
    # (header contract) and the input is left alone
    src = qkv.cuda()
    dst = torch.full_like(src, SENTINEL)
    hip.check(_rope_call(src, dst, cos_g, sin_g, lo, +1), "rope out of place")
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), qkv)
    is_v = (mag == 0)
    assert is_v.sum() == T * lo.Hkv * D
    dst_c, inpl_c = dst.cpu(), inplace.cpu()
    assert torch.equal(dst_c[~is_v], inpl_c[~is_v])
    assert bool((dst_c[is_v] == SENTINEL).all())


@pytest.mark.parametrize("sliced", [False, True], ids=["own", "rowslice"])
@pytest.mark.parametrize("layout,dtype", ROPE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_rope_autograd_backward_vs_float64_and_leaves_dout_alone(layout, dtype, sliced):
    """`rowslice`: the incoming grad is rows [3, 3+T) of a larger sentinel
    buffer — contiguous with a non-zero storage offset, so the backward must
    address it relative to the tensor, not to its storage."""
    head_type, H, Hkv, D = layout
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(60 + D)
    T = ROPE_T
    cos, sin = _rope_tables(D, T)
    qkv = _rand(g, (T, lo.row_len), dtype, 1.0, 0.2)
    dout = _rand(g, (T, lo.row_len), dtype, 0.8, -0.1)

    base = qkv.cuda().requires_grad_(True)
    out = Fx.RoPEPackedQKV.apply(base.clone(), cos.cuda(), sin.cuda(), lo)
    if sliced:
        big = torch.full((T + 5, lo.row_len), SENTINEL, dtype=dtype)
        big[3:3 + T] = dout
        big_g = big.cuda()
        dout_g = big_g[3:3 + T]
        assert dout_g.is_contiguous() and dout_g.storage_offset() == 3 * lo.row_len
    else:
        dout_g = dout.cuda()
    out.backward(dout_g)
    torch.cuda.synchronize()
    assert torch.equal(dout_g.cpu(), dout), "backward rotated the caller's grad tensor in place"
    if sliced:
        assert torch.equal(big_g.cpu(), big)

    # float64 autograd of the oracle rotation, head by head
    x64 = qkv.double().requires_grad_(True)
    q, k, v = lo.unpack_cpu(x64)
    dq, dk, dv = lo.unpack_cpu(dout.double())
    c64, s64 = cos.double(), sin.double()
    loss = (v * dv).sum()
    for h in range(H):
        loss = loss + (oracle.apply_rope_ref(q[:, h], c64, s64) * dq[:, h]).sum()
    for j in range(Hkv):
        loss = loss + (oracle.apply_rope_ref(k[:, j], c64, s64) * dk[:, j]).sum()
    loss.backward()

    # same bound as the forward, on the incoming-gradient pairs
    inv64, mag = _rope_ref64(dout, cos, sin, lo, -1.0)
    torch.testing.assert_close(inv64, x64.grad, rtol=1e-12, atol=1e-12)  # inverse rotation IS the gradient
    _within(f"rope_bwd[{head_type},D={D},{str(dtype)[6:]}]", base.grad,
            _rope_rounded(x64.grad, dtype), _rope_bound(x64.grad, mag, dtype))


def test_rope_rejects_odd_head_dim():
    lo = QKVLayout.make(2, 2, 8, "mha")
    buf = torch.full((4, lo.row_len), SENTINEL, dtype=BF16, device="cuda")
    tab = torch.ones(4, 8, dtype=F32, device="cuda")
    with pytest.raises(RuntimeError, match="9003"):
        hip.check(_rope_call(buf, buf, tab, tab, lo, +1, D=7), "rope odd D")
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ===========================================================================
# Cross entropy
# ===========================================================================

CE_SHAPES = [(5, 100), (7, 1001), (7, 1002), (3, 50257)]


def _ce_abi_fwd(lg, labels_g):
    T, V = lg.shape
    row_loss = torch.full((T,), float("nan"), dtype=F32, device="cuda")
    lse = torch.full((T,), float("nan"), dtype=F32, device="cuda")
    hip.check(hip.lib().dolomite_ce_fwd(hip.stream(), hip.ptr(lg), hip.ptr(labels_g), hip.ptr(row_loss),
                                        hip.ptr(lse), T, V, lg.stride(0), -100, hip.dt(lg)), "ce_fwd")
    return row_loss, lse


def _ce_check(tag, lg_leaf, labels, ref, dtype):
    """lg_leaf: CUDA leaf (possibly a row-strided view). Checks lse and row
    loss through the ABI, the mean loss and dlogits through autograd."""
    b = ce_bounds(ref, dtype)
    labels_g = labels.cuda()
    row_loss, lse = _ce_abi_fwd(lg_leaf.detach(), labels_g)
    loss = Fx.fused_cross_entropy(lg_leaf, labels_g)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(lg_leaf.grad).all())
    _within(f"{tag}.lse", lse, ref["lse"], b["lse"])
    _within(f"{tag}.row_loss", row_loss, ref["row_loss"], b["row_loss"])
    _within(f"{tag}.loss", loss, ref["loss"], torch.tensor(b["loss"], dtype=torch.float64))
    assert lg_leaf.grad.shape == lg_leaf.shape
    _within(f"{tag}.dlogits", lg_leaf.grad, ref["dlogits"], b["dlogits"])


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("TV", CE_SHAPES + [(5, 104)], ids=str)
def test_cross_entropy_edge_shapes_vs_float64(TV, dtype, strided):
    """V % 8 / V % 4 tails (scalar kernels), V < 256 (idle threads), labels
    at column 0 / V-1 / ignored rows; `strided` runs logits = buf[:, :V] of
    a (T, V+24) sentinel buffer, whose pad columns must survive."""
    T, V = TV
    g = torch.Generator().manual_seed(700 + V)
    logits = _rand(g, (T, V), dtype, 2.0, 0.5)
    labels = _ce_labels(g, T, V)
    ref = ce_ref64(logits, labels)
    tag = f"ce[{T}x{V},{str(dtype)[6:]},{'strided' if strided else 'dense'}]"
    if not strided:
        _ce_check(tag, logits.cuda().requires_grad_(True), labels, ref, dtype)
        return
    buf = torch.full((T, V + 24), SENTINEL, dtype=dtype)
    buf[:, :V] = logits
    buf_g = buf.cuda()
    lg = buf_g[:, :V].detach().requires_grad_(True)
    assert lg.stride(0) == V + 24 and lg.data_ptr() == buf_g.data_ptr()
    _ce_check(tag, lg, labels, ref, dtype)
    assert torch.equal(buf_g.cpu(), buf), "logits buffer (pad columns included) must be unchanged"


@pytest.mark.parametrize("V", [1000, 1001])
def test_cross_entropy_large_magnitude(V):
    """60*randn logits plus one row with a single +3e4 entry: finite and
    equal to float64 only with the running-max rescale in place."""
    g = torch.Generator().manual_seed(800 + V)
    T = 6
    logits = _rand(g, (T, V), BF16, 60.0, 5.0)
    logits[3, V // 3] = 3e4
    labels = _ce_labels(g, T, V)
    labels[3] = 7  # a column other than the spike: loss ~ 3e4
    ref = ce_ref64(logits, labels)
    _ce_check(f"ce_large[{V}]", logits.cuda().requires_grad_(True), labels, ref, BF16)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1001, 1024])
def test_cross_entropy_backward_in_place_through_abi(V, dtype):
    """dolomite_ce_bwd with dlogits == logits equals the out-of-place call
    bitwise (the header allows the alias)."""
    g = torch.Generator().manual_seed(900 + V)
    T = 7
    logits = _rand(g, (T, V), dtype, 2.0, 0.5).cuda()
    labels = _ce_labels(g, T, V).cuda()
    _, lse = _ce_abi_fwd(logits, labels)
    gs = torch.tensor([0.125], dtype=F32, device="cuda")
    oop = torch.full_like(logits, SENTINEL)
    inp = logits.clone()
    for src, dst in ((logits, oop), (inp, inp)):
        hip.check(hip.lib().dolomite_ce_bwd(hip.stream(), hip.ptr(src), hip.ptr(labels), hip.ptr(lse), hip.ptr(dst),
                                            hip.ptr(gs), T, V, V, -100, hip.dt(src)), "ce_bwd")
    torch.cuda.synchronize()
    assert not bool((oop == SENTINEL).any())
    assert torch.equal(inp, oop)


# ===========================================================================
# AdamW
# ===========================================================================



@pytest.mark.parametrize("use_scale", [False, True], ids=["noscale", "gradscale"])
@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["g_bf16", "g_fp32"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 262147])
def test_adamw_five_steps_vs_float64(n, gdtype, use_scale):
    g = torch.Generator().manual_seed(1000 + n)
    steps = 5
    p0 = _rand(g, (n,), F32, 1.0, 0.1)
    grads = [_rand(g, (n,), gdtype, 0.5, 0.05) for _ in range(steps)]
    coef = torch.tensor(0.3725, dtype=F32)
    ref = adamw_ref64(p0, grads, float(coef) if use_scale else 1.0, steps, ADAM_HP)
    hp = ADAM_HP

    def run(with_out):
        p = p0.cuda()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        pout = torch.full((n,), SENTINEL, dtype=BF16, device="cuda") if with_out else None
        for t in range(1, steps + 1):
            Fx.adamw_step_flat(p, grads[t - 1].cuda(), m, v, t, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"],
                               param_out=pout, grad_scale=coef.cuda() if use_scale else None)
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu(), None if pout is None else pout.cpu()

    p, m, v, pout = run(True)
    tag = f"adamw[n={n},{str(gdtype)[6:]},{'gs' if use_scale else 'nogs'}]"
    _within(f"{tag}.p", p, ref["p"], ref["tol_p"])
    _within(f"{tag}.m", m, ref["m"], ref["tol_m"])
    _within(f"{tag}.v", v, ref["v"], ref["tol_v"])
    assert torch.equal(pout, p.to(BF16)), "param_out must be the bf16 rounding of the updated master"
    p2, m2, v2, _ = run(False)  # param_out = NULL: same master and moments
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)


def test_adamw_zero_elements_touches_nothing():
    bufs = [torch.full((8,), SENTINEL, dtype=F32, device="cuda") for _ in range(4)]
    pout = torch.full((8,), SENTINEL, dtype=BF16, device="cuda")
    p, grad, m, v = bufs
    hip.check(hip.lib().dolomite_adamw_step(hip.stream(), hip.ptr(p), hip.ptr(pout), hip.ptr(grad), hip.F32,
                                            hip.ptr(m), hip.ptr(v), 0, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1, hip.ptr(None)),
              "adamw n=0")
    torch.cuda.synchronize()
    for t in bufs + [pout]:
        assert bool((t == SENTINEL).all())


# ===========================================================================
# sqsum / scale_inplace
# ===========================================================================


def _sqsum(x, n):
    partials = torch.empty(1024, dtype=F32, device="cuda")
    out = torch.full((2,), SENTINEL, dtype=F32, device="cuda")
    hip.check(hip.lib().dolomite_sqsum(hip.stream(), hip.ptr(x), n, hip.ptr(partials), hip.ptr(out), hip.dt(x)), "sqsum")
    torch.cuda.synchronize()
    assert float(out[1]) == SENTINEL
    return out[0].cpu()


@pytest.mark.parametrize("n", [0, 7, 8, 2_097_152, 2_097_153, 4_200_011])
def test_sqsum_tails_and_second_grid_stride_pass(n):
    """n > 1024*256*8 = 2,097,152 enters the second grid-stride iteration.
    Inputs are bf16-representable, so the bf16 and the fp32 instantiation
    see the same values in the same order and must agree BITWISE.
    Bound: every term is positive and passes at most 3*8 per-thread adds +
    8 + 10 tree steps + its square = 43 fp32 roundings; as a worst case
    that is 43*2^-24 = 2.6e-6, looser than the existing sqsum test's 1e-6,
    so 1e-6 relative is kept (round-off of random sign grows as
    sqrt(43)*2^-24 = 3.9e-7, inside it)."""
    g = torch.Generator().manual_seed(1200)
    xb = (torch.randn(n + 5, generator=g) * 0.1 + 0.01).to(BF16)  # 5 extra: must not be read into the sum
    ref = xb[:n].double().pow(2).sum()
    out_b = _sqsum(xb.cuda(), n)
    out_f = _sqsum(xb.float().cuda(), n)
    assert torch.equal(out_b, out_f), "bf16 and fp32 sqsum must agree bitwise on bf16-representable data"
    _within(f"sqsum[n={n}]", out_b, ref, 1e-6 * ref.abs() if n else torch.tensor(0.0, dtype=torch.float64))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [0, 1, 5, 1024, 100_003])
def test_scale_inplace_exact_and_bounded(n, dtype):
    """(x.double() * s) rounded once to the dtype, exactly: for fp32 the
    kernel's product is the correctly rounded one; for bf16 s is chosen
    bf16-representable, so the fp32 product of two 8-bit significands is
    exact and the store is the only rounding. Elements past n stay put."""
    g = torch.Generator().manual_seed(1300 + n)
    s = float(torch.tensor(0.3725, dtype=dtype))
    x = _rand(g, (n + 13,), dtype, 3.0, 0.4)
    xd = x.cuda()
    hip.check(hip.lib().dolomite_scale_inplace(hip.stream(), hip.ptr(xd), n, s, hip.dt(xd)), "scale")
    torch.cuda.synchronize()
    got = xd.cpu()
    assert torch.equal(got[:n], (x[:n].double() * s).to(dtype))
    assert torch.equal(got[n:], x[n:])
