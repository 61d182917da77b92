"""The four kernels of csrc/moe_gemm.hip (moe_gemm_fwd / dgrad / wgrad and
moe_rows_combine), their dispatch, and the SparseMoE layer they carry, on a
real MI355X against the references of tests/moe_refs.py (pinned on CPU by
tests/test_moe_refs_cpu.py).

Grouped GEMM: small-integer inputs make every fp32 partial sum exact in any
order, so the float64 matmul cast to bf16 is the *bitwise* expectation — one
dropped or doubled element, a neighbour expert's weights on a boundary row, a
wrong fragment mapping or a narrow accumulator all change bits. The same
inputs go through the C ABI with NaN in every row, weight and guard the
kernels must neither read nor write. The combine is bitwise against the
ordered fp32 sum it documents. The layer is held to an eager bf16 baseline's
own error against float64 (see test_sparse_moe_layer_vs_float64; measured
figures in DESIGN.md §7).
"""

import functools

import pytest
import torch

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import grouped_expert_gemm, hip, hip_extension_available
from tests import moe_refs as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
GUARD = 4  # guard rows before and after every output buffer


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hip_extension_available(), "libdolomite_hip.so missing — build() must run first"


@functools.lru_cache(maxsize=None)
def _gemm_case(idx, bias):
    """(inputs, expectation) of GEMM_CASES[idx]; computed once, never modified."""
    E, N, K, counts = R.GEMM_CASES[idx]
    inp = R.int_gemm_inputs(E, N, K, counts, bias)
    return inp, R.gemm_expected(inp, counts)


def _nan_bits_like(t):
    return R.bits(torch.full(t.shape, NAN, dtype=BF16))


def _assert_bits(name, got, exp):
    g, e = R.bits(got), R.bits(exp)
    bad = g != e
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements differ bitwise, first at "
        f"{bad.nonzero()[0].tolist()}: got {got.detach().cpu()[tuple(bad.nonzero()[0])].item()} "
        f"want {exp[tuple(bad.nonzero()[0])].item()}"
    )


# ---------------------------------------------------------------------------
# a. integer-exact grouped GEMM through the dispatcher: fwd, dgrad, wgrad, db
# ---------------------------------------------------------------------------


def _run_grouped(inp, counts):
    """One fwd + bwd through grouped_expert_gemm on fresh device copies."""
    x = inp["x"].cuda().requires_grad_(True)
    w = inp["w"].cuda().requires_grad_(True)
    b = inp["b"].cuda().requires_grad_(True) if inp["b"] is not None else None
    y = grouped_expert_gemm(x, w, b, torch.tensor(counts, device="cuda"))
    assert y is not None, "HIP grouped path did not engage"
    y.backward(inp["dy"].cuda())
    torch.cuda.synchronize()
    return dict(y=y, dx=x.grad, dw=w.grad, db=None if b is None else b.grad)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("idx", range(len(R.GEMM_CASES)), ids=R.GEMM_IDS)
def test_int_gemm_bitwise(idx, bias):
    E, N, K, counts = R.GEMM_CASES[idx]
    inp, exp = _gemm_case(idx, bias)
    got = _run_grouped(inp, counts)
    again = _run_grouped(inp, counts)
    for k in ("y", "dx", "dw", "db"):
        if exp[k] is None:
            assert got[k] is None
            continue
        assert got[k].shape == exp[k].shape and got[k].is_contiguous(), k
        _assert_bits(k, got[k], exp[k])
        assert torch.equal(R.bits(got[k]), R.bits(again[k])), f"{k} differs run to run"
    for e, c in enumerate(counts):
        if c == 0:
            assert not R.bits(got["dw"][e]).any(), f"dw of empty expert {e} is not all +0"


# ---------------------------------------------------------------------------
# b. stray reads and stores, through the C ABI
# ---------------------------------------------------------------------------


def _guarded(rows, cols):
    """(buffer of GUARD + rows + GUARD rows of NaN, pointer to row GUARD)."""
    buf = torch.full((rows + 2 * GUARD, cols), NAN, dtype=BF16, device="cuda")
    return buf, hip.ptr(buf, GUARD * cols)


@pytest.mark.parametrize("idx,bias", [(1, True), (2, False)], ids=["tails-empty-mid-bias", "empty-ends-nobias"])
def test_gemm_abi_touches_only_its_rows(idx, bias):
    E, N, K, counts = R.GEMM_CASES[idx]
    inp, exp = _gemm_case(idx, bias)
    L = hip.lib()
    lead, trail = 5, 3
    T = sum(counts)
    Tb = lead + T + trail
    inside = slice(lead, lead + T)

    off = torch.tensor([lead + o for o in R._offsets(counts)], dtype=torch.int32)
    assert off[0] == 5 and off[E] == Tb - 3
    off = off.cuda()

    def padded(t):
        buf = torch.full((Tb, t.shape[1]), NAN, dtype=BF16)
        buf[inside] = t
        return buf.cuda()

    x, dy = padded(inp["x"]), padded(inp["dy"])
    w = inp["w"].clone()
    b = inp["b"].clone() if bias else None
    for e, c in enumerate(counts):
        if c == 0:  # an expert without rows: its weights must never be read
            w[e] = NAN
            if bias:
                b[e] = NAN
    w = w.cuda()
    b = b.cuda() if bias else None

    ybuf, yptr = _guarded(Tb, N)
    dxbuf, dxptr = _guarded(Tb, K)
    dwbuf, dwptr = _guarded(E * N, K)
    max_rows = max(counts)

    assert L.dolomite_moe_gemm_fwd(
        hip.stream(), hip.ptr(x), hip.ptr(w), hip.ptr(b), yptr, hip.ptr(off), E, max_rows, N, K, hip.BF16) == 0
    assert L.dolomite_moe_gemm_dgrad(
        hip.stream(), hip.ptr(dy), hip.ptr(w), dxptr, hip.ptr(off), E, max_rows, N, K, hip.BF16) == 0
    assert L.dolomite_moe_gemm_wgrad(
        hip.stream(), hip.ptr(dy), hip.ptr(x), dwptr, hip.ptr(off), E, N, K, hip.BF16) == 0
    torch.cuda.synchronize()

    for name, buf, want in (("y", ybuf, exp["y"]), ("dx", dxbuf, exp["dx"])):
        body = buf[GUARD:GUARD + Tb]
        assert not torch.isnan(body[inside]).any(), f"{name}: NaN read into a computed row"
        _assert_bits(name, body[inside], want)
        outside = torch.cat([buf[:GUARD + lead], buf[GUARD + lead + T:]])
        assert torch.equal(R.bits(outside), _nan_bits_like(outside)), f"{name}: store outside the groups"
    body = dwbuf[GUARD:GUARD + E * N].view(E, N, K)
    _assert_bits("dw", body, exp["dw"])
    outside = torch.cat([dwbuf[:GUARD], dwbuf[GUARD + E * N:]])
    assert torch.equal(R.bits(outside), _nan_bits_like(outside)), "dw: store outside (E, N, K)"


# ---------------------------------------------------------------------------
# c. moe_rows_combine, bitwise
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("T,K,k_top", R.COMBINE_CASES)
def test_rows_combine_bitwise(T, K, k_top):
    inp = R.combine_inputs(T, K, k_top)
    exp = R.combine_expected(inp["h"], inp["inv"], T, k_top)
    h, inv = inp["h"].cuda(), inp["inv"].cuda()
    L = hip.lib()

    runs = []
    for _ in range(2):
        buf, ptr = _guarded(T, K)
        assert L.dolomite_moe_rows_combine(hip.stream(), hip.ptr(h), hip.ptr(inv), ptr, T, K, k_top, hip.BF16) == 0
        torch.cuda.synchronize()
        _assert_bits("out", buf[GUARD:GUARD + T], exp)
        guards = torch.cat([buf[:GUARD], buf[GUARD + T:]])
        assert torch.equal(R.bits(guards), _nan_bits_like(guards)), "store outside out"
        runs.append(buf)
    assert torch.equal(R.bits(runs[0]), R.bits(runs[1]))

    # the op the model calls gives the same bits
    out = Fx._rows_combine(h, inv, inp["batch_index"].cuda(), T, k_top)
    _assert_bits("_rows_combine", out, exp)


def test_rows_combine_no_tokens():
    h = torch.full((4, 8), NAN, dtype=BF16, device="cuda")
    inv = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((4, 8), NAN, dtype=BF16, device="cuda")
    assert hip.lib().dolomite_moe_rows_combine(hip.stream(), hip.ptr(h), hip.ptr(inv), hip.ptr(out), 0, 8, 2, hip.BF16) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out), _nan_bits_like(out))


# ---------------------------------------------------------------------------
# d. error codes: refused before any launch
# ---------------------------------------------------------------------------


def test_error_codes():
    L = hip.lib()
    SENT = -777.0  # exact in bf16
    E, T = 2, 16
    # sized for 16 columns, so that even a launch that should not happen
    # would stay inside every buffer
    mk = lambda *shape: torch.full(shape, SENT, dtype=BF16, device="cuda")
    x, w, bias, dy = mk(T, 16), mk(E, 16, 16), mk(E, 16), mk(T, 16)
    y, dx, dw = mk(T, 16), mk(T, 16), mk(E, 16, 16)
    off = torch.tensor([0, 8, 16], dtype=torch.int32, device="cuda")
    inv = torch.zeros(T, dtype=torch.int32, device="cuda")
    out = mk(T, 16)

    def fwd(N=8, K=8, dtype=hip.BF16):
        return L.dolomite_moe_gemm_fwd(
            hip.stream(), hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(y), hip.ptr(off), E, 8, N, K, dtype)

    def dgrad(N=8, K=8, dtype=hip.BF16):
        return L.dolomite_moe_gemm_dgrad(
            hip.stream(), hip.ptr(dy), hip.ptr(w), hip.ptr(dx), hip.ptr(off), E, 8, N, K, dtype)

    def wgrad(N=8, K=8, dtype=hip.BF16):
        return L.dolomite_moe_gemm_wgrad(
            hip.stream(), hip.ptr(dy), hip.ptr(x), hip.ptr(dw), hip.ptr(off), E, N, K, dtype)

    def combine(K=8, dtype=hip.BF16):
        return L.dolomite_moe_rows_combine(hip.stream(), hip.ptr(x), hip.ptr(inv), hip.ptr(out), T // 2, K, 2, dtype)

    for fn in (fwd, dgrad, wgrad):
        assert fn(dtype=hip.F32) == 9010, fn.__name__
        assert fn(K=12) == 9020, fn.__name__
        assert fn(N=12) == 9020, fn.__name__
        assert fn(N=12, K=12) == 9020, fn.__name__
    assert combine(dtype=hip.F32) == 9010
    assert combine(K=12) == 9020
    torch.cuda.synchronize()
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("out", out)):
        assert (t == SENT).all(), f"{name} was written by a refused call"


# ---------------------------------------------------------------------------
# e. dispatch guard
# ---------------------------------------------------------------------------


def test_dispatch_refuses_fp32_parameters():
    """bf16 activations against fp32 parameters must fall back (None), never
    be computed from parameters misread as bf16."""
    E, N, K, counts = 2, 16, 16, [5, 11]
    inp = R.int_gemm_inputs(E, N, K, counts, True)
    x, num = inp["x"].cuda(), torch.tensor(counts, device="cuda")
    w, b = inp["w"].cuda(), inp["b"].cuda()
    assert grouped_expert_gemm(x, w.float(), None, num) is None
    assert grouped_expert_gemm(x, w.float(), b.float(), num) is None
    assert grouped_expert_gemm(x, w, b.float(), num) is None
    assert grouped_expert_gemm(x.float(), w, b, num) is None
    assert grouped_expert_gemm(x, w, b, num) is not None


def test_dispatch_strided_views_match_contiguous():
    """weight = w_big[:, :N] and bias = b_big[:, :N]: values and all four
    gradients are bitwise those of the contiguous copies. The views sit in
    storages twice the size, so a dense misread stays inside them."""
    idx = 1
    E, N, K, counts = R.GEMM_CASES[idx]
    inp, exp = _gemm_case(idx, True)
    g = torch.Generator().manual_seed(77)
    w_big = torch.randint(-3, 4, (E, 2 * N, K), generator=g).to(BF16)
    b_big = torch.randint(-8, 9, (E, 2 * N), generator=g).to(BF16)
    w_big[:, :N] = inp["w"]
    b_big[:, :N] = inp["b"]
    w_big = w_big.cuda().requires_grad_(True)
    b_big = b_big.cuda().requires_grad_(True)
    x = inp["x"].cuda().requires_grad_(True)

    weight, bias = w_big[:, :N], b_big[:, :N]
    assert not weight.is_contiguous() and not bias.is_contiguous()
    y = grouped_expert_gemm(x, weight, bias, torch.tensor(counts, device="cuda"))
    assert y is not None
    y.backward(inp["dy"].cuda())
    torch.cuda.synchronize()

    ref = _run_grouped(inp, counts)
    for name, got in (("y", y), ("dx", x.grad), ("dw", w_big.grad[:, :N]), ("db", b_big.grad[:, :N])):
        assert torch.equal(R.bits(got), R.bits(ref[name])), f"{name} differs from the contiguous run"
        _assert_bits(name, got, exp[name])
    assert not R.bits(w_big.grad[:, N:]).any(), "gradient leaked into the rows outside the view"
    assert not R.bits(b_big.grad[:, N:]).any()


def test_dispatch_unsupported_shapes():
    bf = lambda *s: torch.ones(*s, dtype=BF16, device="cuda")
    num = torch.tensor([4, 4], device="cuda")
    assert grouped_expert_gemm(bf(8, 12), bf(2, 8, 12), None, num) is None       # K % 8
    assert grouped_expert_gemm(bf(8, 8), bf(2, 12, 8), bf(2, 12), num) is None   # N % 8
    assert grouped_expert_gemm(bf(8, 8), bf(2, 8, 8), bf(2, 8), num) is not None
    # documented crossover: few large experts go to the per-expert loop
    assert grouped_expert_gemm(bf(2048, 8), bf(1, 8, 8), None, torch.tensor([2048], device="cuda")) is None
    assert grouped_expert_gemm(bf(2047, 8), bf(1, 8, 8), None, torch.tensor([2047], device="cuda")) is not None
    # no tokens
    y = grouped_expert_gemm(bf(0, 8), bf(2, 16, 8), bf(2, 16), torch.tensor([0, 0], device="cuda"))
    assert y is not None and y.shape == (0, 16) and y.dtype == BF16 and y.is_cuda


# ---------------------------------------------------------------------------
# f. the SparseMoE layer against the float64 restatement
# ---------------------------------------------------------------------------


def _index_add_combine(h, inv, batch_index, total_q, k_top):
    return torch.zeros(total_q, h.shape[1], dtype=h.dtype, device=h.device).index_add(0, batch_index, h)


@pytest.mark.parametrize("cfg", R.LAYER_CONFIGS, ids=R.LAYER_IDS)
def test_sparse_moe_layer_vs_float64(cfg, monkeypatch):
    """out, d hidden, d gate.weight and every expert weight / bias gradient
    of the bf16 layer on the HIP path against moe_refs.layer_ref64.

    No tolerance is fixed: err = max|got - ref64| / max|ref64| per tensor is
    measured for the HIP path and for an eager bf16 baseline on the same GPU
    (the same module with the grouped dispatcher returning None and the
    combine replaced by index_add). Both round to bf16 at the same places and
    differ only in accumulation order, so err_hip <= 2 * err_eager is asked.
    Tokens are pre-filtered (moe_refs.layer_inputs) so that bf16 logits
    cannot flip the top-k; that is asserted first."""
    E, top_k, n_embd, n_inner, act, bias, dead = cfg
    inp = R.layer_inputs(*cfg)
    assert inp["h"].shape[0] == R.LAYER_T
    ref = R.layer_ref64(inp, top_k, act)
    want_sets = R.expert_sets(ref["logits"], top_k)

    def run():
        layer = R.build_sparse_moe(inp, E, top_k, n_embd, n_inner, act, bias, BF16, "cuda")
        h = inp["h"].cuda().requires_grad_(True)
        out, logits = layer(h)
        assert torch.equal(R.expert_sets(logits.detach().cpu(), top_k), want_sets), "routing differs from float64"
        out.backward(inp["dout"].cuda())
        torch.cuda.synchronize()
        return dict(R.layer_grads(layer, h), out=out)

    engaged = []
    real = ops.grouped_expert_gemm

    def counted(*a):
        y = real(*a)
        engaged.append(y is not None)
        return y

    monkeypatch.setattr(ops, "grouped_expert_gemm", counted)
    got = run()
    assert engaged == [True, True], "c_fc / c_proj did not both run on the HIP grouped kernels"

    def refused(*a):
        engaged.append(False)

    monkeypatch.setattr(ops, "grouped_expert_gemm", refused)
    monkeypatch.setattr(Fx, "_rows_combine", _index_add_combine)
    base = run()
    assert engaged == [True, True, False, False], "the baseline did not go through the eager per-expert loop"

    assert set(got) == set(ref) - {"logits"}
    if dead is not None:
        assert not want_sets[:, dead].any()
        for k in ("fc_w", "proj_w"):
            assert not got[k][dead].any(), f"{k} gradient of the never-chosen expert is not zero"

    worse = []
    for k in sorted(got):
        e_hip, e_eager = R.rel_err(got[k], ref[k]), R.rel_err(base[k], ref[k])
        print(f"LAYERERR {R.LAYER_IDS[R.LAYER_CONFIGS.index(cfg)]} {k} hip={e_hip:.3e} eager={e_eager:.3e}")
        if not e_hip <= 2 * e_eager:
            worse.append((k, e_hip, e_eager))
    assert not worse, f"HIP error above twice the eager bf16 baseline's: {worse}"
