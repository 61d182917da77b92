"""csrc/moe_route.hip on a real MI355X: selection and the stable expert sort
exact against the CPU restatement, gates and backward against float64 within
one rounding to the dtype, the layer against the torch routing chain's error."""

import functools

import pytest
import torch

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip, hip_extension_available
from tests import moe_refs as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD, SENT = 64, -7777  # guard elements around every ABI buffer; their fill for int buffers (NaN for floats)
TILE = 128               # tokens per tile of the kernels
EK = [(8, 2), (5, 3), (32, 2), (64, 8), (33, 1), (4, 4)]


def _group(E):  # lanes per token: the next power of two >= E, at least 2
    return max(2, 1 << (E - 1).bit_length())


# T: 1, a wave's token count -+ 1, one tile -+ 1, three tiles + 1; plus two skewed routings
CASES = [(T, E, k, None) for E, k in EK
         for T in sorted({1, 64 // _group(E) - 1, 64 // _group(E) + 1, TILE - 1, TILE + 1, 3 * TILE + 1} - {0})]
CASES += [(3 * TILE + 1, 8, 2, "same"), (3 * TILE + 1, 5, 3, "dead")]


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hip_extension_available(), "libdolomite_hip.so missing — build() must run first"


@functools.lru_cache(maxsize=None)
def _logits(T, E, k, skew, dtype):
    """Random logits (a jittered 2^-3 grid, scaled by 1 or 2 per row) quantised
    to dtype, a row redrawn until its sorted float64 values are >= 2^-4 apart.
    "same": experts 1..k lead every row; "dead": the last expert is never chosen."""
    g = torch.Generator().manual_seed(T * 100 + E)
    boost = torch.zeros(E)
    boost[1:k + 1] = 4.0 if skew == "same" else 0.0
    boost[E - 1] = -4.0 if skew == "dead" else boost[E - 1]
    out, todo = torch.empty(T, E, dtype=dtype), torch.arange(T)
    while todo.numel():
        n = todo.numel()
        x = (torch.rand(n, E, generator=g).argsort(-1) - E / 2) * 2**-3 + torch.rand(n, E, generator=g) * 2**-5
        x = (x * torch.randint(1, 3, (n, 1), generator=g) + boost).to(dtype)
        ok = (x.double().sort(-1).values.diff(dim=-1) >= 2**-4).all(-1)
        out[todo[ok]], todo = x[ok], todo[~ok]
    return out


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan") if dtype.is_floating_point else SENT, dtype=dtype, device="cuda")
    return buf, hip.ptr(buf, GUARD)


def _untouched(buf, n):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((g.isnan() if buf.dtype.is_floating_point else g == SENT).all())


def _route_abi(logits, k, want=0):
    """dolomite_moe_route_fwd on guarded buffers -> dict of the outputs."""
    T, E = logits.shape
    L, dt = hip.lib(), logits.dtype
    n_scr = max(int(L.dolomite_moe_route_scratch_ints(max(T, 1), min(E, 64), min(k, 8, E))), 1)
    spec = dict(selected=(T * k, torch.int32), gates=(T * k, dt), inv=(T * k, torch.int32), batch_index=(T * k, torch.int64),
                batch_gates=(T * k, dt), num=(E, torch.int64), offsets=(E + 1, torch.int32), scratch=(n_scr, torch.int32))
    bufs = {name: _guarded(n, d) for name, (n, d) in spec.items()}
    ret = L.dolomite_moe_route_fwd(hip.stream(), hip.ptr(logits), *(p for _, p in bufs.values()), T, E, k,
                                   hip.dt(logits) if dt.is_floating_point else 2)
    torch.cuda.synchronize()
    assert ret == want, ret
    for name, (buf, _) in bufs.items():
        assert _untouched(buf, spec[name][0]), f"{name}: store outside the buffer"
    return {name: buf[GUARD:GUARD + spec[name][0]] for name, (buf, _) in bufs.items()}


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T,E,k,skew", CASES)
def test_route_exact_and_gates(T, E, k, skew, dtype):
    lg = _logits(T, E, k, skew, dtype)
    got = {n: v.cpu() for n, v in _route_abi(lg.cuda(), k).items()}
    again = _route_abi(lg.cuda(), k)
    # a. selection and sort, exact
    sel64 = lg.double().topk(k, dim=-1).indices
    ref_gates, ref_index, ref_inv, ref_num, ref_sel = Fx._moe_route_ref(lg, k)
    assert torch.equal(got["selected"].view(T, k).long(), sel64) and torch.equal(ref_sel.long(), sel64)
    assert torch.equal(got["num"], sel64.flatten().bincount(minlength=E))
    assert torch.equal(got["offsets"].long(), torch.cat([torch.zeros(1, dtype=torch.long), got["num"].cumsum(0)]))
    assert torch.equal(got["inv"], ref_inv) and torch.equal(got["batch_index"], ref_index)
    bits = lambda t: t.view(torch.int16 if dtype == BF16 else torch.int32)
    assert torch.equal(bits(got["batch_gates"][got["inv"].long()]), bits(got["gates"]))
    for name in ("selected", "gates", "inv", "batch_index", "batch_gates", "num", "offsets"):
        assert torch.equal(got[name].view(torch.uint8), again[name].cpu().view(torch.uint8)), f"{name} differs run to run"
    assert skew != "same" or ((got["num"] == 0).sum() == E - k and got["num"].max() == T)
    assert skew != "dead" or got["num"][E - 1] == 0
    # b. gates vs the float64 softmax: one round to nearest of an 8-bit significand (bf16) + fp32 slop
    ref = torch.softmax(lg.double().gather(1, sel64), dim=-1)
    err = (got["gates"].view(T, k).double() - ref).abs()
    bound = 2**-8 * ref + 1e-6 if dtype == BF16 else torch.full_like(ref, 1e-6)
    print(f"GATEERR T={T} E={E} k={k} {dtype}: max err {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert ((got["gates"].view(T, k).double().sum(-1) - 1).abs() <= k * 2**-8).all()
    # the public op returns the same bits
    for o, name in zip(ops.moe_route(lg.cuda(), k), ("batch_gates", "batch_index", "inv", "num", "selected")):
        assert torch.equal(o.cpu().flatten().view(torch.uint8), got[name].view(torch.uint8)), name


@pytest.mark.parametrize("E,k", [(8, 2), (33, 1), (64, 8)])
def test_ties_select_lowest_index(E, k):
    x = torch.full((2, E), -1.0)
    x[0] = 1.0                                   # all equal -> experts 0..k-1
    tops = [E - 1 - i for i in range(k - 1)]     # k-1 distinct leaders at the high indices
    for i, c in enumerate(tops):
        x[1, c] = 20.0 - i
    x[1, [1, E // 2]] = 1.0                      # k-th and (k+1)-th logits equal -> index 1
    want = torch.tensor([list(range(k)), tops + [1]])
    for dtype in (BF16, F32):
        got = _route_abi(x.to(dtype).cuda(), k)["selected"].cpu().view(2, k)
        assert torch.equal(got.long(), want), dtype
        assert torch.equal(Fx._moe_route_ref(x.to(dtype), k)[4].long(), want)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T,E,k", [(3 * TILE + 1, 8, 2), (TILE + 1, 5, 3), (9, 64, 8), (TILE - 1, 33, 1), (65, 4, 4)])
def test_route_backward(T, E, k, dtype):
    """d_logits vs float64 autograd of softmax(gather(topk)) fed the same d_batch_gates: selected
    columns within 2^-8 max|ref| + 1e-6 max|g| (fp32 evaluation, one rounding), the rest bitwise +0."""
    lg = _logits(T, E, k, None, dtype)
    lg_d = lg.cuda()
    fwd = _route_abi(lg_d, k)
    dbg = torch.randn(T * k, generator=torch.Generator().manual_seed(T)).to(dtype)
    dbg_d = dbg.cuda()
    out, optr = _guarded(T * E, dtype)
    ret = hip.lib().dolomite_moe_route_bwd(hip.stream(), hip.ptr(dbg_d), hip.ptr(fwd["inv"]), hip.ptr(fwd["selected"]),
                                           hip.ptr(lg_d), optr, T, E, k, hip.dt(lg))
    torch.cuda.synchronize()
    assert ret == 0 and _untouched(out, T * E)
    got = out[GUARD:GUARD + T * E].cpu().view(T, E)

    x = lg.double().requires_grad_(True)
    sel = x.detach().topk(k, dim=-1).indices
    w = torch.softmax(x.gather(1, sel), dim=-1)
    (w.flatten() * dbg.double()[fwd["inv"].cpu().long()]).sum().backward()
    chosen = torch.zeros(T, E, dtype=torch.bool).scatter_(1, sel, True)
    err = (got.double() - x.grad).abs()[chosen].max()
    bound = 2**-8 * float(x.grad.abs().max()) + 1e-6 * float(dbg.double().abs().max())
    print(f"BWDERR T={T} E={E} k={k} {dtype}: max err {float(err):.3e} bound {bound:.3e}")
    assert err <= bound
    zero_bits = got.view(torch.int16 if dtype == BF16 else torch.int32) == 0
    assert zero_bits[~chosen].all(), "unselected column is not +0"
    assert k > 1 or zero_bits.all()


def test_refusals():
    lg = torch.zeros(4, 80, dtype=BF16, device="cuda")
    for E, k in [(65, 2), (16, 9), (4, 5)]:
        _route_abi(lg[:, :E].contiguous(), k, want=9051)   # asserts every buffer untouched
        assert ops.moe_route(lg[:, :E].contiguous(), k) is None
    ints = torch.zeros(4, 8, dtype=torch.int32, device="cuda")
    _route_abi(ints, 2, want=9050)
    assert ops.moe_route(ints, 2) is None and ops.moe_route(ints.half(), 2) is None
    out, optr = _guarded(32, BF16)
    for E, k, dt in [(65, 2, hip.BF16), (8, 9, hip.BF16), (4, 5, hip.BF16), (8, 2, 2)]:
        assert hip.lib().dolomite_moe_route_bwd(hip.stream(), hip.ptr(lg), hip.ptr(lg), hip.ptr(lg), hip.ptr(lg), optr, 4, E, k, dt) != 0
    torch.cuda.synchronize()
    assert _untouched(out, 0)
    _route_abi(lg[:0, :8].contiguous(), 2, want=0)          # T = 0: legal, nothing written
    assert [tuple(o.shape) for o in ops.moe_route(lg[:0, :8].contiguous(), 2)] == [(0,), (0,), (0,), (8,), (0, 2)]


@pytest.mark.parametrize("cfg", R.LAYER_CONFIGS, ids=R.LAYER_IDS)
def test_sparse_moe_layer_routes_on_hip(cfg, monkeypatch):
    """SparseMoE with ops.moe_route engaged and with it patched to None (the torch chain), both against
    moe_refs.layer_ref64: err_route <= 2 * err_baseline per tensor, as test_sparse_moe_layer_vs_float64 asks."""
    E, top_k, n_embd, n_inner, act, bias, dead = cfg
    inp = R.layer_inputs(*cfg)
    ref = R.layer_ref64(inp, top_k, act)
    engaged = []
    real = ops.moe_route

    def run(route):
        monkeypatch.setattr(ops, "moe_route", route)
        layer = R.build_sparse_moe(inp, E, top_k, n_embd, n_inner, act, bias, BF16, "cuda")
        h = inp["h"].cuda().requires_grad_(True)
        out, _ = layer(h)
        out.backward(inp["dout"].cuda())
        torch.cuda.synchronize()
        return dict(R.layer_grads(layer, h), out=out)

    spy = lambda *a: engaged.append(real(*a)) or engaged[-1]
    got, base = run(spy), run(lambda *a: None)
    assert len(engaged) == 1 and engaged[0] is not None, "ops.moe_route did not engage"
    errs = {name: (R.rel_err(got[name], ref[name]), R.rel_err(base[name], ref[name])) for name in sorted(got)}
    print(f"ROUTEERR {R.LAYER_IDS[R.LAYER_CONFIGS.index(cfg)]} (route, baseline): {errs}")
    worse = {name: e for name, e in errs.items() if not e[0] <= 2 * e[1]}
    assert not worse, f"error above twice the torch routing chain's: {worse}"
