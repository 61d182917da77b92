"""Register-resident P / dS in the gfx950 dkv kernel: S = Q*K^T and
dP = dO*V^T are computed with the KEY on the lane (4 query rows per lane and
16-query block), packed in registers into the B operand of dV^T += dO^T*P and
dK^T += Q^T*dS, whose A operands are transpose reads of the row-major Q / dO
images in a PERMUTED query order. These tests pin what that layout can get
wrong:

- the query order of the second contraction (flat softmax, so P depends on
  the query only, against a dO pattern asymmetric in query and d);
- the 16-byte transposed epilogue stores into the per-q-head fp32 partials
  (every slot finalize reads is written, no pad column, no row >= T);
- the per-query lse / delta rows at a packed offset that is not a multiple
  of 4, with a ragged last sequence and a NaN tail behind the buffers;
- run-to-run determinism of the partials;
- the dropout mask's lane -> (q, k) mapping (1 column word, 4 row words).

References: the fp32 oracle.attention_varlen_ref on CPU, and for dropout the
CPU restatement of Fx.varlen_attention with the same seed. Tolerances are
those of test_varlen_attention_fwd_bwd_vs_oracle (2e-2 for o, 3e-2 for the
gradients) and of test_dropout_mask_mapping_sharp_scale."""

import functools
import math

import pytest
import torch

import oracle
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def _pack(lo: QKVLayout, q, k, v):
    """Inverse of QKVLayout.unpack_cpu: q (T,H,D), k/v (T,Hkv,D) -> (T,row_len)."""
    T = q.shape[0]
    H, Hkv, D, G = lo.H, lo.Hkv, lo.D, lo.G
    if G == 1:
        return torch.cat([q, k, v], dim=-1).reshape(T, lo.row_len)
    if Hkv > 1:
        return torch.cat([q.reshape(T, Hkv, G * D), k, v], dim=-1).reshape(T, lo.row_len)
    return torch.cat([q.reshape(T, H * D), k.reshape(T, D), v.reshape(T, D)], dim=-1)


def _oracle_fwd_bwd(lo, qkv, cu, scale, do):
    q, k, v = lo.unpack_cpu(qkv)
    qc, kc, vc = (x.float().requires_grad_(True) for x in (q, k, v))
    oc = oracle.attention_varlen_ref(qc, kc, vc, cu, scale)
    oc.backward(do.float().reshape(oc.shape))
    return oc.detach(), qc.grad, kc.grad, vc.grad


# ---------------------------------------------------------------------------
# 1. query order of the second contraction
# ---------------------------------------------------------------------------

_Q_LENS = [33, 65, 129, 200]  # both 32-query chunks, both halves, 2nd key strip, ragged tails
_Q_SHAPES = [("mha", 2, 2, 64), ("mqa", 4, 1, 80), ("gqa", 4, 2, 128)]  # DPAD 64 / 96 / 128


@functools.lru_cache(maxsize=None)
def _query_order_case(head_type, H, Hkv, D, c):
    """K rows are +-1 vectors, q_i = c * K[(29 i + 7) % (i + 1)] (c = 0: flat
    softmax, P[i, k] = 1 / (i + 1) for every causal k), V random, dO a
    small-integer pattern that is exact in bf16 and asymmetric in query, head
    and d. Returns the inputs and the fp32 oracle's fwd+bwd (computed once)."""
    g = torch.Generator().manual_seed(4321 + D)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = _cu(_Q_LENS)
    T = int(cu[-1])
    k = (torch.randint(0, 2, (T, Hkv, D), generator=g) * 2 - 1).float()
    tgt = torch.empty(T, dtype=torch.int64)
    for s, L in zip(cu[:-1].tolist(), _Q_LENS):
        for i in range(L):
            tgt[s + i] = s + (29 * i + 7) % (i + 1)
    q = c * k[tgt][:, torch.arange(H) // (H // Hkv), :]              # (T, H, D)
    v = torch.randint(-4, 5, (T, Hkv, D), generator=g).float() * 0.25
    qkv = _pack(lo, q, k, v).to(torch.bfloat16)
    assert torch.equal(qkv.float(), _pack(lo, q, k, v))              # exact in bf16
    i = torch.arange(T)[:, None, None]
    hh = torch.arange(H)[None, :, None]
    d = torch.arange(D)[None, None, :]
    do = ((5 * i + 3 * d + 7 * hh) % 13 - 6).float().reshape(T, H * D)
    assert torch.equal(do.to(torch.bfloat16).float(), do)
    do = do.to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    return lo, cu, qkv, do, scale, _oracle_fwd_bwd(lo, qkv, cu, scale, do)


@pytest.mark.parametrize("c", [0.0, 0.125], ids=["flat", "mild"])
@pytest.mark.parametrize("head_type,H,Hkv,D", _Q_SHAPES)
def test_query_order_dkv(head_type, H, Hkv, D, c):
    """c = 0: dV[k] = sum_{i >= k} dO[i] / (i + 1) — every causal (q, key)
    pair with a weight that depends on the query only, so pairing a packed P
    slot with another query's dO^T row moves dV by O(1) (dO steps by >= 1
    between neighbouring queries; the tolerance is 3e-2). c = 0.125 adds a
    nonzero dS, which checks the same pairing of the packed dS with the Q^T
    ladder through dK. At L = 200 the waves of the first key strip take the
    maskless body on the tiles at qs = 64 and 128, the masked one elsewhere."""
    lo, cu, qkv, do, scale, (o_ref, dq_ref, dk_ref, dv_ref) = _query_order_case(head_type, H, Hkv, D, c)
    T = qkv.shape[0]
    x = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(x, cu.cuda(), max(_Q_LENS), lo, scale)
    o.backward(do.cuda())
    torch.cuda.synchronize()
    o_g = o.detach().cpu().float().reshape(T, H, D)
    dq_g, dk_g, dv_g = (t.float() for t in lo.unpack_cpu(x.grad.cpu()))
    if c != 0.0:
        assert float(dk_ref.abs().max()) > 0.1                        # dK is really exercised
    for name, got, ref, tol in (("o", o_g, o_ref, 2e-2), ("dq", dq_g, dq_ref, 3e-2),
                                ("dk", dk_g, dk_ref, 3e-2), ("dv", dv_g, dv_ref, 3e-2)):
        print(f"{name}: max|err| {float((got - ref).abs().max()):.3e}  max|ref| {float(ref.abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=tol, atol=tol, msg=lambda m, n=name: f"{n}: {m}")


# ---------------------------------------------------------------------------
# direct ABI sequence: fwd, preprocess, dkv + dq, finalize
# ---------------------------------------------------------------------------

_SENT = -1024.0  # exact in bf16 / fp32 and far outside every result
_TAIL = 4


class _Abi:
    """One packed batch run through the C ABI with caller-owned buffers, so the
    per-q-head fp32 partials are visible before finalize. lse / delta carry
    `stat_fill` in a tail past H*T, dk_acc / dv_acc `_SENT` everywhere."""

    def __init__(self, lo, qkv, do, lens, scale, stat_fill=_SENT):
        self.lo, self.lens, self.scale = lo, lens, scale
        H, D = lo.H, lo.D
        self.T = T = qkv.shape[0]
        self.cu = _cu(lens).cuda()
        self.qkv = qkv.cuda()
        self.do = do.cuda()
        self.o = torch.empty(T, H * D, dtype=torch.bfloat16, device="cuda")
        self.lse = torch.full((H * T + 64,), stat_fill, dtype=torch.float32, device="cuda")
        self.delta = torch.full((H * T + 64,), stat_fill, dtype=torch.float32, device="cuda")
        ts = lo.row_len
        hip.check(
            hip.lib().dolomite_fa_varlen_fwd(
                hip.stream(), *lo.operands(self.qkv),
                hip.ptr(self.o), hip.ptr(self.lse), hip.ptr(self.cu), len(lens), max(lens), T,
                H, lo.Hkv, D, lo.G, *lo.strides(ts), scale, hip.BF16,
            ),
            "fa_varlen_fwd",
        )
        hip.check(
            hip.lib().dolomite_fa_bwd_preprocess(
                hip.stream(), hip.ptr(self.o), hip.ptr(self.do), hip.ptr(self.delta), T, H, D, H * D, H * D,
                hip.BF16),
            "fa_bwd_preprocess",
        )

    def backward(self):
        """dkv + dq into fresh sentinel-filled buffers; returns (dqkv, dk_acc, dv_acc)."""
        lo, T, H, D, ts = self.lo, self.T, self.lo.H, self.lo.D, self.lo.row_len
        dqkv = torch.zeros(T, ts, dtype=torch.bfloat16, device="cuda")
        dk_acc = torch.full((T + _TAIL, H, D), _SENT, dtype=torch.float32, device="cuda")
        dv_acc = torch.full((T + _TAIL, H, D), _SENT, dtype=torch.float32, device="cuda")
        hip.check(
            hip.lib().dolomite_fa_varlen_bwd(
                hip.stream(), *lo.operands(self.qkv),
                hip.ptr(self.do), hip.ptr(self.lse), hip.ptr(self.delta), hip.ptr(dqkv),
                hip.ptr(dk_acc), hip.ptr(dv_acc), hip.ptr(self.cu), len(self.lens), max(self.lens), T,
                H, lo.Hkv, D, lo.G, *lo.strides(ts), H * D, self.scale, hip.BF16,
            ),
            "fa_varlen_bwd",
        )
        torch.cuda.synchronize()
        return dqkv, dk_acc, dv_acc

    def finalize(self, dqkv, dk_acc, dv_acc):
        lo, T = self.lo, self.T
        hip.check(
            hip.lib().dolomite_fa_grad_finalize(
                hip.stream(), hip.ptr(dk_acc), hip.ptr(dv_acc), hip.ptr(dqkv), T, lo.Hkv, lo.D, lo.G,
                lo.row_len, lo.k_off, lo.kv_hstride, lo.v_off, hip.BF16),
            "fa_grad_finalize",
        )
        torch.cuda.synchronize()
        return tuple(t.float() for t in lo.unpack_cpu(dqkv.cpu()))


def _random_case(head_type, H, Hkv, D, lens, seed):
    g = torch.Generator().manual_seed(seed)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    T = sum(lens)
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    return lo, qkv, do, 1.0 / math.sqrt(D)


# ---------------------------------------------------------------------------
# 2. epilogue stores: 16 bytes per lane, block and buffer
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("lens", [[77, 50], [10, 5]], ids=["77-50", "10-5"])
@pytest.mark.parametrize(
    "head_type,H,Hkv,D",
    [
        ("mha", 1, 1, 48),   # DPAD 64, one head: a pad column would land in the next token's row
        ("mqa", 4, 1, 16),   # DPAD 32
        ("mqa", 4, 1, 80),   # DPAD 96
    ],
)
def test_dkv_partial_stores_cover_rows_and_nothing_else(head_type, H, Hkv, D, lens):
    lo, qkv, do, scale = _random_case(head_type, H, Hkv, D, lens, 19 + D)
    T = sum(lens)
    _, dq_ref, dk_ref, dv_ref = _oracle_fwd_bwd(lo, qkv, _cu(lens), scale, do)
    run = _Abi(lo, qkv, do, lens, scale)
    dqkv, dk_acc, dv_acc = run.backward()
    for name, acc in (("dk_acc", dk_acc), ("dv_acc", dv_acc)):
        a = acc.cpu()
        # finalize reads every (t < T, h, d < D) slot: each must have been written
        assert torch.isfinite(a[:T]).all(), name
        assert int((a[:T] == _SENT).sum()) == 0, name
        assert torch.all(a[T:] == _SENT), name
    dq_g, dk_g, dv_g = run.finalize(dqkv, dk_acc, dv_acc)
    for name, got, ref in (("dq", dq_g, dq_ref), ("dk", dk_g, dk_ref), ("dv", dv_g, dv_ref)):
        print(f"{name}: max|err| {float((got - ref).abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2, msg=lambda m, n=name: f"{n}: {m}")


# ---------------------------------------------------------------------------
# 3. lse / delta rows: 4 consecutive queries per lane at an unaligned offset
# ---------------------------------------------------------------------------


def test_dkv_stat_rows_unaligned_offset_ragged_tail_nan_behind():
    """lens [37, 70, 45]: the second sequence starts at packed row 37 and the
    third at 107 (neither a multiple of 4), the last one ends ragged
    (45 % 16 = 13, 45 % 4 = 1) at the very end of the last head's lse / delta
    row, behind which the buffers hold NaN. A row load that reaches past L
    and lets the value through poisons dk / dv; nothing here relies on a
    fault."""
    lens = [37, 70, 45]
    lo, qkv, do, scale = _random_case("mqa", 4, 1, 80, lens, 123)
    T = sum(lens)
    _, dq_ref, dk_ref, dv_ref = _oracle_fwd_bwd(lo, qkv, _cu(lens), scale, do)
    run = _Abi(lo, qkv, do, lens, scale, stat_fill=float("nan"))
    assert torch.isnan(run.lse[lo.H * T:]).all() and torch.isnan(run.delta[lo.H * T:]).all()
    assert torch.isfinite(run.lse[: lo.H * T]).all() and torch.isfinite(run.delta[: lo.H * T]).all()
    dqkv, dk_acc, dv_acc = run.backward()
    assert torch.isfinite(dk_acc[:T]).all() and torch.isfinite(dv_acc[:T]).all()
    dq_g, dk_g, dv_g = run.finalize(dqkv, dk_acc, dv_acc)
    for name, got, ref in (("dq", dq_g, dq_ref), ("dk", dk_g, dk_ref), ("dv", dv_g, dv_ref)):
        assert torch.isfinite(got).all(), name
        print(f"{name}: max|err| {float((got - ref).abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2, msg=lambda m, n=name: f"{n}: {m}")


# ---------------------------------------------------------------------------
# 4. run-to-run determinism of the partials
# ---------------------------------------------------------------------------


def test_dkv_partials_are_bitwise_reproducible():
    lens = [129, 200]
    lo, qkv, do, scale = _random_case("mqa", 4, 1, 80, lens, 55)
    run = _Abi(lo, qkv, do, lens, scale)
    _, dk1, dv1 = run.backward()
    _, dk2, dv2 = run.backward()
    assert torch.equal(dk1, dk2) and torch.equal(dv1, dv2)
    assert int((dk1[: sum(lens)] == _SENT).sum()) == 0


# ---------------------------------------------------------------------------
# 5. dropout: 1 column word + 4 row words per lane and block
# ---------------------------------------------------------------------------


def test_dkv_dropout_mask_mapping_sharp_scale():
    """p = 0.3 at lens [200, 65] (maskless and masked bodies, a second key
    strip, a one-query tail tile), D = 80, softmax sharpened 8x so each row
    leans on a few keys and a lane -> (q, k) mis-mapping of the mask in dkv
    moves dk / dv by far more than the tolerance. Reference: the fp32 CPU
    restatement with the same seed; tolerances of
    test_dropout_mask_mapping_sharp_scale."""
    H, D, p, lens = 4, 80, 0.3, [200, 65]
    lo = QKVLayout.make(H, 1, D, "mqa")
    g = torch.Generator().manual_seed(37)
    cu = _cu(lens)
    T = int(cu[-1])
    scale = 8.0 / math.sqrt(D)
    seed = (0xD1 << 32) + 2424
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)

    x = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(x, cu.cuda(), max(lens), lo, scale, dropout_p=p, seed=seed)
    o.backward(do.cuda())
    torch.cuda.synchronize()
    xc = qkv.float().requires_grad_(True)
    oc = Fx.varlen_attention(xc, cu, max(lens), lo, scale, dropout_p=p, seed=seed)
    oc.backward(do.float())

    rp = 1.0 / (1.0 - p)
    got = dict(zip(("dq", "dk", "dv"), (t.float() for t in lo.unpack_cpu(x.grad.cpu()))))
    ref = dict(zip(("dq", "dk", "dv"), lo.unpack_cpu(xc.grad)))
    for name in ("dk", "dv"):
        print(f"{name}: max|err| {float((got[name] - ref[name]).abs().max()):.3e}  max|ref| {float(ref[name].abs().max()):.3e}")
        torch.testing.assert_close(got[name], ref[name], rtol=3e-2, atol=3e-2 * rp, msg=lambda m, n=name: f"{n}: {m}")
