"""Workgroup shapes of the flash forward and dq kernels: an instantiation runs
either 8 waves over 128 q rows or 4 waves over 64 q rows per workgroup, with
its own grid, heaviest-tile-first order, XCD remap and K/V staging. These
tests cross every boundary the tile height and the grid introduce:

- sequence lengths around 64 and 128 (one row, one short of a tile, exactly
  one, one over, two tiles, a ragged multi-tile tail) packed into ONE call,
  so workgroups of surplus tiles exit and the reversed tile order is used;
- batch * heads a multiple of 8 (the XCD remap permutes the grid) and not
  (its identity fallback);
- every head-dim instantiation (D 16 / 64 / 80 / 128 -> DPAD 32 / 64 / 96 /
  128), MQA and GQA, with and without dropout: which shape each of them runs
  is the launcher's choice, the results must not depend on it.

References: the fp32 oracle.attention_varlen_ref; with dropout the fp32 CPU
restatement built on attention_dropout_keep_mask with the same seed.
Tolerances: those of tests/test_gpu_attention_regfrag.py for the same
comparisons (2e-2 for o, 3e-2 for dq/dk/dv, atol scaled by 1/(1-p) with
dropout).
"""

import functools
import math

import pytest
import torch

import oracle
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops.functional import QKVLayout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


PACKS = {
    # every boundary of a 64-row and of a 128-row q tile, 8 sequences in one call
    "ragged": ([1, 63, 64, 65, 127, 128, 129, 200], [("mqa", 4, 1), ("gqa", 4, 2)]),
    # 8 sequences x 4 heads: batch * heads % 8 == 0, the XCD remap permutes the grid
    "remap": ([130, 70, 64, 5, 192, 33, 100, 129], [("mqa", 4, 1), ("gqa", 4, 2)]),
    # 3 sequences x 2 heads: the remap's identity fallback
    "identity": ([150, 64, 97], [("mqa", 2, 1)]),
}
DIMS = [16, 64, 80, 128]
CASES = [
    pytest.param(pack, ht, H, Hkv, D, id=f"{pack}-{ht}-H{H}-D{D}")
    for pack, (_, heads) in PACKS.items()
    for ht, H, Hkv in heads
    for D in DIMS
]


def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def _seed(D, H):
    return (0x0CC << 32) + 1000 * D + H


@functools.lru_cache(maxsize=None)
def _case(pack, head_type, H, Hkv, D, p):
    """Inputs and the CPU reference's (o, dq, dk, dv), computed once."""
    lens = PACKS[pack][0]
    lo = QKVLayout.make(H, Hkv, D, head_type)
    cu = _cu(lens)
    T = int(cu[-1])
    g = torch.Generator().manual_seed(4321 + D + 7 * H + Hkv)
    qkv = (torch.randn(T, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(T, H * D, generator=g) * 0.5).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    if p == 0.0:
        q, k, v = lo.unpack_cpu(qkv)
        qc, kc, vc = (x.float().requires_grad_(True) for x in (q, k, v))
        oc = oracle.attention_varlen_ref(qc, kc, vc, cu, scale)
        oc.backward(do.float().reshape(oc.shape))
        ref = (oc.detach().reshape(T, H * D), qc.grad, kc.grad, vc.grad)
    else:
        xc = qkv.float().requires_grad_(True)
        oc = Fx.varlen_attention(xc, cu, max(lens), lo, scale, dropout_p=p, seed=_seed(D, H))
        oc.backward(do.float())
        ref = (oc.detach(), *lo.unpack_cpu(xc.grad))
    return lo, cu, lens, qkv, do, scale, ref


def _run_gpu(lo, cu, lens, qkv, do, scale, p, D, H):
    x = qkv.cuda().requires_grad_(True)
    o = Fx.varlen_attention(x, cu.cuda(), max(lens), lo, scale, dropout_p=p, seed=_seed(D, H) if p else None)
    o.backward(do.cuda())
    torch.cuda.synchronize()
    return o.detach(), x.grad


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("pack,head_type,H,Hkv,D", CASES)
def test_fwd_bwd_vs_reference(pack, head_type, H, Hkv, D, p):
    lo, cu, lens, qkv, do, scale, (o_ref, dq_ref, dk_ref, dv_ref) = _case(pack, head_type, H, Hkv, D, p)
    o, dqkv = _run_gpu(lo, cu, lens, qkv, do, scale, p, D, H)
    dq_g, dk_g, dv_g = (t.float() for t in lo.unpack_cpu(dqkv.cpu()))
    rp = 1.0 / (1.0 - p)
    for name, got, ref, tol in (("o", o.cpu().float(), o_ref, 2e-2), ("dq", dq_g, dq_ref, 3e-2),
                                ("dk", dk_g, dk_ref, 3e-2), ("dv", dv_g, dv_ref, 3e-2)):
        print(f"{name}: max|err| {float((got - ref).abs().max()):.3e}  max|ref| {float(ref.abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=tol, atol=tol * rp, msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("D", DIMS)
def test_two_calls_are_bitwise_equal(D, p):
    """Exclusive stores and a fixed reduction order: outputs and gradients of
    two calls on the same inputs are the same bits."""
    lo, cu, lens, qkv, do, scale, _ = _case("ragged", "gqa", 4, 2, D, p)
    o1, g1 = _run_gpu(lo, cu, lens, qkv, do, scale, p, D, 4)
    o2, g2 = _run_gpu(lo, cu, lens, qkv, do, scale, p, D, 4)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)), "o"
    assert torch.equal(g1.view(torch.int16), g2.view(torch.int16)), "dqkv"


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("D", DIMS)
def test_half_padded_dense_batch_is_bitwise_the_packed_batch(D, side):
    """span_attention on a (B=2, S=192) batch whose first row is half padding
    equals varlen_attention on the packed copy, and its pad rows are +0."""
    B, S, lens = 2, 192, [96, 192]
    lo = QKVLayout.make(4, 1, D, "mqa")
    g = torch.Generator().manual_seed(99 + D)
    qkv = (torch.randn(B * S, lo.row_len, generator=g) * 0.5).to(torch.bfloat16)
    do = (torch.randn(B * S, lo.H * D, generator=g) * 0.5).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    begin = [b * S + (0 if side == "right" else S - n) for b, n in enumerate(lens)]
    end = [s + n for s, n in zip(begin, lens)]
    rows = torch.cat([torch.arange(s, e) for s, e in zip(begin, end)])

    xp = qkv[rows].cuda().requires_grad_(True)
    op = Fx.varlen_attention(xp, _cu(lens).cuda(), max(lens), lo, scale)
    op.backward(do[rows].cuda())

    x = qkv.cuda().requires_grad_(True)
    o = Fx.span_attention(x, torch.tensor(begin, dtype=torch.int32).cuda(),
                          torch.tensor(end, dtype=torch.int32).cuda(), max(lens), lo, scale)
    o.backward(do.cuda())
    torch.cuda.synchronize()

    r = rows.cuda()
    assert torch.equal(o.detach()[r].view(torch.int16), op.detach().view(torch.int16)), "o"
    assert torch.equal(x.grad[r].view(torch.int16), xp.grad.view(torch.int16)), "dqkv"
    pad = torch.ones(B * S, dtype=torch.bool)
    pad[rows] = False
    assert int(pad.sum()) == B * S - sum(lens)
    assert int(o.detach()[pad.cuda()].view(torch.int16).count_nonzero()) == 0
    assert int(x.grad[pad.cuda()].view(torch.int16).count_nonzero()) == 0
