"""The routing contract's torch statement (ops/functional.py _moe_route_ref)
against an independent restatement, and SparseMoE on CPU staying on its own
torch lines: ops.moe_route is asked and answers None."""

import pytest
import torch

import dolomite_engine_amd.ops as ops
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from tests import moe_refs as R


@pytest.mark.parametrize("T,E,k", [(37, 8, 2), (130, 5, 3)])
def test_ref_selection_and_stable_sort(T, E, k):
    g = torch.Generator().manual_seed(T)
    # distinct values per row: a permuted grid, exact in bf16
    lg = ((torch.rand(T, E, generator=g).argsort(-1) - E / 2) * 0.25).to(torch.bfloat16)
    gates, index, inv, num, sel = Fx._moe_route_ref(lg, k)
    sel64 = lg.double().topk(k, dim=-1).indices
    assert sel.dtype == torch.int32 and torch.equal(sel.long(), sel64)
    assert torch.equal(num, sel64.flatten().bincount(minlength=E))
    # the stable sort, pair by pair
    order = sorted(range(T * k), key=lambda p: (int(sel64.flatten()[p]), p))
    assert index.tolist() == [p // k for p in order]
    assert inv.dtype == torch.int32 and [int(inv[p]) for p in order] == list(range(T * k))
    want = torch.softmax(lg.double().gather(1, sel64), dim=-1).flatten()[order]
    assert gates.dtype == lg.dtype and ((gates.double() - want).abs() <= 2**-8 * want + 1e-6).all()


def test_ref_ties_select_lowest_index():
    x = torch.tensor([[1.0] * 8, [-1.0, 1.0, -1.0, -1.0, 1.0, -1.0, -1.0, 20.0]])
    assert Fx._moe_route_ref(x, 2)[4].tolist() == [[0, 1], [7, 1]]
    assert Fx._moe_route_ref(x.to(torch.bfloat16), 3)[4].tolist() == [[0, 1, 2], [7, 1, 4]]


def test_sparse_moe_on_cpu_keeps_torch_routing(monkeypatch):
    cfg = R.LAYER_CONFIGS[0]
    inp = R.layer_inputs(*cfg)
    answers = []
    real = ops.moe_route
    monkeypatch.setattr(ops, "moe_route", lambda *a: answers.append(real(*a)))
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the HIP library was asked for on CPU"))
    out, logits = R.build_sparse_moe(inp, *cfg[:6], torch.float32)(inp["h"].float())
    assert answers == [None] and torch.isfinite(out).all()
    assert real(logits.detach(), cfg[1]) is None and real(logits.detach().bfloat16(), cfg[1]) is None
