"""Return codes of the attention C entry points for rejected arguments.

Every case here returns before any HIP call (an argument check, or an early
0 for an empty problem), so the table runs with null pointers on a machine
without a GPU. It pins each entry point's codes AND their precedence: a
two-fault case names the code that must win.

  9010 dtype is not bf16        9013 p_drop outside [0, 1) (NaN included)
  9011 D > 128                  9014 negative / oversized extent
  9015 scale is not > 0         9016 row_bytes not a positive multiple of 16
"""

import ctypes
from pathlib import Path

import pytest

from dolomite_engine_amd.ops import hip

SO = Path(__file__).resolve().parent.parent / "dolomite_engine_amd" / "libdolomite_hip.so"
NAN = float("nan")


@pytest.fixture(scope="module")
def solib():
    if not SO.exists():
        from dolomite_engine_amd.csrc.build import build

        build()
    lib = ctypes.CDLL(str(SO))
    for name in _ENTRY_POINTS:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGNATURES[name]
    return lib


def _attn_args(entry, batch=2, max_seqlen=128, T=256, H=4, D=64, scale=0.125, dtype=hip.BF16,
               p=0.0, seed=1):
    """Positional arguments of one of the six attention entry points: null
    stream and null pointers, an MHA row of H heads, the values above."""
    bwd, spans = "_bwd" in entry, "_spans_" in entry
    row = 3 * H * D
    # q k v + (o lse | dout lse delta dqkv_q dk_acc dv_acc) + bounds
    args = [None] * (1 + 3 + (6 if bwd else 2) + (2 if spans else 1))
    args += [batch, max_seqlen, T, H, H, D, 1, row, 3 * D, row, 3 * D, row, 3 * D]
    if bwd:
        args.append(H * D)
    args += [scale, dtype]
    if spans or entry.endswith("_dropout"):
        args += [p, seed]
    return args


# (entry point, overrides of _attn_args' defaults, expected return code)
_ATTENTION_CASES = [
    # varlen_fwd: 9010, 9011, 9015 in that order
    ("dolomite_fa_varlen_fwd", dict(dtype=hip.F32), 9010),
    ("dolomite_fa_varlen_fwd", dict(D=136), 9011),
    ("dolomite_fa_varlen_fwd", dict(scale=0.0), 9015),
    ("dolomite_fa_varlen_fwd", dict(scale=NAN), 9015),
    ("dolomite_fa_varlen_fwd", dict(scale=-1.0), 9015),
    ("dolomite_fa_varlen_fwd", dict(dtype=hip.F32, D=136, scale=0.0), 9010),
    ("dolomite_fa_varlen_fwd", dict(D=136, scale=0.0), 9011),
    # varlen_fwd_dropout: 9013 first, then 9010, 9011, 9015
    ("dolomite_fa_varlen_fwd_dropout", dict(dtype=hip.F32, p=1.0), 9013),
    ("dolomite_fa_varlen_fwd_dropout", dict(p=NAN), 9013),
    ("dolomite_fa_varlen_fwd_dropout", dict(p=-0.1), 9013),
    ("dolomite_fa_varlen_fwd_dropout", dict(dtype=hip.F32, D=136, p=0.5), 9010),
    ("dolomite_fa_varlen_fwd_dropout", dict(D=136, scale=0.0, p=0.5), 9011),
    ("dolomite_fa_varlen_fwd_dropout", dict(scale=0.0, p=0.5), 9015),
    ("dolomite_fa_varlen_fwd_dropout", dict(scale=NAN, p=0.0), 9015),
    # varlen_bwd: 9010, 9011 and nothing else. It has no scale check; that
    # cannot be shown without a launch, so scale = 0 rides on a case the
    # D check rejects (a 9015 ahead of 9011 would show here).
    ("dolomite_fa_varlen_bwd", dict(dtype=hip.F32), 9010),
    ("dolomite_fa_varlen_bwd", dict(D=136), 9011),
    ("dolomite_fa_varlen_bwd", dict(dtype=hip.F32, D=136), 9010),
    ("dolomite_fa_varlen_bwd", dict(D=136, scale=0.0), 9011),
    # varlen_bwd_dropout: 9013, 9010, 9011
    ("dolomite_fa_varlen_bwd_dropout", dict(p=1.0), 9013),
    ("dolomite_fa_varlen_bwd_dropout", dict(p=NAN), 9013),
    ("dolomite_fa_varlen_bwd_dropout", dict(dtype=hip.F32, p=1.0), 9013),
    ("dolomite_fa_varlen_bwd_dropout", dict(dtype=hip.F32, D=136, p=0.5), 9010),
    ("dolomite_fa_varlen_bwd_dropout", dict(D=136, scale=0.0, p=0.5), 9011),
    # spans_fwd: 9013, 9010, 9011, 9015, then the gap zeroing's 9016 / 9014,
    # then 0 for a problem without rows
    ("dolomite_fa_spans_fwd", dict(dtype=hip.F32, p=-0.1), 9013),
    ("dolomite_fa_spans_fwd", dict(p=NAN), 9013),
    ("dolomite_fa_spans_fwd", dict(dtype=hip.F32, D=136, scale=0.0, p=0.0), 9010),
    ("dolomite_fa_spans_fwd", dict(D=136, scale=0.0), 9011),
    ("dolomite_fa_spans_fwd", dict(scale=-1.0), 9015),
    ("dolomite_fa_spans_fwd", dict(scale=-1.0, H=1, D=4), 9015),  # ahead of 9016
    ("dolomite_fa_spans_fwd", dict(scale=0.0, T=-1), 9015),       # ahead of 9014
    ("dolomite_fa_spans_fwd", dict(H=1, D=4), 9016),              # an 8-byte o row
    ("dolomite_fa_spans_fwd", dict(H=1, D=4, T=-1), 9016),
    ("dolomite_fa_spans_fwd", dict(T=-1), 9014),
    ("dolomite_fa_spans_fwd", dict(batch=-1), 9014),
    ("dolomite_fa_spans_fwd", dict(batch=0, T=0), 0),
    ("dolomite_fa_spans_fwd", dict(batch=2, max_seqlen=0, T=0), 0),
    # spans_bwd: 9013, 9010, 9011, then 0 for a problem without rows
    ("dolomite_fa_spans_bwd", dict(dtype=hip.F32, p=-0.1), 9013),
    ("dolomite_fa_spans_bwd", dict(p=1.0), 9013),
    ("dolomite_fa_spans_bwd", dict(dtype=hip.F32, D=136), 9010),
    ("dolomite_fa_spans_bwd", dict(D=136, scale=0.0), 9011),
    ("dolomite_fa_spans_bwd", dict(D=136, batch=0), 9011),        # ahead of the early 0
    ("dolomite_fa_spans_bwd", dict(dtype=hip.F32, max_seqlen=0), 9010),
    ("dolomite_fa_spans_bwd", dict(batch=0), 0),
    ("dolomite_fa_spans_bwd", dict(max_seqlen=0), 0),
    ("dolomite_fa_spans_bwd", dict(max_seqlen=-3, scale=0.0), 0),
]

# (stream, buf, row_bytes, seq_begin, seq_end, batch, T)
_ZERO_GAP_CASES = [
    (dict(row_bytes=0), 9016),
    (dict(row_bytes=-16), 9016),
    (dict(row_bytes=24), 9016),
    (dict(row_bytes=24, T=-1), 9016),
    (dict(batch=-1), 9014),
    (dict(T=-1), 9014),
    (dict(batch=65535), 9014),
    (dict(T=0), 0),
    (dict(batch=0, T=0), 0),
]

# (stream, out, seed, p_drop, H, tq0, nq, tk0, nk)
_MASK_PROBE_CASES = [
    (dict(p=1.0), 9013),
    (dict(p=-0.5), 9013),
    (dict(p=NAN), 9013),
    (dict(p=1.0, H=-1), 9013),
    (dict(H=-1), 9014),
    (dict(nq=-1), 9014),
    (dict(nk=-1), 9014),
    (dict(H=65536, nq=65536, nk=65536), 9014),  # more than 2^31 - 1 blocks
    (dict(H=0), 0),
    (dict(nq=0), 0),
    (dict(nk=0), 0),
]

_ENTRY_POINTS = sorted({c[0] for c in _ATTENTION_CASES}
                       | {"dolomite_fa_zero_gap_rows", "dolomite_fa_dropout_mask_probe"})


def _case_id(case):
    over = case[-2]
    return "-".join([*case[:-2], *(f"{k}={v}" for k, v in over.items())]).replace("dolomite_fa_", "")


def test_table_covers_all_six_entry_points():
    assert {c[0] for c in _ATTENTION_CASES} == {
        "dolomite_fa_varlen_fwd", "dolomite_fa_varlen_fwd_dropout",
        "dolomite_fa_varlen_bwd", "dolomite_fa_varlen_bwd_dropout",
        "dolomite_fa_spans_fwd", "dolomite_fa_spans_bwd",
    }


@pytest.mark.parametrize("case", _ATTENTION_CASES, ids=_case_id)
def test_attention_entry_point_return_code(solib, case):
    entry, over, want = case
    assert getattr(solib, entry)(*_attn_args(entry, **over)) == want


@pytest.mark.parametrize("case", _ZERO_GAP_CASES, ids=_case_id)
def test_zero_gap_rows_return_code(solib, case):
    over, want = case
    a = dict(row_bytes=512, batch=2, T=256)
    a.update(over)
    got = solib.dolomite_fa_zero_gap_rows(None, None, a["row_bytes"], None, None, a["batch"], a["T"])
    assert got == want


@pytest.mark.parametrize("case", _MASK_PROBE_CASES, ids=_case_id)
def test_dropout_mask_probe_return_code(solib, case):
    over, want = case
    a = dict(p=0.5, H=2, nq=4, nk=4)
    a.update(over)
    got = solib.dolomite_fa_dropout_mask_probe(None, None, 1, a["p"], a["H"], 0, a["nq"], 0, a["nk"])
    assert got == want
