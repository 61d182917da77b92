"""Return codes of the elementwise C entry points that are decided before any
launch.

Every call here returns before any HIP call (the width rejection, RoPE's odd
head dim, or an early 0 for an empty problem), so the table runs with a null
stream and null pointers on a machine without a GPU. dolomite_ce_* and
dolomite_sqsum are absent on purpose: with empty inputs they still reach the
HIP runtime.

  9002 norm row wider than 16 vectors per lane at the selected vector width
  9003 RoPE head dim is odd
"""

import ctypes
from pathlib import Path

import pytest

from dolomite_engine_amd.ops import hip

SO = Path(__file__).resolve().parent.parent / "dolomite_engine_amd" / "libdolomite_hip.so"
PRESENT = 0x1000  # a non-null res_in / dres operand; never dereferenced

_ENTRY_POINTS = [
    "dolomite_rmsnorm_fwd", "dolomite_rmsnorm_bwd", "dolomite_layernorm_fwd", "dolomite_layernorm_bwd",
    "dolomite_rmsnorm_bwd_nblocks", "dolomite_reduce_partials", "dolomite_rope_qkv",
    "dolomite_adamw_step", "dolomite_scale_inplace",
]


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


def _norm_args(entry, operand, T_rows, H, dtype):
    """Positional arguments of a norm entry point: null stream and pointers,
    except res_in (forward) / dres (backward), which is `operand`."""
    if entry == "dolomite_rmsnorm_fwd":    # x res_in w y res_out rstd
        return [None, None, operand, None, None, None, None, T_rows, H, 1e-5, dtype]
    if entry == "dolomite_layernorm_fwd":  # x res_in w b y res_out mean rstd
        return [None, None, operand, None, None, None, None, None, None, T_rows, H, 1e-5, dtype]
    if entry == "dolomite_rmsnorm_bwd":    # dy s w rstd dx dw_partial dres
        return [None, None, None, None, None, None, None, operand, T_rows, H, dtype]
    assert entry == "dolomite_layernorm_bwd"  # dy s w mean rstd dx dwdb_partial dres
    return [None, None, None, None, None, None, None, None, operand, T_rows, H, dtype]


_NORM_ENTRIES = _ENTRY_POINTS[:4]
# vectors per lane = ceil(H / (64 * V)) = 17 in each: one past the widest bucket
_TOO_WIDE = [
    (hip.BF16, 8200),  # V = 8
    (hip.BF16, 1025),  # V = 1 (1025 % 8 != 0)
    (hip.F32, 1025),   # V = 1 (1025 % 4 != 0)
    (hip.F32, 4100),   # V = 4
]


@pytest.mark.parametrize("dtype,H", _TOO_WIDE, ids=lambda v: str(v))
@pytest.mark.parametrize("operand", [None, PRESENT], ids=["plain", "res"])
@pytest.mark.parametrize("entry", _NORM_ENTRIES)
def test_norm_rejects_too_wide_row(solib, entry, operand, dtype, H):
    assert getattr(solib, entry)(*_norm_args(entry, operand, 3, H, dtype)) == 9002


@pytest.mark.parametrize("dtype,H", _TOO_WIDE, ids=lambda v: str(v))
@pytest.mark.parametrize("operand", [None, PRESENT], ids=["plain", "res"])
@pytest.mark.parametrize("entry", _NORM_ENTRIES)
def test_norm_empty_problem_wins_over_width(solib, entry, operand, dtype, H):
    assert getattr(solib, entry)(*_norm_args(entry, operand, 0, H, dtype)) == 0


def _rope(solib, T_rows, D, dtype=hip.BF16):
    H, Hkv = 4, 4
    row = 3 * H * D
    # stream qkv_in qkv_out cos sin | T_rows row_len H Hkv D G q_gstride k_off kv_hstride dir rotate_v_copy dtype
    return solib.dolomite_rope_qkv(None, None, None, None, None, T_rows, row, H, Hkv, D, 1, 3 * D, D, 3 * D, 1, 0, dtype)


@pytest.mark.parametrize("dtype", [hip.BF16, hip.F32])
def test_rope_odd_head_dim_wins_over_empty_problem(solib, dtype):
    assert _rope(solib, 16, 7, dtype) == 9003
    assert _rope(solib, 0, 7, dtype) == 9003
    assert _rope(solib, 0, 8, dtype) == 0


@pytest.mark.parametrize("grad_dtype", [hip.BF16, hip.F32])
def test_adamw_empty_shard(solib, grad_dtype):
    # stream master param_out grad grad_dtype m v n lr beta1 beta2 eps weight_decay step gscale
    got = solib.dolomite_adamw_step(None, None, None, None, grad_dtype, None, None, 0,
                                    1e-3, 0.9, 0.95, 1e-8, 0.1, 1, None)
    assert got == 0


@pytest.mark.parametrize("dtype", [hip.BF16, hip.F32])
def test_scale_inplace_empty_buffer(solib, dtype):
    assert solib.dolomite_scale_inplace(None, None, 0, 0.5, dtype) == 0


def test_reduce_partials_no_columns(solib):
    assert solib.dolomite_reduce_partials(None, None, None, 4096, 0) == 0


def test_norm_bwd_partial_rows(solib):
    assert solib.dolomite_rmsnorm_bwd_nblocks(1) == 4096
    assert solib.dolomite_rmsnorm_bwd_nblocks(1 << 20) == 4096
