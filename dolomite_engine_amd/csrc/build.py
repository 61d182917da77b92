"""Build libdolomite_hip.so in-tree for gfx950.

Usage: python -m dolomite_engine_amd.csrc.build
Called by __graft_entry__.build(). hipcc cross-compiles without a GPU.
The .so lands next to the package (dolomite_engine_amd/libdolomite_hip.so)
so it travels with the repo snapshot to the GPU box.
"""

import subprocess
import sys
import tempfile
from pathlib import Path

CSRC = Path(__file__).resolve().parent
PKG = CSRC.parent
REPO = PKG.parent
SO_PATH = PKG / "libdolomite_hip.so"

SOURCES = [CSRC / "elementwise.hip", CSRC / "attention.hip", CSRC / "decode.hip", CSRC / "moe_gemm.hip", CSRC / "data_index.cpp", CSRC / "extend.hip", CSRC / "moe_route.hip", CSRC / "decode_fp8.hip", CSRC / "extend_fp8.hip", CSRC / "fp8_linear.hip", CSRC / "moe_decode.hip", CSRC / "fp8_gemm.hip"]

# Sources compiled on their own, with packed fp32 VALU ops (v_pk_mul_f32 and
# kin) off, and linked in as objects. The other sources keep the one-command
# build they were measured with.
NO_PACKED_FP32 = [CSRC / "extend.hip", CSRC / "moe_route.hip", CSRC / "decode_fp8.hip", CSRC / "extend_fp8.hip", CSRC / "fp8_linear.hip", CSRC / "moe_decode.hip", CSRC / "fp8_gemm.hip"]
_NO_PACKED_FP32_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]

_COMMON = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def _needs_rebuild() -> bool:
    if not SO_PATH.exists():
        return True
    so_mtime = SO_PATH.stat().st_mtime
    deps = SOURCES + [CSRC / "common.h", CSRC / "mfma_tiles.h", CSRC / "extend_common.h", REPO / "include" / "dolomite_hip.h"]
    return any(p.stat().st_mtime > so_mtime for p in deps)


def _run(cmd) -> None:
    print("+", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def build(force: bool = False) -> Path:
    if not force and not _needs_rebuild():
        return SO_PATH
    with tempfile.TemporaryDirectory(prefix="dolomite_hip_build_") as tmp:
        objects = []
        for src in NO_PACKED_FP32:
            obj = str(Path(tmp) / (src.stem + ".o"))
            _run([*_COMMON, *_NO_PACKED_FP32_FLAGS, "-c", str(src), "-o", obj])
            objects.append(obj)
        _run([
            *_COMMON,
            "-shared",
            *objects,  # ahead of the sources: hipcc reads what follows a .cpp as HIP source
            *[str(s) for s in SOURCES if s not in NO_PACKED_FP32],
            "-o",
            str(SO_PATH),
        ])
    return SO_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(SO_PATH)
