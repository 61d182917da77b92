"""Read/write golden fixtures whose tensors do not fit one committed file.

A fixture is a dict saved with torch.save. Committed files must stay below
1 MiB, so save_golden() moves tensor-dict entries (state_dict, grads, ...)
that would push `name.pt` over PART_BYTES into sibling files
`name.part{k}.pt`, each a {top-level key: {sub key: tensor}} dict, and
load_golden() merges them back. Values are stored unchanged. TEST
INFRASTRUCTURE ONLY (see oracle/__init__.py).
"""

from pathlib import Path

import torch

PART_BYTES = 900 * 1024  # payload per file; leaves room for pickle/zip overhead


def _nbytes(t):
    return t.numel() * t.element_size()


def _is_tensor_dict(v):
    return isinstance(v, dict) and bool(v) and all(isinstance(t, torch.Tensor) for t in v.values())


def save_golden(fx: dict, path) -> list[Path]:
    """Save `fx` at `path`, spilling tensor dicts into .part files when the
    whole would exceed PART_BYTES. Returns the files written."""
    path = Path(path)
    for old in path.parent.glob(path.stem + ".part*.pt"):
        old.unlink()

    total = sum(
        sum(_nbytes(t) for t in v.values()) if _is_tensor_dict(v) else (_nbytes(v) if isinstance(v, torch.Tensor) else 0)
        for v in fx.values()
    )
    if total <= PART_BYTES:
        torch.save(fx, path)
        return [path]

    main, parts, cur, cur_bytes = {}, [], {}, 0
    for k, v in fx.items():
        if not _is_tensor_dict(v):
            main[k] = v
            continue
        main[k] = {}  # keeps the key (and its position) in the main file
        for kk, t in v.items():
            assert _nbytes(t) <= PART_BYTES, f"{k}.{kk} alone exceeds the part size"
            if cur and cur_bytes + _nbytes(t) > PART_BYTES:
                parts.append(cur)
                cur, cur_bytes = {}, 0
            cur.setdefault(k, {})[kk] = t.clone()  # clone: drop shared storage before pickling
            cur_bytes += _nbytes(t)
    if cur:
        parts.append(cur)

    written = [path]
    torch.save(main, path)
    for i, part in enumerate(parts):
        p = path.with_name(f"{path.stem}.part{i}.pt")
        torch.save(part, p)
        written.append(p)
    return written


def load_golden(path) -> dict:
    path = Path(path)
    fx = torch.load(path, weights_only=False)
    for p in sorted(path.parent.glob(path.stem + ".part*.pt"), key=lambda q: int(q.stem.rsplit("part", 1)[1])):
        for k, sub in torch.load(p, weights_only=False).items():
            fx[k].update(sub)
    return fx
