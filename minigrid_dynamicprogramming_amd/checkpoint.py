"""What a value-iteration checkpoint may resume on, and its file format: the rules of
dp.ValueIteration.resume / save_checkpoint / load_checkpoint, which need no handle (Jacobi is memoryless
given V_k, so a checkpoint is V, the sweep count and the meta that names its grids and parameters).
"""
from __future__ import annotations

import json

import numpy as np


def resume_values(mine: dict, ckpt: dict, np_dtype, B: int, S: int, verify_cells: bool = True) -> np.ndarray:
    """The contiguous (B, S) V of `ckpt` for a handle whose _ckpt_meta() is `mine`.  Refused (ValueError), in
    this order: no meta, a parameter that differs, cells unknown or other cells (with verify_cells), V of
    another dtype, V of another shape."""
    meta = ckpt.get("meta")
    if meta is None:
        raise ValueError("checkpoint has no meta (grids and parameters); refusing to resume blind")
    for key, val in mine.items():
        if key == "cells_sha256":
            continue
        if meta.get(key) != val:
            raise ValueError(f"checkpoint {key}={meta.get(key)!r} does not match the handle's {val!r}")
    if verify_cells:
        if mine["cells_sha256"] is None or meta.get("cells_sha256") is None:
            raise ValueError("cells digest unknown (load_device); pass verify_cells=False to resume anyway")
        if meta["cells_sha256"] != mine["cells_sha256"]:
            raise ValueError("checkpoint was taken on other grids (cells sha256 differs)")
    V = np.asarray(ckpt["V"])
    if V.dtype != np_dtype:
        raise ValueError(f"checkpoint V is {V.dtype}, the handle computes in {np.dtype(np_dtype)}")
    if V.shape != (B, S):
        raise ValueError(f"checkpoint V of shape {V.shape} does not match the handle's {(B, S)}")
    return np.ascontiguousarray(V)


def save_checkpoint(path, ckpt: dict) -> None:
    """Write a checkpoint as .npz (plain arrays and a JSON string: np.load needs no pickle)."""
    np.savez(path, V=ckpt["V"], pi=ckpt["pi"], sweeps=np.int64(ckpt["sweeps"]), dv=np.float64(ckpt["dv"]),
             converged=np.bool_(ckpt["converged"]), meta=np.str_(json.dumps(ckpt.get("meta"))))


def load_checkpoint(path) -> dict:
    z = np.load(path)  # allow_pickle=False
    return {"V": z["V"], "pi": z["pi"], "sweeps": int(z["sweeps"]), "dv": float(z["dv"]),
            "converged": bool(z["converged"]), "meta": json.loads(str(z["meta"])) if "meta" in z else None}
