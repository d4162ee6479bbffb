"""Shared test helpers: golden loading, parameter shapes of the hot-path modules, filled
state dicts keyed exactly as tests/golden/gen_golden.py keyed them."""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, Tuple

import numpy as np
import torch

from eavsr_amd.utils.synthetic import fill_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 1_000_000      # raw array bytes per fixture file: every committed file stays under 1 MiB
REGULAR = torch.tensor([[-1, -1, -1, 0, 0, 0, 1, 1, 1], [-1, 0, 1, -1, 0, 1, -1, 0, 1]], dtype=torch.float32)


def golden(name: str) -> Dict[str, torch.Tensor]:
    """GOLDEN/name.npz merged with name.part1.npz, name.part2.npz, ... where save_golden split the fixture"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: torch.from_numpy(z[k]) for k in z.files}
    i = 1
    while os.path.exists(os.path.join(GOLDEN, f"{name}.part{i}.npz")):
        z = np.load(os.path.join(GOLDEN, f"{name}.part{i}.npz"))
        out.update({k: torch.from_numpy(z[k]) for k in z.files})
        i += 1
    return out


def save_golden(name: str, arrays: Dict[str, np.ndarray]) -> None:
    """`arrays` as GOLDEN/name.npz; once PART_BYTES of raw data are in a file, the next arrays go to name.part1.npz, ..."""
    for f in glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")):
        os.remove(f)
    parts, size = [{}], 0
    for k, v in arrays.items():
        if parts[-1] and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for i, p in enumerate(parts):
        np.savez_compressed(os.path.join(GOLDEN, name + (f".part{i}" if i else "") + ".npz"), **p)


def golden_keys(tag: str = "x4") -> dict:
    with open(os.path.join(GOLDEN, f"eavsrp_{tag}_keys.json")) as f:
        return json.load(f)


def model_shapes(tag: str = "x4") -> Dict[str, Tuple[int, ...]]:
    return {k: tuple(v) for k, v in golden_keys(tag)["shapes"].items()}


def _conv(p, co, ci, k):
    return {p + "weight": (co, ci, k, k), p + "bias": (co,)}


def adapt_front_shapes(p, c=64):
    s = {p + "regular_matrix": (2, 9)}
    s.update(_conv(p + "concat.0.", 2 * c, 1, 3))
    s.update(_conv(p + "concat2.0.", c, 2, 3))
    return s


def adapt3x3_shapes(p):
    s = adapt_front_shapes(p)
    s.update(_conv(p + "transform_matrix_conv.", 4, 64, 3))
    s.update(_conv(p + "translation_conv.", 2, 64, 3))
    return s


def adaptoffset_shapes(p, D=8):
    s = adapt_front_shapes(p)
    s.update(_conv(p + "transform_matrix_conv.", 4 * D, 64, 5))
    s.update(_conv(p + "translation_conv.", 2 * D, 64, 5))
    s.update(_conv(p + "mask_conv.", 9 * D, 64, 5))
    return s


def trans_shapes(p):
    return _conv(p + "conv_first.", 2, 18, 3)


def multiadstn_shapes(p, D=8):
    s = _conv(p, 64, 64, 3)
    for l in (1, 2, 3):
        s.update(adapt3x3_shapes(f"{p}flow_l{l}."))
        s.update(trans_shapes(f"{p}trans_l{l}."))
    s.update(adaptoffset_shapes(p + "adastn.", D))
    return s


def rcab_shapes(p):
    s = _conv(p + "res.0.", 64, 64, 3)
    s.update(_conv(p + "res.2.", 64, 64, 3))
    s.update(_conv(p + "ca.conv_du.0.", 4, 64, 1))
    s.update(_conv(p + "ca.conv_du.2.", 64, 4, 1))
    return s


def rcagroup_shapes(p, nb):
    s = {}
    for k in range(nb):
        s.update(rcab_shapes(f"{p}rg.{k}."))
    s.update(_conv(f"{p}rg.{nb}.", 64, 64, 3))
    return s


def rbic_shapes(p, cin, nb):
    s = _conv(p + "main.0.", 64, cin, 3)
    s.update(rcagroup_shapes(p + "main.2.", nb))
    return s


def filled(shapes, preset="default", seed=0):
    fixed = {k: REGULAR for k in shapes if k.endswith("regular_matrix")}
    fixed.update({k: torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1) for k in shapes if k.endswith("mean")})
    fixed.update({k: torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1) for k in shapes if k.endswith("std")})
    return fill_state_dict(shapes, preset, seed, fixed=fixed)


def maxabs(a, b):
    return (a.double() - b.double()).abs().max().item()


def restate_pairs(store, frames, desc, ph, pw, s=1):
    """the training item of the reference restated in numpy (crop -> [:, :, ::-1] -> [:, ::-1, :] -> transpose(0, 2, 1) ->
    np.float32(.) / 255; data/realvsr_dataset.py:166-175, util/util.py:223-227), what ops.gather_pairs is compared with:
    store (F, C, H, W) uint8 ndarray at resolution s x LR; frames (n, t), desc (n, 4) in LR pixels -> (n, t, C, s ph, s pw) fp32"""
    n, t = frames.shape
    out = np.empty((n, t, store.shape[1], s * ph, s * pw), np.float32)
    for i in range(n):
        top, left, flags = (int(v) for v in desc[i, :3])
        for j in range(t):
            img = store[frames[i, j]][..., s * top:s * (top + ph), s * left:s * (left + pw)]
            if flags & 1:
                img = img[:, :, ::-1]
            if flags & 2:
                img = img[:, ::-1, :]
            if flags & 4:
                img = img.transpose(0, 2, 1)
            out[i, j] = np.float32(np.ascontiguousarray(img)) / 255
    return out
