"""NIQE (Mittal, Soundararajan, Bovik: "Making a completely blind image quality analyzer", SPL 2013), the report's no-reference
column: the host half.  The device computes 25 moments per 96 x 96 block at two scales (`ops.niqe_moments`,
`ops.niqe_half`); here they become the 36 features of a block and the distance to the pristine model the USER supplies -- no
pristine model ships with this project, and the values depend on it.  float64 numpy throughout; scipy is not needed.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Tuple

import numpy as np

BLOCK = 96                       # block side at scale 1; 48 at scale 2
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))      # the np.roll shifts of the four paired products
ALPHA_GRID = np.arange(0.2, 10.001, 0.001)      # the shape values the fit searches: 0.2, 0.201, ..., 10.0 (9801 of them)

_WINDOW = None
_GAMMA = None


def gaussian_window() -> Tuple[np.ndarray, np.ndarray]:
    """(g1 (7,), g (7, 7)): g[i, j] = exp(-(i^2 + j^2) / (2 sigma^2)) over i, j in -3..3 with sigma = 7 / 6, normalised to sum 1, and
    its marginal g1 (exp(-i^2 / (2 sigma^2)) normalised): g is the outer product of g1 within 1e-15, and the device applies g1
    along W, then along H."""
    global _WINDOW
    if _WINDOW is None:
        i = np.arange(-3, 4, dtype=np.float64)
        sigma = 7.0 / 6.0
        e = np.exp(-(i * i) / (2.0 * sigma * sigma))
        g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * sigma * sigma))
        g1, g = e / e.sum(), g / g.sum()
        g1.setflags(write=False)
        g.setflags(write=False)
        _WINDOW = (g1, g)
    return _WINDOW


def luma601(r, g, b):
    """BT.601 studio-range luma of 8-bit R, G, B (integer arrays) in integers: 16 + round_half_even((65481 R + 128553 G + 24966 B)
    / 255000) -- MATLAB's rgb2ycbcr on uint8, with the division and its tie decided exactly (DESIGN 7m counts the ties)."""
    n = 65481 * np.asarray(r, np.int64) + 128553 * np.asarray(g, np.int64) + 24966 * np.asarray(b, np.int64)
    q, rem = np.divmod(n, 255000)
    return 16 + q + ((2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1)))


def _cubic(x: np.ndarray) -> np.ndarray:
    a = np.abs(x)
    a2, a3 = a * a, a * a * a
    return (1.5 * a3 - 2.5 * a2 + 1.0) * (a <= 1) + (-0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0) * ((a > 1) & (a <= 2))


def resize_tables(length: int, scale: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of MATLAB's `imresize(I, scale)` (bicubic, a = -0.5, antialiased) for scale <= 1: (idx int32 (out, taps), weight
    fp64 (out, taps)), out = ceil(length scale).  Output o (1-based x = o + 1) sits at u = x / scale + 0.5 (1 - 1 / scale); the
    kernel is stretched to the width 4 / scale; its ceil(width) + 2 taps start at floor(u - width / 2) and weigh
    scale k(scale (u - i)), normalised to sum 1; indices outside 1..length are reflected symmetrically (.. 2, 1, 1, 2 ..); taps whose
    weight is 0 for every output are dropped.  idx is 0-based.  At scale 0.5 an interior output o reads 2 o - 3 .. 2 o + 4 with the
    weights (-3, -9, 29, 111, 111, 29, -9, -3) / 256."""
    length = int(length)
    if length < 1 or not (0.0 < scale <= 1.0):
        raise ValueError(f"resize_tables: length {length}, scale {scale}: at least one sample and a scale in (0, 1]")
    out = int(math.ceil(length * scale))
    x = np.arange(1, out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1.0 - 1.0 / scale)
    width = 4.0 / scale
    left = np.floor(u - width / 2.0)
    taps = int(math.ceil(width)) + 2
    ind = left[:, None] + np.arange(taps, dtype=np.float64)[None, :]
    w = scale * _cubic(scale * (u[:, None] - ind))
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(length), np.arange(length - 1, -1, -1)])
    idx = aux[np.mod(ind.astype(np.int64) - 1, 2 * length)]
    keep = np.any(w != 0.0, axis=0)
    return np.ascontiguousarray(idx[:, keep], np.int32), np.ascontiguousarray(w[:, keep], np.float64)


def _gamma_tables():
    """(rho, sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a)) over ALPHA_GRID, rho = G(2/a)^2 / (G(1/a) G(3/a)), built once with math.lgamma"""
    global _GAMMA
    if _GAMMA is None:
        l1 = np.array([math.lgamma(1.0 / a) for a in ALPHA_GRID])
        l2 = np.array([math.lgamma(2.0 / a) for a in ALPHA_GRID])
        l3 = np.array([math.lgamma(3.0 / a) for a in ALPHA_GRID])
        rho = np.exp(2.0 * l2 - l1 - l3)
        if not (np.diff(rho) > 0).all():      # the search below relies on it
            raise RuntimeError("niqe: the gamma-ratio table is not increasing")
        _GAMMA = (rho, np.sqrt(np.exp(l1 - l3)), np.exp(l2 - l1))
    return _GAMMA


def features_from_moments(moments, block: int = BLOCK) -> np.ndarray:
    """moments (..., 25) -- per map (M and its four rolled products, `ops.niqe_moments`) n_neg, n_pos, sum v^2 over v < 0, sum v^2
    over v > 0, sum |v| over the block^2 values of a block -- -> the 18 features (..., 18) of DESIGN 7m: the asymmetric generalised
    gaussian fit of every map, [alpha, (beta_l + beta_r) / 2] of M and [alpha, (beta_r - beta_l) G(2/alpha) / G(1/alpha), beta_l,
    beta_r] of each product.  A map with no negative or no positive value gives `nan`, which propagates."""
    m = np.asarray(moments, np.float64)
    if m.shape[-1] != 25:
        raise ValueError(f"features_from_moments: (..., 25) moments, got {m.shape}")
    m = m.reshape(m.shape[:-1] + (5, 5))
    n_neg, n_pos, s_neg, s_pos, s_abs = (m[..., k] for k in range(5))
    count = float(block * block)
    rho, root13, ratio21 = _gamma_tables()
    with np.errstate(divide="ignore", invalid="ignore"):
        left, right = np.sqrt(s_neg / n_neg), np.sqrt(s_pos / n_pos)
        gam = left / right
        rhat = (s_abs / count) ** 2 / ((s_neg + s_pos) / count)
        rhatn = rhat * (gam ** 3 + 1.0) * (gam + 1.0) / (gam ** 2 + 1.0) ** 2
    ok = np.isfinite(rhatn)
    r = np.where(ok, rhatn, 0.0)
    hi = np.clip(np.searchsorted(rho, r, side="left"), 1, len(rho) - 1)      # rho[hi - 1] < r <= rho[hi] inside the table
    lo = hi - 1
    pick = np.where((rho[lo] - r) ** 2 <= (rho[hi] - r) ** 2, lo, hi)         # the first minimum wins
    alpha = np.where(ok, ALPHA_GRID[pick], np.nan)
    beta_l, beta_r = left * root13[pick], right * root13[pick]
    beta_l, beta_r = np.where(ok, beta_l, np.nan), np.where(ok, beta_r, np.nan)
    out = np.empty(m.shape[:-2] + (18,), np.float64)
    out[..., 0] = alpha[..., 0]
    out[..., 1] = (beta_l[..., 0] + beta_r[..., 0]) / 2.0
    for j in range(1, 5):
        out[..., 4 * j - 2] = alpha[..., j]
        out[..., 4 * j - 1] = (beta_r[..., j] - beta_l[..., j]) * ratio21[pick[..., j]]
        out[..., 4 * j] = beta_l[..., j]
        out[..., 4 * j + 1] = beta_r[..., j]
    return out


def score(features1, features2, params) -> float:
    """The NIQE score of one image: features1 / features2 (blocks, 18), the two scales' features of the same block positions;
    params = (mu_p (36,), cov_p (36, 36)), the pristine model.  m = the nan-mean of every column, S = np.cov over the rows without
    a `nan`, score = sqrt((mu_p - m) pinv((cov_p + S) / 2) (mu_p - m)^T); `nan` with fewer than two clean rows."""
    mu_p, cov_p = params
    f = np.concatenate([np.asarray(features1, np.float64).reshape(-1, 18), np.asarray(features2, np.float64).reshape(-1, 18)], axis=1)
    clean = f[~np.isnan(f).any(axis=1)]
    if clean.shape[0] < 2:
        return math.nan
    seen = ~np.isnan(f)
    with np.errstate(invalid="ignore"):
        m = np.where(seen, f, 0.0).sum(axis=0) / seen.sum(axis=0)
    s = np.cov(clean, rowvar=False)
    d = (np.asarray(mu_p, np.float64).reshape(-1) - m)[None, :]
    return float(np.sqrt((d @ np.linalg.pinv((np.asarray(cov_p, np.float64) + s) / 2.0) @ d.T)[0, 0]))


def load_niqe_params(source) -> Tuple[np.ndarray, np.ndarray]:
    """The pristine model: an `.npz` file (or a mapping) with `mu_pris_param` (36 or 1 x 36) and `cov_pris_param` (36 x 36); a `.mat`
    file with `mu_prisparam` / `cov_prisparam` where scipy.io imports.  A `gaussian_window` in it must be the definition's within
    1e-6.  ValueError (naming the file) for a missing file, missing keys, wrong shapes, non-finite entries or another window."""
    if isinstance(source, (str, os.PathLike)):
        name = os.fspath(source)
        if not os.path.isfile(name):
            raise ValueError(f"niqe: pristine model {name!r} not found (no pristine model ships with this project: name the file)")
        if name.lower().endswith(".mat"):
            try:
                from scipy.io import loadmat
            except ImportError as e:
                raise ValueError(f"niqe: {name!r} is a .mat file and scipy.io does not import here: convert it to .npz "
                                 "(mu_pris_param, cov_pris_param)") from e
            try:
                data = dict(loadmat(name))
            except Exception as e:
                raise ValueError(f"niqe: cannot read {name!r}: {e}") from e
        else:
            try:
                with np.load(name, allow_pickle=False) as z:
                    data = {k: z[k] for k in z.files}
            except Exception as e:
                raise ValueError(f"niqe: cannot read {name!r}: {e}") from e
    elif hasattr(source, "keys"):
        name, data = "<mapping>", {k: source[k] for k in source.keys()}
    else:
        raise ValueError(f"niqe: the pristine model is a file name or a mapping, got {type(source)}")
    mu = data.get("mu_pris_param", data.get("mu_prisparam"))
    cov = data.get("cov_pris_param", data.get("cov_prisparam"))
    if mu is None or cov is None:
        raise ValueError(f"niqe: {name}: mu_pris_param and cov_pris_param (.mat: mu_prisparam, cov_prisparam) are needed, found {sorted(data)}")
    mu, cov = np.asarray(mu, np.float64), np.asarray(cov, np.float64)
    if mu.shape not in ((36,), (1, 36)) or cov.shape != (36, 36):
        raise ValueError(f"niqe: {name}: mu_pris_param {mu.shape} and cov_pris_param {cov.shape}: (36,) or (1, 36), and (36, 36)")
    if not (np.isfinite(mu).all() and np.isfinite(cov).all()):
        raise ValueError(f"niqe: {name}: the pristine model holds non-finite entries")
    if data.get("gaussian_window") is not None:
        win = np.asarray(data["gaussian_window"], np.float64)
        if win.shape != (7, 7) or np.abs(win - gaussian_window()[1]).max() > 1e-6:
            raise ValueError(f"niqe: {name}: its gaussian_window is not the 7 x 7, sigma = 7 / 6 window of the definition: "
                             "a model fitted with another window is refused")
    return mu.reshape(36).copy(), cov.copy()


_DEVICE_TABLES: Dict = {}      # (h, w, device) -> ops.NiqeHalfTables


def clear_device_tables() -> None:
    """drop the resize tables cached on the device"""
    _DEVICE_TABLES.clear()


class NIQE:
    """`NIQE(params)(frames)`: the score of every frame.  `params`: what `load_niqe_params` reads, or its (mu, cov) result."""

    def __init__(self, params):
        if isinstance(params, tuple) and len(params) == 2:
            params = {"mu_pris_param": params[0], "cov_pris_param": params[1]}
        self.params = load_niqe_params(params)

    @staticmethod
    def blocks(h: int, w: int, crop_border: int = 0) -> Tuple[int, int]:
        return max(h - 2 * crop_border, 0) // BLOCK, max(w - 2 * crop_border, 0) // BLOCK

    def moments(self, frames, scale: float = 255.0, crop_border: int = 0):
        """(N, C, H, W) fp32 frames on the device -> (N, blocks, 50) fp64 on the device, a block's 25 moments at scale 1 followed by
        those of the same block position at scale 2: two `ops.niqe_moments` launches and one `ops.niqe_half`, nothing read back.
        None where the frame holds fewer than two blocks (the score is `nan`; nothing is launched)."""
        from . import ops
        if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
            raise ValueError(f"niqe: crop_border {crop_border!r}: a number of pixels >= 0")
        if frames.dim() != 4:
            raise ValueError(f"niqe: (N, C, H, W) frames, got {tuple(frames.shape)}")
        n, _, h, w = (int(v) for v in frames.shape)
        bh, bw = self.blocks(h, w, crop_border)
        if bh * bw < 2 or n < 1:
            return None
        ch, cw = bh * BLOCK, bw * BLOCK
        m1, luma = ops.niqe_moments(frames.detach(), scale, BLOCK, crop=(crop_border, crop_border, ch, cw))
        key = (ch, cw, str(frames.device))
        if key not in _DEVICE_TABLES:
            if len(_DEVICE_TABLES) >= 16:
                _DEVICE_TABLES.clear()
            _DEVICE_TABLES[key] = ops.niqe_half_tables(resize_tables(ch), resize_tables(cw), frames.device)
        m2, _ = ops.niqe_moments(ops.niqe_half(luma, _DEVICE_TABLES[key]), 1.0, BLOCK // 2)
        import torch
        return torch.cat([m1.view(n, bh * bw, 25), m2.view(n, bh * bw, 25)], dim=2)

    def scores(self, moments) -> List[float]:
        """`moments` of `self.moments`, read back ((N, blocks, 50), any array) -> one score per frame, on the host"""
        m = np.asarray(moments, np.float64)
        f1, f2 = features_from_moments(m[..., :25], BLOCK), features_from_moments(m[..., 25:], BLOCK // 2)
        return [score(f1[i], f2[i], self.params) for i in range(m.shape[0])]

    def __call__(self, frames, scale: float = 255.0, crop_border: int = 0) -> List[float]:
        m = self.moments(frames, scale, crop_border)
        if m is None:
            return [math.nan] * int(frames.shape[0])
        return self.scores(m.cpu().numpy())
