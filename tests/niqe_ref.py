"""NIQE restated from its definition (Mittal et al., SPL 2013) in float64 with numpy and `math` only: what
eavsr_amd/niqe.py and csrc/niqe.hip are compared with.  Everything here works on block ARRAYS -- the features come straight from
`M[block]`, never from moments -- the correlate pads explicitly, and `imresize` is MATLAB's general form (any scale below 1, odd
lengths too), applied as a dense weight matrix per axis.

The local mean is defined separably (along W, then along H, taps in ascending order, every product and sum rounded on its own),
which is what makes the device's M the same bits as this file's and the sign counts equal; `window()` is the 2-D definition and
tests/test_niqe_host.py checks the outer product of the marginal against it."""
import math

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
GRID = np.arange(0.2, 10.001, 0.001)


def window():
    i = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def window1():
    i = np.arange(-3, 4, dtype=np.float64)
    e = np.exp(-(i * i) / (2.0 * (7.0 / 6.0) ** 2))
    return e / e.sum()


def quantise(frames, scale):
    """rint(clamp(v * scale, 0, 255)) in float32, as ops.frame_metrics quantises"""
    v = np.asarray(frames, np.float32) * np.float32(scale)
    return np.rint(np.minimum(np.maximum(v, np.float32(0)), np.float32(255))).astype(np.int64)


def luma(img8):
    """(C, H, W) integers 0..255 -> (H, W) integers: the channel itself, or BT.601 studio range with the tie decided in integers"""
    if img8.shape[0] == 1:
        return img8[0].astype(np.int64)
    out = np.empty(img8.shape[1:], np.int64)
    for y in range(img8.shape[1]):
        for x in range(img8.shape[2]):
            n = 65481 * int(img8[0, y, x]) + 128553 * int(img8[1, y, x]) + 24966 * int(img8[2, y, x])
            q, rem = divmod(n, 255000)
            if 2 * rem > 255000 or (2 * rem == 255000 and q % 2 == 1):
                q += 1
            out[y, x] = 16 + q
    return out


def crop(plane, crop_border=0, block=BLOCK):
    b = crop_border
    plane = plane[b:plane.shape[0] - b, b:plane.shape[1] - b] if b else plane
    return plane[:plane.shape[0] // block * block, :plane.shape[1] // block * block]


def correlate2d(img, g):
    """sum over the 7 x 7 window of g[i, j] * padded[y + i, x + j], replicate padding: the textbook form (scipy's mode='nearest')"""
    pad = np.pad(np.asarray(img, np.float64), 3, mode="edge")
    out = np.zeros(img.shape, np.float64)
    for i in range(7):
        for j in range(7):
            out += g[i, j] * pad[i:i + img.shape[0], j:j + img.shape[1]]
    return out


def correlate(img):
    """the same window applied separably: along W, then along H, taps in ascending order, explicit replicate padding"""
    g1 = window1()
    img = np.asarray(img, np.float64)
    h, w = img.shape
    pad = np.pad(img, ((0, 0), (3, 3)), mode="edge")
    a = np.zeros((h, w), np.float64)
    for k in range(7):
        a = a + g1[k] * pad[:, k:k + w]
    pad = np.pad(a, ((3, 3), (0, 0)), mode="edge")
    out = np.zeros((h, w), np.float64)
    for k in range(7):
        out = out + g1[k] * pad[k:k + h, :]
    return out


def mscn(plane):
    plane = np.asarray(plane, np.float64)
    mu = correlate(plane)
    sigma = np.sqrt(np.abs(correlate(plane * plane) - mu * mu))
    return (plane - mu) / (sigma + 1.0)


def cubic(x):
    x = abs(x)
    if x <= 1:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x <= 2:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def resize_matrix(length, scale):
    """MATLAB imresize's contributions along one axis as a dense (out, length) matrix, one output at a time"""
    out = int(math.ceil(length * scale))
    width = 4.0 / scale if scale < 1 else 4.0
    taps = int(math.ceil(width)) + 2
    mat = np.zeros((out, length), np.float64)
    for o in range(out):
        u = (o + 1) / scale + 0.5 * (1.0 - 1.0 / scale)
        left = math.floor(u - width / 2.0)
        idx = [left + t for t in range(taps)]
        wts = [(scale * cubic(scale * (u - i)) if scale < 1 else cubic(u - i)) for i in idx]
        total = sum(wts)
        for i, wt in zip(idx, wts):
            r = (i - 1) % (2 * length)             # 1-based index reflected symmetrically: .. 2, 1, 1, 2 ..
            r = r if r < length else 2 * length - 1 - r
            mat[o, r] += wt / total
    return mat


def imresize(img, scale):
    img = np.asarray(img, np.float64)
    rows = resize_matrix(img.shape[0], scale) @ img      # rows (along H) first
    return rows @ resize_matrix(img.shape[1], scale).T


def gamma_ratio(a):
    return math.gamma(2.0 / a) ** 2 / (math.gamma(1.0 / a) * math.gamma(3.0 / a))


_RHO = None


def rho_table():
    global _RHO
    if _RHO is None:
        _RHO = np.array([gamma_ratio(a) for a in GRID])
    return _RHO


def aggd(v):
    """-> (alpha, beta_l, beta_r, margin): margin = the relative gap between the best and the second-best grid distance"""
    v = np.asarray(v, np.float64).reshape(-1)
    neg, pos = v[v < 0], v[v > 0]
    if neg.size == 0 or pos.size == 0:
        return math.nan, math.nan, math.nan, math.inf
    left, right = math.sqrt(np.mean(neg * neg)), math.sqrt(np.mean(pos * pos))
    gam = left / right
    rhat = np.mean(np.abs(v)) ** 2 / np.mean(v * v)
    rhatn = rhat * (gam ** 3 + 1) * (gam + 1) / (gam ** 2 + 1) ** 2
    dist = (rho_table() - rhatn) ** 2
    best = int(np.argmin(dist))
    rest = np.delete(dist, best)
    margin = (rest.min() - dist[best]) / max(rest.min(), 1e-300)
    a = float(GRID[best])
    root = math.sqrt(math.gamma(1.0 / a) / math.gamma(3.0 / a))
    return a, left * root, right * root, margin


def block_features(m):
    """the 18 features of one block of M, and the smallest fit margin"""
    a, bl, br, margin = aggd(m)
    feats = [a, (bl + br) / 2.0]
    for shift in SHIFTS:
        a, bl, br, mg = aggd(m * np.roll(m, shift, axis=(0, 1)))
        margin = min(margin, mg)
        mean = (br - bl) * (math.gamma(2.0 / a) / math.gamma(1.0 / a)) if a == a else math.nan
        feats += [a, mean, bl, br]
    return np.array(feats, np.float64), margin


def block_moments(m):
    """the 25 numbers of ops.niqe_moments for one block of M, in numpy"""
    out = []
    for v in [m] + [m * np.roll(m, s, axis=(0, 1)) for s in SHIFTS]:
        neg, pos = v[v < 0], v[v > 0]
        out += [float(neg.size), float(pos.size), float(np.sum(neg * neg)), float(np.sum(pos * pos)), float(np.sum(np.abs(v)))]
    return np.array(out, np.float64)


def blocks_of(plane, block):
    bh, bw = plane.shape[0] // block, plane.shape[1] // block
    return [[plane[i * block:(i + 1) * block, j * block:(j + 1) * block] for j in range(bw)] for i in range(bh)]


def plane_moments(plane, block):
    """(blocks_h, blocks_w, 25) of a plane that holds whole blocks"""
    m = mscn(plane)
    return np.array([[block_moments(b) for b in row] for row in blocks_of(m, block)])


def plane_features(plane, block):
    """((blocks, 18) features, smallest margin) of a plane that holds whole blocks"""
    m = mscn(plane)
    feats, margin = [], math.inf
    for row in blocks_of(m, block):
        for b in row:
            f, mg = block_features(b)
            feats.append(f)
            margin = min(margin, mg)
    return np.array(feats), margin


def niqe(frame, mu_p, cov_p, scale=255.0, crop_border=0):
    """one frame (C, H, W) float32 -> (score, smallest fit margin, rows with a nan)"""
    y = crop(luma(quantise(frame, scale)), crop_border).astype(np.float64)
    if (y.shape[0] // BLOCK) * (y.shape[1] // BLOCK) < 2:
        return math.nan, math.inf, 0
    f1, m1 = plane_features(y, BLOCK)
    f2, m2 = plane_features(imresize(y, 0.5), BLOCK // 2)
    f = np.concatenate([f1, f2], axis=1)
    bad = np.isnan(f).any(axis=1)
    clean = f[~bad]
    if clean.shape[0] < 2:
        return math.nan, min(m1, m2), int(bad.sum())
    m = np.array([np.mean(col[~np.isnan(col)]) if (~np.isnan(col)).any() else math.nan for col in f.T])
    s = np.cov(clean, rowvar=False)
    d = (np.asarray(mu_p, np.float64).reshape(-1) - m)[None, :]
    return float(np.sqrt((d @ np.linalg.pinv((np.asarray(cov_p, np.float64) + s) / 2.0) @ d.T)[0, 0])), min(m1, m2), int(bad.sum())


def test_image(c, h, w, seed, constant_block=None, block=BLOCK):
    """noise plus gradients in [0, 1], float32 (C, h, w); `constant_block` = (i, j): that block and 3 samples around it are one
    grey level whose luma (64) the window reproduces exactly, so its M is 0 everywhere"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([0.45 + 0.25 * np.sin(0.013 * (k + 1) * yy + 0.021 * xx) + 0.2 * (xx / max(w - 1, 1) - 0.5) for k in range(c)])
    img = np.clip(img + rng.normal(0, 0.08, img.shape), 0, 1)
    if constant_block is not None:
        i, j = constant_block
        y0, y1, x0, x1 = max(i * block - 3, 0), (i + 1) * block + 3, max(j * block - 3, 0), (j + 1) * block + 3
        img[:, y0:y1, x0:x1] = (np.array([56, 56, 55]) if c == 3 else np.array([64]))[:, None, None] / 255.0
    return img.astype(np.float32)
