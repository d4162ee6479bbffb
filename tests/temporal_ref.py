"""The temporal metrics of DESIGN 7l restated in numpy, twice.

`temporal_ref32` follows the definition operation for operation in float32 -- every product, sum and difference is one numpy
float32 operation, rounded on its own, in the order the definition writes them -- and sums in float64: what csrc/temporal.hip must
reproduce (its `count` exactly; its sums up to the order of the float64 additions).
`temporal_ref64` is the same definition in float64 throughout, with the three constants taken as the float32 values of 0.01, 0.5 and
0.002: where every float32 operation of the definition happens to be exact (flows that are multiples of 1/8 pixel, 8-bit frames)
the two agree, which checks the restatement against itself.

Both take seq (F, C, H, W), fw / bw (F - 1, 2, H, W), an optional flow_b, and return (err float64 (F - 1,), count int64 (F - 1,),
epe float64 (F - 1,) or None)."""
import numpy as np

K_FB, K_FB0, K_G0 = np.float32(0.01), np.float32(0.5), np.float32(0.002)


def quantise(p, scale, dt):
    """rint(clamp(p * scale, 0, 255)), round half to even; a NaN sample clamps to 0 as fmaxf / fminf clamp it"""
    v = (p.astype(dt) * dt(scale)).astype(dt)
    return np.rint(np.fmin(np.fmax(v, dt(0)), dt(255))).astype(dt)


def _pair(cur, nxt, fw, bw, flow_b, scale, dt):
    C, H, W = cur.shape
    one = dt(1)
    with np.errstate(all="ignore"):
        u, v = fw[0].astype(dt), fw[1].astype(dt)
        xs = np.broadcast_to(np.arange(W, dtype=dt)[None, :], (H, W))
        ys = np.broadcast_to(np.arange(H, dtype=dt)[:, None], (H, W))
        sx, sy = (xs + u).astype(dt), (ys + v).astype(dt)
        inside = (sx >= 0) & (sx <= dt(W - 1)) & (sy >= 0) & (sy <= dt(H - 1))
        sx0, sy0 = np.where(inside, sx, dt(0)), np.where(inside, sy, dt(0))      # nothing is read for a pixel that is not inside
        fx0, fy0 = np.floor(sx0), np.floor(sy0)
        ax, ay = (sx0 - fx0).astype(dt), (sy0 - fy0).astype(dt)
        bx, by = (one - ax).astype(dt), (one - ay).astype(dt)
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)

        def bil(P):
            P = P.astype(dt)
            top = ((bx * P[y0, x0]).astype(dt) + (ax * P[y0, x1]).astype(dt)).astype(dt)
            bot = ((bx * P[y1, x0]).astype(dt) + (ax * P[y1, x1]).astype(dt)).astype(dt)
            return ((by * top).astype(dt) + (ay * bot).astype(dt)).astype(dt)

        sq = lambda a: (a * a).astype(dt)
        bu, bv = bil(bw[0]), bil(bw[1])
        m_f = (sq(u) + sq(v)).astype(dt)
        m_b = (sq(bu) + sq(bv)).astype(dt)
        m_fb = (sq((u + bu).astype(dt)) + sq((v + bv).astype(dt))).astype(dt)
        xr, yd = np.minimum(np.arange(W) + 1, W - 1), np.minimum(np.arange(H) + 1, H - 1)
        gx = (sq((u[:, xr] - u).astype(dt)) + sq((v[:, xr] - v).astype(dt))).astype(dt)
        gy = (sq((u[yd, :] - u).astype(dt)) + sq((v[yd, :] - v).astype(dt))).astype(dt)
        g = (gx + gy).astype(dt)
        lim_fb = ((dt(K_FB) * (m_f + m_b).astype(dt)).astype(dt) + dt(K_FB0)).astype(dt)
        lim_g = ((dt(K_FB) * m_f).astype(dt) + dt(K_G0)).astype(dt)
        valid = inside & (m_fb <= lim_fb) & (g <= lim_g)      # a comparison with a NaN is False
        err = 0.0
        for c in range(C):
            d = (quantise(cur[c], scale, dt) - bil(quantise(nxt[c], scale, dt))).astype(dt)
            d64 = d.astype(np.float64)
            err += float(np.sum((d64 * d64)[valid], dtype=np.float64))
        epe = None
        if flow_b is not None:
            eu = (flow_b[0].astype(dt) - u).astype(dt).astype(np.float64)
            ev = (flow_b[1].astype(dt) - v).astype(dt).astype(np.float64)
            epe = float(np.sum(np.sqrt(eu * eu + ev * ev), dtype=np.float64))
    return err, int(valid.sum()), epe, valid


def _run(seq, fw, bw, scale, flow_b, dt, masks):
    seq, fw, bw = np.asarray(seq), np.asarray(fw), np.asarray(bw)
    F = seq.shape[0]
    assert seq.ndim == 4 and F >= 2 and fw.shape == bw.shape == (F - 1, 2) + seq.shape[2:]
    rows = [_pair(seq[t], seq[t + 1], fw[t], bw[t], None if flow_b is None else np.asarray(flow_b)[t], scale, dt) for t in range(F - 1)]
    err = np.array([r[0] for r in rows], np.float64)
    count = np.array([r[1] for r in rows], np.int64)
    epe = None if flow_b is None else np.array([r[2] for r in rows], np.float64)
    if masks:
        return err, count, epe, np.stack([r[3] for r in rows], 0)
    return err, count, epe


def temporal_ref32(seq, fw, bw, scale=255.0, flow_b=None, masks=False):
    return _run(seq, fw, bw, scale, flow_b, np.float32, masks)


def temporal_ref64(seq, fw, bw, scale=255.0, flow_b=None, masks=False):
    return _run(seq, fw, bw, scale, flow_b, np.float64, masks)
