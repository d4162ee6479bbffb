"""numpy oracle of the scene-cut statistics (`ops.frame_change`, csrc/scene.hip), written from the definition alone -- it shares no
code with the product:

    Y = (77 R + 150 G + 29 B + 128) >> 8 for three channels, Y = v for one
    hist[f][Y >> 2] = pixels of frame f with that luma bin (int32, 64 bins)
    sad[f]          = sum over the pixels of |Y_f - Y_{f+1}| (int64, F - 1 entries)

frames: uint8 array (F, C, h, w), C 1 or 3, or (F, h, w, 3) with hwc=True.
"""
import numpy as np


def luma(frames, hwc=False):
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.ndim == 4
    if hwc:
        assert a.shape[3] == 3
        a = np.moveaxis(a, 3, 1)
    if a.shape[1] == 1:
        return a[:, 0].astype(np.int64)
    assert a.shape[1] == 3
    r, g, b = (a[:, c].astype(np.int64) for c in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def frame_change(frames, hwc=False):
    y = luma(frames, hwc)
    f = y.shape[0]
    hist = np.stack([np.bincount((y[i] >> 2).ravel(), minlength=64) for i in range(f)]).astype(np.int32)
    sad = np.array([np.abs(y[i] - y[i + 1]).sum() for i in range(f - 1)], dtype=np.int64)
    return hist, sad
