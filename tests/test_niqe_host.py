"""NIQE on the host: the window, the resize tables and the integer luma; `niqe.features_from_moments` and `niqe.score`
against the block-array restatement (tests/niqe_ref.py); the loader, the option forms, `scene_report` and the log; the C ABI; and a
transcription of both kernels' address arithmetic against numpy slicing.  No GPU."""
import math
import os
import re
from argparse import Namespace

import numpy as np
import pytest

from eavsr_amd import harness
from eavsr_amd import niqe as Q
from tests import niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS_HALF = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.float64) / 256


def _model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (36, 36))
    return rng.normal(0, 1, 36), a @ a.T + np.eye(36)


# ------------------------------------------------------------------------------------------------ window, tables, luma
def test_window_sums_to_one_and_is_the_outer_product_of_its_marginal():
    g1, g = Q.gaussian_window()
    assert g.shape == (7, 7) and g1.shape == (7,)
    assert abs(g.sum() - 1) <= 1e-15 and abs(g1.sum() - 1) <= 1e-15
    assert np.abs(np.outer(g1, g1) - g).max() <= 1e-15
    assert np.array_equal(g, R.window()) and np.array_equal(g1, R.window1())
    i = np.arange(-3, 4)
    assert np.allclose(g / g[3, 3], np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2 * (7 / 6) ** 2)), rtol=1e-14)


def test_separable_correlate_is_the_two_dimensional_one():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (23, 31)).astype(np.float64)
    assert np.abs(R.correlate(img) - R.correlate2d(img, R.window())).max() <= 1e-12


def test_reference_correlate_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (23, 31)).astype(np.float64)
    want = ndimage.correlate(img, R.window(), mode="nearest")
    assert np.abs(R.correlate2d(img, R.window()) - want).max() <= 1e-12 and np.abs(R.correlate(img) - want).max() <= 1e-12


@pytest.mark.parametrize("length", [48, 96, 10])
def test_resize_tables_at_half_size(length):
    idx, w = Q.resize_tables(length, 0.5)
    out = length // 2
    assert idx.shape == w.shape == (out, 8) and idx.dtype == np.int32 and w.dtype == np.float64
    for o in range(out):
        taps = np.arange(2 * o - 3, 2 * o + 5)
        if taps[0] >= 0 and taps[-1] < length:      # interior: the eight weights, exactly
            assert idx[o].tolist() == taps.tolist() and np.array_equal(w[o], WEIGHTS_HALF)
    # the first and last two outputs: indices reflected symmetrically (.. 1, 0, 0, 1 ..), weights unchanged
    reflect = lambda i: (-1 - i) if i < 0 else (2 * length - 1 - i if i >= length else i)
    for o in (0, 1, out - 2, out - 1):
        assert idx[o].tolist() == [reflect(i) for i in range(2 * o - 3, 2 * o + 5)], (length, o)
        assert np.array_equal(w[o], WEIGHTS_HALF)
    assert idx[0].tolist()[:4] == [2, 1, 0, 0] and idx[out - 1].tolist()[-4:] == [length - 1, length - 1, length - 2, length - 3]


@pytest.mark.parametrize("length,scale", [(48, 0.5), (96, 0.5), (10, 0.5), (11, 0.5), (37, 0.3), (20, 0.75), (9, 1.0)])
def test_resize_tables_equal_the_general_imresize(length, scale):
    idx, w = Q.resize_tables(length, scale)
    dense = np.zeros((idx.shape[0], length))
    for o in range(idx.shape[0]):
        for k in range(idx.shape[1]):
            dense[o, idx[o, k]] += w[o, k]
    assert idx.min() >= 0 and idx.max() < length
    assert np.abs(dense - R.resize_matrix(length, scale)).max() <= 1e-15
    assert np.abs(w.sum(axis=1) - 1).max() <= 1e-15


def test_general_imresize_reproduces_a_constant_image():
    for shape, scale in (((13, 20), 0.37), ((96, 192), 0.5), ((11, 7), 0.5)):
        out = R.imresize(np.full(shape, 7.0), scale)
        assert out.shape == (math.ceil(shape[0] * scale), math.ceil(shape[1] * scale)) and np.abs(out - 7.0).max() <= 1e-13


def test_integer_luma():
    assert int(Q.luma601(0, 0, 0)) == 16 and int(Q.luma601(255, 255, 255)) == 235
    # a tie by hand: 65481 * 0 + 128553 * 204 + 24966 * 68 = 27 922 500 = 109.5 * 255000 -> half to even: 110 -> Y = 126
    assert 128553 * 204 + 24966 * 68 == 27922500 and 2 * 27922500 == 219 * 255000
    assert int(Q.luma601(0, 204, 68)) == 16 + 110
    # and one that rounds down to even: find it among the ties
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    n = 65481 * r + 128553 * g + 24966 * b
    ties = 2 * (n % 255000) == 255000
    assert int(ties.sum()) == 194      # the count DESIGN 7m quotes
    y = Q.luma601(r, g, b)
    q = n // 255000
    assert ((y[ties] - 16) % 2 == 0).all() and (np.abs(y[ties] - 16 - q[ties] - 0.5) == 0.5).all()
    assert ((y - 16)[~ties] == np.floor(n[~ties] / 255000 + 0.5)).all() and y.min() == 16 and y.max() == 235
    pix = np.array([[[0]], [[204]], [[68]]])
    assert int(R.luma(pix)[0, 0]) == 126 and np.array_equal(R.luma(np.array([[[7, 200]]])), [[7, 200]])


# ------------------------------------------------------------------------------------------------ features and score
def _plane(seed, h=96, w=192):
    return R.crop(R.luma(R.quantise(R.test_image(3, h, w, seed), 255.0))).astype(np.float64)


@pytest.mark.parametrize("seed,block", [(11, 96), (12, 96), (13, 48)])
def test_features_from_moments_equal_the_block_array_restatement(seed, block):
    plane = _plane(seed) if block == 96 else R.imresize(_plane(seed), 0.5)
    want, margin = R.plane_features(plane, block)
    assert margin > 1e-9, margin      # no fit near a tie between two grid values: alpha is then the same on both sides
    got = Q.features_from_moments(R.plane_moments(plane, block), block).reshape(-1, 18)
    assert got.shape == want.shape and np.isfinite(want).all()
    alphas = [0] + [4 * j - 2 for j in range(1, 5)]
    assert np.array_equal(got[:, alphas], want[:, alphas])
    assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all(), np.abs(got / want - 1).max()


@pytest.mark.parametrize("shape", [2.0, 1.0])
def test_a_generalised_gaussian_sample_recovers_its_shape(shape):
    rng = np.random.default_rng(5)
    n = 480 * 480      # a sample of a generalised gaussian: sign * gamma(1 / shape)^(1 / shape)
    v = (rng.gamma(1.0 / shape, 1.0, n) ** (1.0 / shape) * rng.choice([-1.0, 1.0], n)).reshape(480, 480)
    mom = np.array([float((v < 0).sum()), float((v > 0).sum()), (v[v < 0] ** 2).sum(), (v[v > 0] ** 2).sum(), np.abs(v).sum()] * 5)
    got = Q.features_from_moments(mom, 480)
    assert abs(got[0] - shape) <= 0.05
    assert abs(R.aggd(v)[0] - shape) <= 0.05 and got[0] == R.aggd(v)[0]


def test_nan_rows():
    plane = _plane(14, 96, 288)
    plane[:, 96:192] = 64.0      # the middle block is constant, and 64 is reproduced by the window exactly
    plane[:, 93:195] = 64.0
    mom = R.plane_moments(plane, 96)
    assert (mom[0, 1, [0, 1]] == 0).all() and mom[0, 0, 0] > 0
    f = Q.features_from_moments(mom, 96).reshape(-1, 18)
    assert np.isnan(f[1]).all() and np.isfinite(f[[0, 2]]).all()
    ref_f, _ = R.plane_features(plane, 96)
    assert np.isnan(ref_f[1]).all()
    params = _model()
    # the nan row is left out of m and S: the score is that of the two clean rows alone
    want = Q.score(f[[0, 2]], f[[0, 2]], params)
    assert math.isfinite(want) and Q.score(f, f, params) == want
    # ... and a row that is nan at one scale only still counts in the columns where it has a value
    g = f.copy()
    g[1] = f[0] * 1.5
    mixed = Q.score(g, f, params)
    full = np.concatenate([g, f], axis=1)
    m = np.array([np.nanmean(full[:, k]) for k in range(36)])
    s = np.cov(full[[0, 2]], rowvar=False)
    d = (params[0] - m)[None]
    assert abs(mixed - math.sqrt((d @ np.linalg.pinv((params[1] + s) / 2) @ d.T)[0, 0])) <= 1e-12 * mixed
    # fewer than two clean rows
    assert math.isnan(Q.score(f[:2], f[:2], params)) and math.isnan(Q.score(f[1:2], f[1:2], params))


def test_score_equals_the_restatement():
    img = R.test_image(3, 96, 192, 11)
    mu_p, cov_p = _model(3)
    want, margin, bad = R.niqe(img, mu_p, cov_p)
    assert margin > 1e-9 and bad == 0 and math.isfinite(want)
    y = _plane(11)
    f1 = Q.features_from_moments(R.plane_moments(y, 96), 96)
    f2 = Q.features_from_moments(R.plane_moments(R.imresize(y, 0.5), 48), 48)
    got = Q.score(f1, f2, (mu_p, cov_p))
    assert abs(got - want) <= 1e-9 * want
    assert math.isnan(R.niqe(img[:, :, :96], mu_p, cov_p)[0])


# ------------------------------------------------------------------------------------------------ the interface
def test_loader_reads_and_refuses(tmp_path):
    mu, cov = _model()
    good = str(tmp_path / "model.npz")
    np.savez(good, mu_pris_param=mu[None, :], cov_pris_param=cov, gaussian_window=Q.gaussian_window()[1] + 1e-8)
    got = Q.load_niqe_params(good)
    assert np.array_equal(got[0], mu) and got[0].shape == (36,) and np.array_equal(got[1], cov)
    got = Q.load_niqe_params({"mu_prisparam": mu, "cov_prisparam": cov})
    assert np.array_equal(got[0], mu)
    assert np.array_equal(Q.NIQE(good).params[1], cov) and np.array_equal(Q.NIQE((mu, cov)).params[0], mu)

    def refused(match, **arrays):
        path = str(tmp_path / "bad.npz")
        np.savez(path, **arrays)
        with pytest.raises(ValueError, match=match) as e:
            Q.load_niqe_params(path)
        assert "bad.npz" in str(e.value)
    with pytest.raises(ValueError, match="no-such-model.npz"):
        Q.load_niqe_params(str(tmp_path / "no-such-model.npz"))
    refused("are needed", mu_pris_param=mu)
    refused(r"\(36,\) or \(1, 36\)", mu_pris_param=mu[:35], cov_pris_param=cov)
    refused(r"\(36, 36\)", mu_pris_param=mu, cov_pris_param=cov[:35])
    refused("non-finite", mu_pris_param=np.where(np.arange(36) == 3, np.nan, mu), cov_pris_param=cov)
    refused("non-finite", mu_pris_param=mu, cov_pris_param=cov + np.where(np.eye(36) > 0, np.inf, 0))
    refused("gaussian_window", mu_pris_param=mu, cov_pris_param=cov, gaussian_window=Q.gaussian_window()[1] + 1e-5)
    refused("gaussian_window", mu_pris_param=mu, cov_pris_param=cov, gaussian_window=np.ones((5, 5)) / 25)
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not a zip file")
    with pytest.raises(ValueError, match="junk.npz"):
        Q.load_niqe_params(str(junk))
    with pytest.raises(ValueError, match="file name or a mapping"):
        Q.load_niqe_params(3)


def test_every_spelling_of_the_option(tmp_path, monkeypatch):
    mu, cov = _model()
    path = str(tmp_path / "model.npz")
    np.savez(path, mu_pris_param=mu, cov_pris_param=cov)
    monkeypatch.delenv("EAVSR_NIQE", raising=False)
    assert harness.niqe_option(None) == (None, 0) and harness.niqe_option(Namespace()) == (None, 0)
    assert harness.niqe_option(Namespace(niqe_path=path, niqe_crop=5)) == (path, 5)
    monkeypatch.setenv("EAVSR_NIQE", path)
    assert harness.niqe_option(None) == (path, 0) and harness.niqe_option(Namespace(niqe_path="other.npz"))[0] == "other.npz"
    monkeypatch.setenv("EAVSR_NIQE", "")
    assert harness.niqe_option(None) == (None, 0)
    monkeypatch.delenv("EAVSR_NIQE")
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="niqe_crop"):
            harness.niqe_option(Namespace(niqe_crop=bad))
    with pytest.raises(ValueError, match="niqe_path"):
        harness.niqe_option(Namespace(niqe_path=3))
    scorer = Q.NIQE(path)
    assert harness.niqe_scorer(scorer) is scorer
    assert np.array_equal(harness.niqe_scorer(path).params[0], mu)
    assert np.array_equal(harness.niqe_scorer(True, Namespace(niqe_path=path)).params[0], mu)
    assert np.array_equal(harness.niqe_scorer({"mu_pris_param": mu, "cov_pris_param": cov}).params[1], cov)
    with pytest.raises(ValueError, match="opt.niqe_path"):
        harness.niqe_scorer(True, Namespace())
    with pytest.raises(ValueError, match="missing.npz"):
        harness.niqe_scorer(str(tmp_path / "missing.npz"))
    with pytest.raises(ValueError, match="niqe=3"):
        harness.niqe_scorer(3)
    # the arguments of evaluate / super_resolve: None reads the options, False is off whatever they say
    opt = Namespace(niqe_path=path, niqe_crop=4)
    got, crop = harness._resolve_niqe(None, None, opt, "t")
    assert isinstance(got, Q.NIQE) and crop == 4
    assert harness._resolve_niqe(False, None, opt, "t") == (None, 4) and harness._resolve_niqe(None, None, None, "t") == (None, 0)
    assert harness._resolve_niqe(scorer, 7, opt, "t") == (scorer, 7)
    with pytest.raises(ValueError, match="t: niqe_crop"):
        harness._resolve_niqe(scorer, -2, opt, "t")
    with pytest.raises(ValueError, match="per_frame"):
        harness.evaluate(None, [], niqe=scorer)


def test_scene_report_and_log_with_and_without_the_column(tmp_path):
    names = ["000_00000.png", "000_00001.png", "001_00000.png", "001_00001.png"]
    psnr, ssim = [30.0, 32.0, 28.0, math.inf], [0.9, 0.92, 0.88, 1.0]
    temporal = {"ewarp": [None, 0.001, None, math.nan], "tof": None}
    plain = harness.scene_report(names, psnr, ssim)
    old = ("scene 000\n  000_00000.png  psnr 30.00  ssim 0.9000\n  000_00001.png  psnr 32.00  ssim 0.9200\n"
           "  mean of 2 frames  psnr 31.00  ssim 0.9100\nscene 001\n  001_00000.png  psnr 28.00  ssim 0.8800\n"
           "  001_00001.png  psnr inf  ssim 1.0000\n  mean of 2 frames  psnr inf  ssim 0.9400\n"
           "final, mean of 2 scenes  psnr inf  ssim 0.9250\n")
    assert open(harness.write_metrics_log(plain, str(tmp_path / "a.txt"))).read() == old
    assert set(plain["final"]) == {"psnr", "ssim", "scenes"} and set(plain["frames"][0]) == {"name", "scene", "psnr", "ssim"}
    full = harness.scene_report(names, psnr, ssim, [0.1, 0.2, 0.3, 0.4], temporal)
    text_full = open(harness.write_metrics_log(full, str(tmp_path / "b.txt"))).read()
    assert "  lpips 0.100  ewarp -  tof -\n" in text_full and "ewarp nan" in text_full and "niqe" not in text_full
    # with the column: every old field and every old byte is there, the column is appended
    vals = [4.5, math.nan, 6.25, 7.75]
    rep = harness.scene_report(names, psnr, ssim, [0.1, 0.2, 0.3, 0.4], temporal, niqe=vals)
    for fr, fr_old, v in zip(rep["frames"], full["frames"], vals):
        assert {k: fr[k] for k in fr_old if k != "ewarp"} == {k: fr_old[k] for k in fr_old if k != "ewarp"}
        assert fr["niqe"] == v or (v != v and fr["niqe"] != fr["niqe"])
    assert rep["scenes"]["000"]["niqe"] == 4.5 and rep["scenes"]["001"]["niqe"] == 7.0 and rep["final"]["niqe"] == 5.75
    assert rep["final"]["psnr"] == full["final"]["psnr"] and rep["final"]["lpips"] == full["final"]["lpips"]
    lines_full = text_full.splitlines()
    lines = open(harness.write_metrics_log(rep, str(tmp_path / "c.txt"))).read().splitlines()
    tails = [ln[len(o):] for ln, o in zip(lines, lines_full)]
    assert len(lines) == len(lines_full) and all(ln.startswith(o) for ln, o in zip(lines, lines_full))
    assert tails == ["", "  niqe 4.5000", "  niqe -", "  niqe 4.5000", "", "  niqe 6.2500", "  niqe 7.7500", "  niqe 7.0000", "  niqe 5.7500"]
    # every score nan: None in the means, `-` in the log
    rep = harness.scene_report(names[:2], psnr[:2], ssim[:2], niqe=[math.nan, math.nan])
    assert rep["scenes"]["000"]["niqe"] is None and rep["final"]["niqe"] is None
    assert open(harness.write_metrics_log(rep, str(tmp_path / "d.txt"))).read().splitlines()[-1] == \
        "final, mean of 1 scenes  psnr 31.00  ssim 0.9100  niqe -"
    # footage without ground truth: the names and the column only
    rep = harness.scene_report(names, None, None, niqe=vals)
    assert [set(fr) for fr in rep["frames"]] == [{"name", "scene", "niqe"}] * 4
    assert rep["scenes"]["001"] == {"frames": 2, "niqe": 7.0} and rep["final"] == {"scenes": 2, "niqe": 5.75}
    assert open(harness.write_metrics_log(rep, str(tmp_path / "e.txt"))).read() == (
        "scene 000\n  000_00000.png  niqe 4.5000\n  000_00001.png  niqe -\n  mean of 2 frames  niqe 4.5000\nscene 001\n"
        "  001_00000.png  niqe 6.2500\n  001_00001.png  niqe 7.7500\n  mean of 2 frames  niqe 7.0000\nfinal, mean of 2 scenes  niqe 5.7500\n")
    with pytest.raises(ValueError, match="needs niqe"):
        harness.scene_report(names, None, None)
    with pytest.raises(ValueError, match="together"):
        harness.scene_report(names, psnr, None, niqe=vals)
    with pytest.raises(ValueError, match="3 NIQE values"):
        harness.scene_report(names, psnr, ssim, niqe=vals[:3])


def test_c_abi_symbols():
    from eavsr_amd import _native
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header.split("EXPERIMENTAL -- exported by the LAB build only")[0]
    source = open(os.path.join(ROOT, "eavsr_amd", "csrc", "niqe.hip")).read()
    for name, args in (("eavsr_niqe_moments", 16), ("eavsr_niqe_half_f64", 16)):
        assert name in _native.SIGNATURES and name not in _native.LAB_SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == args
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", stable)
        assert decl is not None and decl.group(1).count(",") == args - 1, name
        assert re.search(r'extern "C" int ' + name + r"\(", source)
    from eavsr_amd import build
    assert build.PER_FILE_FLAGS["niqe.hip"] == ["-ffp-contract=off"]
    assert os.path.join(build.CSRC, "niqe.hip") in build.sources() and "niqe.hip" not in build.LAB_SOURCES


# ------------------------------------------------------------------------------------------------ the kernels' address arithmetic
STRIP, HALO = 16, 3


def _moments_kernel(src, y0, x0, p, bh, bw, by, bx):
    """csrc/niqe.hip niqe_moments_kernel for one workgroup, index by index: the staged tile, the strips, M, the rolled reads"""
    g = Q.gaussian_window()[0]
    tp = p + 2 * HALO
    ch, cw = bh * p, bw * p
    tile = np.empty(tp * tp)
    luma = {}
    for i in range(tp * tp):
        ty, tx = divmod(i, tp)
        cy, cx = by * p + ty - HALO, bx * p + tx - HALO
        gy, gx = min(max(cy, 0), ch - 1), min(max(cx, 0), cw - 1)
        tile[i] = src[y0 + gy, x0 + gx]
        if HALO <= ty < HALO + p and HALO <= tx < HALO + p:
            luma[(cy, cx)] = tile[i]
    m = np.empty(p * p)
    for s0 in range(0, p, STRIP):
        rows = min(STRIP, p - s0)
        h1, h2 = np.empty((rows + 2 * HALO) * p), np.empty((rows + 2 * HALO) * p)
        for i in range((rows + 2 * HALO) * p):
            r, x = divmod(i, p)
            a = b = 0.0
            for k in range(7):
                v = tile[(s0 + r) * tp + x + k]
                a += g[k] * v
                b += g[k] * (v * v)
            h1[i], h2[i] = a, b
        for i in range(rows * p):
            r, x = divmod(i, p)
            mu = e2 = 0.0
            for k in range(7):
                mu += g[k] * h1[(r + k) * p + x]
                e2 += g[k] * h2[(r + k) * p + x]
            v = tile[(s0 + r + HALO) * tp + x + HALO]
            m[(s0 + r) * p + x] = (v - mu) / (math.sqrt(abs(e2 - mu * mu)) + 1.0)
    maps = np.empty((5, p * p))
    for i in range(p * p):
        y, x = divmod(i, p)
        ym, xm, xp = (y - 1 if y else p - 1), (x - 1 if x else p - 1), (x + 1 if x + 1 < p else 0)
        maps[:, i] = [m[i], m[i] * m[y * p + xm], m[i] * m[ym * p + x], m[i] * m[ym * p + xm], m[i] * m[ym * p + xp]]
    return m.reshape(p, p), maps.reshape(5, p, p), luma


def test_moments_kernel_arithmetic_against_numpy_slicing():
    rng = np.random.default_rng(8)
    p, bh, bw, y0, x0 = 20, 2, 3, 5, 2      # 20 = a strip of 16 and one of 4: a seam inside every block; 2 x 3 blocks: every edge
    src = rng.integers(0, 256, (y0 + bh * p + 7, x0 + bw * p + 9)).astype(np.float64)
    plane = src[y0:y0 + bh * p, x0:x0 + bw * p]
    want = R.mscn(plane)      # replicates at the CROPPED plane's edges, not the frame's
    seen = {}
    for by in range(bh):
        for bx in range(bw):
            m, maps, luma = _moments_kernel(src, y0, x0, p, bh, bw, by, bx)
            blk = want[by * p:(by + 1) * p, bx * p:(bx + 1) * p]
            assert np.array_equal(m, blk), (by, bx)      # the same bits: the same operations in the same order
            assert np.array_equal(maps[0], blk)
            for j, shift in enumerate(R.SHIFTS):
                assert np.array_equal(maps[j + 1], blk * np.roll(blk, shift, axis=(0, 1))), (by, bx, shift)
            seen.update(luma)
    assert len(seen) == plane.size and all(plane[k] == v for k, v in seen.items())


def _half_kernel(plane, rows, cols, tile_y=8, tile_x=32):
    (ridx, rw), (cidx, cw) = rows, cols
    H, W = plane.shape
    h, w = ridx.shape[0], cidx.shape[0]
    runs = [cidx[a:a + tile_x] for a in range(0, w, tile_x)]
    col_lo = [int(r.min()) for r in runs]
    span = max(int(r.max()) - int(r.min()) + 1 for r in runs)
    out = np.full((h, w), np.nan)
    for bx in range(-(-w // tile_x)):
        for by in range(-(-h // tile_y)):
            lo = min(max(col_lo[bx], 0), W - 1)
            tmp = np.zeros(tile_y * span)
            for i in range(tile_y * span):
                r, j = divmod(i, span)
                oy, c = by * tile_y + r, min(lo + j, W - 1)
                if oy < h:
                    a = 0.0
                    for k in range(ridx.shape[1]):
                        a += rw[oy, k] * plane[min(max(ridx[oy, k], 0), H - 1), c]
                    tmp[i] = a
            for i in range(tile_y * tile_x):
                r, jx = divmod(i, tile_x)
                oy, ox = by * tile_y + r, bx * tile_x + jx
                if oy >= h or ox >= w:
                    continue
                a = 0.0
                for k in range(cidx.shape[1]):
                    a += cw[ox, k] * tmp[r * span + min(max(cidx[ox, k] - lo, 0), span - 1)]
                out[oy, ox] = a
    return out, span


@pytest.mark.parametrize("shape", [(20, 70), (18, 136)])
def test_half_kernel_arithmetic_against_the_general_imresize(shape):
    rng = np.random.default_rng(9)
    plane = rng.random(shape) * 255
    got, span = _half_kernel(plane, Q.resize_tables(shape[0]), Q.resize_tables(shape[1]))
    assert span <= 2 * 32 + 6
    assert got.shape == (shape[0] // 2, shape[1] // 2) and np.abs(got - R.imresize(plane, 0.5)).max() <= 1e-12
