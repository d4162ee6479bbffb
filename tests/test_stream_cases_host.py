"""tests/stream_cases.py against eavsr_amd.ops, on the host: every public function that hands a stream to the library is classified
-- a row of the table, a model op that a whole-model graph test runs, or lab-only -- so that a function a later change adds, and
nobody classifies, fails here."""
import inspect

from tests import stream_cases as S


def _ops():
    from eavsr_amd import ops
    return ops


def _public(ops):
    return {n: f for n, f in vars(ops).items() if not n.startswith("_") and inspect.isfunction(f) and f.__module__ == ops.__name__}


def test_every_op_that_passes_a_stream_is_classified():
    ops = _ops()
    rows = {r.op for r in S.ROWS}
    takes_stream = sorted(n for n, f in _public(ops).items() if "_stream(" in inspect.getsource(f))
    assert len(takes_stream) > 60      # the scan sees the library's wrappers
    unclassified = [n for n in takes_stream if n not in rows and n not in S.MODEL_OPS and n not in S.LAB_ONLY]
    assert not unclassified, (f"{unclassified}: give each a row in tests/stream_cases.py (or name it in MODEL_OPS with the whole-model "
                              "graph test that runs it, or in LAB_ONLY)")


def test_the_table_names_existing_public_functions_once():
    public = _public(_ops())
    names = [r.name for r in S.ROWS]
    assert len(set(names)) == len(names)
    for r in S.ROWS:
        assert r.op in public, f"row {r.name}: ops.{r.op} does not exist"
        assert r.name == r.op or r.name.startswith(r.op + "-"), r.name
    for table in (S.MODEL_OPS, S.LAB_ONLY):
        for n in table:
            assert n in public, f"ops.{n} does not exist"
            assert n not in {r.op for r in S.ROWS}, f"ops.{n} is a row and is also classified away"
    assert not set(S.MODEL_OPS) & set(S.LAB_ONLY)
    # a model op names the whole-model graph test that runs it, and that test exists
    import glob
    import os
    import re
    defined = set()
    for path in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_*.py")):
        with open(path) as f:
            defined.update(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
    for n, test in S.MODEL_OPS.items():
        assert isinstance(test, str) and test in defined, f"MODEL_OPS[{n!r}] = {test!r} is no test function under tests/"
    for n in S.LAB_ONLY:
        assert "require_lab(" in inspect.getsource(public[n])


def test_the_required_rows_are_there():
    required = ("rgb8 u8_to_f32 ingest_pad ingest_window tile_blend dihedral blend_dihedral pack16 pack16_census unpack16 frame_change "
                "gather_pairs resize_cubic_u8 png_filter deflate_huffman png_encode png_unfilter frame_metrics temporal_metrics niqe_moments "
                "niqe_half lpips_conv1 lpips_conv lpips_maxpool lpips_tap pwc_conv3x3 pwc_deconv4x4s2 pwc_correlation pwc_backwarp normalize "
                "avg_pool2 resize_bilinear concat3").split()
    rows = [r.op for r in S.ROWS]
    assert not [n for n in required if n not in rows]
    assert rows.count("u8_to_f32") == 2 and rows.count("blend_dihedral") == 2 and rows.count("png_unfilter") == 2


def test_the_exception_sets_hold_rows_only_each_with_a_reason():
    names = {r.name for r in S.ROWS}
    for table in (S.HOST_SYNC, S.NOT_CAPTURED):
        for n, why in table.items():
            assert n in names, n
            assert isinstance(why, str) and len(why) > 20, n
    assert set(S.NOT_CAPTURED) <= {"png_unfilter-wide"}
    ops = _ops()
    for n, why in S.HOST_SYNC.items():      # the reason quotes the docstring's promise of a host value
        doc = " ".join(getattr(ops, next(r.op for r in S.ROWS if r.name == n)).__doc__.split())
        assert why.split('"')[1] in doc, n


def test_the_lds_row_length_is_read_from_the_kernel_source():
    assert S.lds_pixels() >= 1
