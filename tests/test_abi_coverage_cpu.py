"""CPU: a ledger of which GPU test reaches which C-ABI entry point, so that a kernel cannot lose (or never get) a direct test unnoticed.

For every name in ``_lib.EXPORTS`` some ``tests/test_*_gpu.py`` must either call the ``_lib`` wrapper that binds it (``L.<wrapper>(...)`` /
``_lib.<wrapper>(...)``) or name ``la_<name>`` in the docstring of a test that runs it (kernels reached through an autograd node or the
engine).  What neither holds for stands in ``EXEMPT`` with the higher-level test that covers it.  The decoder-side entry points that
tests/test_decoder_ops_gpu.py was written for may not be exempted: that module must reach each of them.
"""
import ast
import glob
import os
import re

from labelanything_amd import _lib

TESTS = os.path.dirname(os.path.abspath(__file__))
LIB_NAMES = {"L", "_lib"}                 # the names the GPU test modules bind labelanything_amd._lib to

# entry point -> the test that exercises it through the product's own Python layer (optimizer, loss, image / annotation preparation,
# an autograd node) and neither calls the wrapper itself nor names the symbol in its docstring
EXEMPT = {
    "la_bilinear_rows_bwd_set": "test_ops_gpu.py::test_bilinear_on_nhwc_rows_forward_and_backward",
    "la_error_count": "test_substitution_gpu.py::test_sampler_multi_tile_against_host",
    "la_error_points": "test_substitution_gpu.py::test_sampler_reproduces_the_reference_draws",
    "la_prompt_masks": "test_image_prep_gpu.py::test_prompt_masks_match_reference_apply_masks",
    "la_resample_u8": "test_image_prep_gpu.py::test_device_resample_is_bit_exact_with_pillow",
    "la_u8_to_chw_norm": "test_image_prep_gpu.py::test_device_preprocess_matches_reference_chain_bit_for_bit",
    "la_rle_scan": "test_rle_gpu.py::test_scan_gives_ends_and_areas",
    "la_rle_decode": "test_rle_gpu.py::test_decode_matches_the_fixture_and_the_definition",
    "la_rle_prompt_masks": "test_rle_gpu.py::test_prompt_masks_points_and_ground_truths_match_the_reference",
    "la_rle_ground_truth": "test_rle_gpu.py::test_prompt_masks_points_and_ground_truths_match_the_reference",
    "la_rle_points": "test_rle_gpu.py::test_points_at_the_first_and_last_rank_and_edge_shapes",
}

NEVER_EXEMPT = {
    "la_dense_pe", "la_point_embed", "la_mask_embed", "la_colmean", "la_class_mean", "la_classify", "la_classify_bwd", "la_add_cast",
    "la_nchw_to_nhwc", "la_nhwc_to_nchw", "la_post_final", "la_row_broadcast", "la_act_fwd", "la_act_bwd", "la_cast", "la_axpy", "la_attn_small",
}


def wrapper_bindings():
    """wrapper function of _lib.py -> the la_* symbols it calls (``lib().la_x`` attributes in its body)."""
    with open(_lib.__file__.replace(".pyc", ".py")) as fh:
        tree = ast.parse(fh.read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            syms = {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute) and n.attr in _lib.EXPORTS}
            if syms:
                out[node.name] = syms
    return out


def gpu_test_coverage():
    """la_* symbol -> the test ids (file::function) that call its wrapper or name it in their docstring."""
    binds = wrapper_bindings()
    cover = {}
    for path in sorted(glob.glob(os.path.join(TESTS, "test_*_gpu.py"))):
        with open(path) as fh:
            tree = ast.parse(fh.read())
        helpers = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and not n.name.startswith("test_")}

        def called(fn, seen):
            """Symbols bound by the wrappers that fn calls, following the module's own helper functions."""
            syms = set()
            for n in ast.walk(fn):
                if not isinstance(n, ast.Call):
                    continue
                f = n.func
                if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in LIB_NAMES and f.attr in binds:
                    syms |= binds[f.attr]
                elif isinstance(f, ast.Name) and f.id in helpers and f.id not in seen:
                    syms |= called(helpers[f.id], seen | {f.id})
            return syms

        for fn in tree.body:
            if not (isinstance(fn, ast.FunctionDef) and fn.name.startswith("test_")):
                continue
            tid = f"{os.path.basename(path)}::{fn.name}"
            doc = ast.get_docstring(fn) or ""
            for sym in called(fn, frozenset()) | {s for s in _lib.EXPORTS if re.search(rf"\b{s}\b", doc)}:
                cover.setdefault(sym, []).append(tid)
    return cover


def test_every_export_has_a_wrapper():
    """la_gemm_tn is la_gemm_tn_db without the bias gradient: ``_lib.gemm_tn`` binds the latter for both."""
    bound = set().union(*wrapper_bindings().values())
    assert sorted(set(_lib.EXPORTS) - bound) == ["la_gemm_tn"]


def test_every_entry_point_is_reached_by_a_gpu_test():
    cover = gpu_test_coverage()
    missing = sorted(s for s in _lib.EXPORTS if s not in cover and s not in EXEMPT)
    assert missing == [], f"no GPU test calls or names these entry points (add a test, or an EXEMPT entry with the covering test): {missing}"


def test_exemptions_are_few_current_and_never_the_decoder_kernels():
    cover = gpu_test_coverage()
    assert NEVER_EXEMPT <= set(_lib.EXPORTS)
    assert not (set(EXEMPT) & NEVER_EXEMPT), "the decoder-side entry points need a direct test"
    assert sorted(s for s in NEVER_EXEMPT if not any(t.startswith("test_decoder_ops_gpu.py::") for t in cover.get(s, []))) == []
    assert sorted(set(EXEMPT) - set(_lib.EXPORTS)) == [], "exemption for a symbol that is not exported"
    assert sorted(s for s in EXEMPT if s in cover) == [], "stale exemption: a GPU test reaches the entry point now"
    for sym, tid in EXEMPT.items():
        fname, _, func = tid.partition("::")
        with open(os.path.join(TESTS, fname)) as fh:
            names = {n.name for n in ast.parse(fh.read()).body if isinstance(n, ast.FunctionDef)}
        assert func in names, f"{sym}: covering test {tid} does not exist"
