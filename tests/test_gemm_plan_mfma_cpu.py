"""CPU: LaGemmPlan.mfma, the MFMA shape of the four-wave main loop, over the literal dispatch table of tests/test_gemm_plan_cpu.py.

The field says 16x16x32 exactly where an instance exists and was measured ahead (profiles/r12_mfma_shape.md): gemm_t256w with its direct
epilogue, except EPI 12, the ragged EPI 9 instance and the residual epilogues (EPI 3, 7, 10, 11) below K = 1536; ``GEMM_VARIANT_MFMA32`` keeps 32x32x16 there.  Either way every other field of
every row - kernel, epilogue, grid, workgroup, LDS - is what the table says: the shape changes nothing about the launch.
"""
import pytest

from labelanything_amd import _lib as L
from tests.test_gemm_plan_cpu import A, BIAS, NCU, O16, O32, RES, TABLE, T256W, W


def _ask(c, variant):
    prev = L.gemm_variant(variant)
    try:
        return L.gemm_plan(c["a"], c["lda"], W, c["ldw"], c["m"], c["n"], c["k"], c["dt"], NCU, **c["epi"])
    finally:
        L.gemm_variant(prev)


@pytest.mark.parametrize("name,c,want", TABLE, ids=[t[0] for t in TABLE])
def test_mfma_field_and_unchanged_launch(name, c, want):
    if want["kchunk"] is None:
        want = dict(want, kchunk=c["k"])
    on, off = _ask(c, c["variant"]), _ask(c, c["variant"] | L.GEMM_VARIANT_MFMA32)
    for got in (on, off):
        assert {f: getattr(got, f) for f in want} == want
    direct_w4 = want["kernel"] == T256W and want["direct"] == 1
    short_res = want["epi"] in (3, 7, 10, 11) and c["k"] // want["planes"] < 1536
    assert on.mfma == int(direct_w4 and want["epi"] != 12 and not (want["epi"] == 9 and want["ragged"]) and not short_res)
    assert off.mfma == 0


def test_table_reaches_both_answers():
    shapes = {_ask(c, c["variant"]).mfma for _, c, _ in TABLE}
    assert shapes == {0, 1}


def test_variant_bit_round_trips_and_rejects_unknown_values():
    prev = L.gemm_variant(-1)
    try:
        L.gemm_variant(2 | L.GEMM_VARIANT_MFMA32)
        assert L.gemm_variant(-1) == 2 | L.GEMM_VARIANT_MFMA32
        L.gemm_variant(7)                                   # not a main loop of the product library: ignored
        assert L.gemm_variant(-1) == 2 | L.GEMM_VARIANT_MFMA32
    finally:
        L.gemm_variant(prev)
    assert L.gemm_variant(-1) == prev


def test_plain_epilogues_reach_the_four_wave_kernel_from_k256_only():
    """plan_t256 gives the persistent kernels to the plain epilogues (EPI 1 - 3) from K / 32 >= 8: at K = 128 and 192 (two and three
    k-tiles) no row count sends them to gemm_t256w, at K = 256 one round of 256 x 256 tiles does.  This is why tests/test_mfma_shape_gpu.py
    runs those epilogues from K = 256 and the fused ones (which take the four-wave kernel at every K >= 128) from K = 128."""
    for n in (256, 768):
        for kw in (dict(out16=O16), dict(out16=O16, act=L.ACT_GELU), dict(res=RES, out32=O32)):
            for dt in (L.LA_F16, L.LA_BF16):
                for k in (128, 192):
                    assert all(L.gemm_plan(A, k, W, k, 256 * t, n, k, dt, NCU, bias=BIAS, **kw).kernel != T256W for t in range(1, 1025))
                first = next(t for t in range(1, 1025) if L.gemm_plan(A, 256, W, 256, 256 * t, n, 256, dt, NCU, bias=BIAS, **kw).kernel == T256W)
                assert first * (n // 256) >= 2 * NCU > (first - 1) * (n // 256)
    fused = L.gemm_plan(A, 128, W, 128, 512, 256, 128, L.LA_F16, NCU, bias=BIAS, out16=O16, nstat_in=RES, ncol=O32)
    assert fused.kernel == T256W and fused.epi == 8 and fused.mfma == 1
