"""GPU: the two forms of the four-wave GEMM's own epilogue (gemm_w4.hip, epilogue_w4) compute the same thing.

A call whose row count is a multiple of 256 runs the interior form (no row predicates, one scalar base per matrix and tile + 32-bit lane
offsets); a ragged row count runs the predicated form with per-lane 64-bit addresses.  For every fused epilogue that la_gemm reaches on fp16
operands, a ragged M and the same operands zero-extended to the next multiple of 256 must give rows < M that are equal bit for bit in
every output, and the ragged call must not touch memory behind row M.
"""
import math

import pytest
import torch
from tests.helpers import L, rnd

pytestmark = pytest.mark.gpu

SENT = -3.0e4          # (exact in fp16 and fp32; no output of these cases comes near it)


def _ext(x, rows):
    """x zero-extended to ``rows`` rows"""
    out = torch.zeros(rows, *x.shape[1:], dtype=x.dtype, device=x.device)
    out[: x.shape[0]] = x
    return out


def _case(L, name, m, mp, n, k, fill):
    """Buffers of mp rows.  fill: what rows >= m of the outputs / in-place streams hold before the call (the sentinel for the ragged call, zero =
    the zero-extension for the whole-tile call).  Returns (keyword arguments, {output name: tensor})."""
    def buf(cols, dtype, init=None):
        t = torch.full((mp, cols), fill, dtype=dtype, device="cuda")
        if init is not None:
            t[:m] = init
        return t

    bias = rnd(n, seed=3)
    if name == "plain16":
        o = buf(n, torch.float16)
        return dict(bias=bias, out16=o), {"out16": o}
    if name == "gelu16":
        o = buf(n, torch.float16)
        return dict(bias=bias, out16=o, act=L.ACT_GELU), {"out16": o}
    if name == "res32":
        s = buf(n, torch.float32, rnd(m, n, seed=4))
        return dict(bias=bias, res=s, out32=s), {"out32": s}
    if name.startswith("producer32"):
        s = buf(n, torch.float32, rnd(m, n, seed=4))
        o = buf(n, torch.float16)
        part = torch.full((mp, n // 64, 2), fill, device="cuda")
        kw = dict(bias=bias, res=s, out32=s, out16=o, nstat_out=part)
        rpg = {"producer32": 0, "producer32_rvec_tiles": 512, "producer32_rvec_groups": 901}[name]
        if rpg:
            kw.update(rvec=_ext(rnd(-(-m // rpg), n, seed=5, scale=0.3), -(-mp // rpg)), rvec_rpg=rpg)
        return kw, {"out32": s, "out16": o, "nstat_out": part}
    if name.startswith("planes"):
        x0 = rnd(m, n, seed=6) * 3.0
        xs = buf(2 * n, torch.float16, torch.cat([x0.half(), (x0 - x0.half().float()).half()], dim=1))
        part = torch.full((mp, n // 64, 2), fill, device="cuda")
        kw = dict(bias=bias, out16=xs[:, :n], aux16=xs[:, n:], nstat_out=part)
        rpg = {"planes": 0, "planes_rvec_tiles": 512, "planes_rvec_groups": 901}[name]
        if rpg:
            kw.update(rvec=_ext(rnd(-(-m // rpg), n, seed=5, scale=0.3), -(-mp // rpg)), rvec_rpg=rpg)
        return kw, {"out16": xs[:, :n], "aux16": xs[:, n:], "nstat_out": part}
    if name.startswith("consumer"):
        mr = torch.zeros(mp, 2, device="cuda")
        mr[:m, 0] = rnd(m, seed=7, scale=0.2)
        mr[:m, 1] = 0.5 + rnd(m, seed=8).abs()
        o = buf(n, torch.float16)
        kw = dict(bias=bias, out16=o, nstat_in=mr, ncol=rnd(n, seed=9))
        if name == "consumer_gelu":
            kw["act"] = L.ACT_GELU
        return kw, {"out16": o}
    raise KeyError(name)


CASES = ["plain16", "gelu16", "res32", "producer32", "producer32_rvec_tiles", "producer32_rvec_groups", "planes", "planes_rvec_tiles",
         "planes_rvec_groups", "consumer", "consumer_gelu"]


@pytest.mark.parametrize("m", [57664, 3 * 256 + 37])
@pytest.mark.parametrize("name", CASES)
def test_interior_and_ragged_epilogue_agree_bit_for_bit(L, name, m):
    n, k = 768, 256
    mp = -(-m // 256) * 256
    a = _ext(rnd(m, k, seed=1).half(), mp)
    w = (rnd(n, k, seed=2) / math.sqrt(k)).half()
    kw_r, out_r = _case(L, name, m, mp, n, k, SENT)
    L.gemm(a, w, M=m, **kw_r)
    kw_w, out_w = _case(L, name, m, mp, n, k, 0.0)
    L.gemm(a, w, **kw_w)
    torch.cuda.synchronize()
    for key in out_r:
        r, wh = out_r[key], out_w[key]
        assert bool(torch.isfinite(r[:m].float()).all()), key
        assert torch.equal(r[:m], wh[:m]), key
        assert bool((r[m:] == SENT).all()), key          # nothing written behind row M


def test_epilogue_reaches_rows_beyond_four_gigabytes(L):
    """The interior form keeps the tile's base as a 64-bit scalar and only the lane's offset inside the wave's 128 rows in 32 bits: an output
    whose rows lie more than 2^32 bytes apart from the first (leading dimension 2^21 halves = 4 MiB per row, 1280 rows = 5 GiB) comes out
    like the compact one.  Skipped where the device has less than 12 GiB free."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("needs 5 GiB for one strided output")
    m, n, k, ld = 1280, 256, 256, 1 << 21
    a = rnd(m, k, seed=11).half()
    w = (rnd(n, k, seed=12) / math.sqrt(k)).half()
    bias = rnd(n, seed=13)
    mr = torch.zeros(m, 2, device="cuda")
    mr[:, 0], mr[:, 1] = rnd(m, seed=14, scale=0.2), 0.5 + rnd(m, seed=15).abs()
    ncol = rnd(n, seed=16)
    ref = torch.empty(m, n, dtype=torch.float16, device="cuda")
    L.gemm(a, w, bias=bias, out16=ref, nstat_in=mr, ncol=ncol)
    big = torch.empty(m * ld, dtype=torch.float16, device="cuda")
    out = big.view(m, ld)[:, :n]
    L.gemm(a, w, bias=bias, out16=out, nstat_in=mr, ncol=ncol)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
