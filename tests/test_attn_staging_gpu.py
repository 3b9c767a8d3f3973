"""GPU: la_attn_fwd_rows on the smallest shapes where the K / V tile staging of attn_fwd_kernel's key loop can go wrong.

A wave requests the next tile's LDS-DMA pieces from inside the current tile's softmax, every wave reads pieces that other waves
requested, and the wait + barrier at the bottom of the tile is all that orders the two.  The shapes: one tile (nothing to request), two
tiles, a ragged last tile with an idle fourth wave in the second query block (it only stages, and must still arrive at every barrier),
64 tiles with the rel-pos table refill at tile 32, 14 x 14 windows in image order with edge windows (half last tile), and 128-wide heads
(eight pieces per wave).  A missing wait or barrier shows as stale LDS - a wrong or a changing result, not a fault - so every case is
held to the fp64 reference (tests/softmax_profiles.py, TOL16, per row as check_rows of tests/test_attention_conditioning_gpu.py) and
runs the launch twice on the same inputs: the two outputs must be bit-equal.

Inputs are N(0, 1) in q, k and v (score spread ~1 nat at either head width): every tile carries a comparable share of every row's mass,
so a tile read from the wrong stage moves the output by ~1 / tiles >= 1.5e-2 of its size, far above the bounds."""
import functools
import math

import pytest
import torch

from tests import softmax_profiles as SP
from tests.helpers import L, NAN

pytestmark = pytest.mark.gpu


def check_rows(tag, got, ref_rows, heads, tol):
    """max-norm relative to the output's maximum, and every (row, head) relative to its own maximum (4 x)."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    err = (got - ref_rows).abs()
    e_all = float(err.max() / ref_rows.abs().max())
    rows = ref_rows.shape[0]
    e_row = float((err.view(rows, heads, -1).amax(-1) / ref_rows.abs().view(rows, heads, -1).amax(-1)).max())
    print(f"[staging] {tag}: out {e_all:.2e} (bound {tol:.1e})  worst row {e_row:.2e} (bound {4 * tol:.1e})")
    assert e_all <= tol, (tag, e_all)
    assert e_row <= 4 * tol, (tag, e_row)


@functools.lru_cache(maxsize=None)
def random_case(t, hd, dt, b, heads, g):
    """-> (q | k | v rows in the operand type on the device, fp64 reference rows, tables or None); built once per shape"""
    gen = torch.Generator().manual_seed(100 * t + hd + g)
    q, k, v = (SP.round_to(torch.randn(b, heads, t, hd, generator=gen, dtype=torch.float64), dt).cuda() for _ in range(3))
    tabh = tabw = None
    if g:
        tabh, tabw = (SP.round_to(0.3 * torch.randn(2 * g - 1, hd, generator=gen, dtype=torch.float64), dt).cuda() for _ in range(2))
    o, _ = SP.attention(q, k, v, 1.0 / math.sqrt(hd), g, tabh, tabw)
    qkv = SP.pack_qkv({"q": q, "k": k, "v": v}, SP.TORCH_DT[dt], "cuda")
    return qkv, SP.rows_of(o), tabh, tabw


def run_twice(tag, launch, shape, dtype):
    """the same launch into two NaN-filled outputs: bit-equal, and the first one is returned"""
    outs = []
    for _ in range(2):
        out = torch.full(shape, NAN, dtype=dtype, device="cuda")
        launch(out)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{tag}: two launches on the same inputs differ"
    return outs[0]


PLAIN = [(64, 64, "f16", 2, 2),        # one tile: nothing to request
         (128, 64, "f16", 2, 2),       # two tiles
         (200, 64, "f16", 2, 2),       # ragged last tile (Tpad 256), the second query block's fourth wave is idle
         (200, 64, "bf16", 2, 2),
         (200, 128, "f16", 2, 2)]      # 128-wide heads: eight pieces per wave, ragged + idle wave


@pytest.mark.parametrize("t,hd,dt,b,heads", PLAIN, ids=lambda x: str(x))
def test_plain_rows_small_tile_counts(L, t, hd, dt, b, heads):
    qkv, ref, _, _ = random_case(t, hd, dt, b, heads, 0)
    dtype, e, tpad, sc = SP.TORCH_DT[dt], heads * hd, (t + 63) // 64 * 64, 1.0 / math.sqrt(hd)
    tag = f"plain T{t} hd{hd} {dt}"
    out = run_twice(tag, lambda o: L.attn_fwd_rows(qkv, o, b, heads, t, tpad, 0, e, sc, L.ATTN_PLAIN), (b * t, e), dtype)
    check_rows(tag, out, ref, heads, SP.TOL16[dt])


def test_global_relpos_rows_64_tiles_with_table_refill(L):
    """G = 64, T = 4096, one image, two heads: 64 tiles, the second half of the row terms is rebuilt in LDS beside the stages at tile 32"""
    t, g, hd, dt, b, heads = 4096, 64, 64, "f16", 1, 2
    qkv, ref, tabh, tabw = random_case(t, hd, dt, b, heads, g)
    dtype, e, sc = SP.TORCH_DT[dt], heads * hd, 1.0 / math.sqrt(hd)
    launch = lambda o: L.attn_fwd_rows(qkv, o, b, heads, t, t, g, e, sc, L.ATTN_RELPOS, tabh=tabh.to(dtype), tabw=tabw.to(dtype))
    out = run_twice("global G64", launch, (b * t, e), dtype)
    check_rows("global G64 T4096 la_attn_fwd_rows", out, ref, heads, SP.TOL16[dt])


@functools.lru_cache(maxsize=None)
def image_windows():
    return SP.build_image_windows("f16", ih=64, iw=64)


def test_windows_image_order_64x64_grid_with_edge_windows(L):
    """14 x 14 windows on a 64 x 64 token grid in image order: 5 x 5 windows, the right and bottom ones reach beyond the image (pad row
    keys), every window's last key tile runs its lower half only."""
    iw = image_windows()
    win = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in iw["win"].items()}
    g, ih, iwid, sc = iw["g"], iw["ih"], iw["iw"], iw["scale"]
    nwin, heads, t, hd = win["q"].shape
    assert (g, ih, iwid, nwin) == (14, 64, 64, 25) and int((iw["rows"] < 0).sum()) > 0
    dt = "f16"
    dtype, e = SP.TORCH_DT[dt], heads * hd
    o, _ = SP.attention(win["q"], win["k"], win["v"], sc, g, win["tabh"], win["tabw"])
    ref_w = SP.rows_of(o)
    q, k, v = iw["img"]
    qkv = SP.pack_qkv({"q": q, "k": k, "v": v}, dtype, "cuda")
    padrow = torch.cat([z.reshape(-1) for z in iw["pad"]]).to(dtype).cuda().contiguous()
    tpad = (16 * g + 63) // 64 * 64
    tabh, tabw = win["tabh"].to(dtype), win["tabw"].to(dtype)
    launch = lambda o_: L.attn_fwd_rows(qkv, o_, nwin, heads, t, tpad, g, e, sc, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw, img_hw=(ih, iwid), padrow=padrow)
    out = run_twice("win16 image order", launch, (ih * iwid, e), dtype)
    rows = iw["rows"].reshape(-1).cuda()
    ins = rows >= 0
    check_rows("win16 image order 64x64 G14 la_attn_fwd_rows", out[rows[ins]], ref_w[ins], heads, SP.TOL16[dt])
