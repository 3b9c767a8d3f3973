"""GPU: image-order window attention (la_attn_fwd_rows, LA_ATTN_RELPOS_WIN16 with an image grid) skips query blocks that hold padded
queries only.

window_partition (image_encoder.py:258-304) pads the token grid to whole windows.  A padded key takes part in the softmax, a padded query
has no output row: a 128-query block that starts in a window row beyond the image is not computed at all.  What must hold whatever is
skipped: every image token is written, nothing but image tokens is written, every column-sum slot is defined (all-padding blocks: exactly
0.0) and the slots fold to the token means of the stored rows.
"""
import pytest
import torch
from tests.helpers import L

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _all_padding_blocks(nimg, ih, iw, gg):
    """[windows, query blocks] bool: no query of the block lies inside the image (queries run row-major over the gg x gg window)."""
    t = gg * gg
    nq = (t + 127) // 128
    nwy, nwx = -(-ih // gg), -(-iw // gg)
    q = torch.arange(nq * 128)
    ty, tx = (q // gg)[None, None], (q % gg)[None, None]
    wy, wx = torch.arange(nwy)[:, None, None], torch.arange(nwx)[None, :, None]
    inside = (q < t)[None, None] & (wy * gg + ty < ih) & (wx * gg + tx < iw)                       # [wy, wx, q]
    empty = ~inside.view(nwy, nwx, nq, 128).any(-1)
    return empty.view(1, nwy * nwx, nq).expand(nimg, -1, -1).reshape(nimg * nwy * nwx, nq)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom", [(2, 64, 64, 14, 12), (1, 20, 27, 8, 2), (5, 33, 50, 14, 6), (2, 28, 42, 14, 4)])
def test_window_attention_skips_all_padding_query_blocks(L, dt, geom):
    nimg, ih, iw, gg, heads = geom
    hd = 64
    e = heads * hd
    t = gg * gg
    nwy, nwx = -(-ih // gg), -(-iw // gg)
    b = nimg * nwy * nwx
    nq = (t + 127) // 128
    tpad = (16 * gg + 63) // 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(ih * 100 + iw + 7)
    qkv = (torch.randn(nimg * ih * iw, 3 * e, device="cuda", generator=gen) * 0.8).to(dt)
    padrow = (torch.randn(3 * e, device="cuda", generator=gen) * 0.5).to(dt)
    tabh = (torch.randn(2 * gg - 1, hd, device="cuda", generator=gen) * 0.3).to(dt)
    tabw = (torch.randn(2 * gg - 1, hd, device="cuda", generator=gen) * 0.3).to(dt)
    # the output with a guard band of rows in front of and behind the image tokens: the sentinel survives nowhere inside, everywhere outside
    guard = 256
    sentinel = -768.0      # (exact in both 16-bit types)
    buf = torch.full((guard + nimg * ih * iw + guard, e), sentinel, dtype=dt, device="cuda")
    out = buf[guard:guard + nimg * ih * iw]
    part = torch.full((b * nq * e,), float("nan"), device="cuda")
    L.attn_fwd_rows(qkv, out, b, heads, t, tpad, gg, e, 0.125, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw, cspart=part, img_hw=(ih, iw),
                    padrow=padrow)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    # (a softmax-weighted mean of v rows with sigma 0.8 cannot come near the sentinel's magnitude)
    assert bool((out != sentinel).all()) and bool((out.float().abs() < 100.0).all())
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + nimg * ih * iw:] == sentinel).all())
    assert bool(torch.isfinite(part).all())
    empty = _all_padding_blocks(nimg, ih, iw, gg).cuda()
    slots = part.view(b, nq, e)
    assert bool((slots[empty] == 0.0).all())
    if ih % gg == 0 and iw % gg == 0:
        assert not bool(empty.any())
    bar = torch.empty(nimg, e, device="cuda")
    L.colsum_fold(part, nimg, nwy * nwx * nq, e, 1.0 / (ih * iw), bar)
    torch.cuda.synchronize()
    want = out.double().view(nimg, ih * iw, e).mean(1)
    assert float((bar.double() - want).abs().max()) <= 3e-6 * max(1.0, float(want.abs().max()))
    # the same rows without column sums asked for
    out2 = torch.full_like(out, float("nan"))
    L.attn_fwd_rows(qkv, out2, b, heads, t, tpad, gg, e, 0.125, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw, img_hw=(ih, iw), padrow=padrow)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
