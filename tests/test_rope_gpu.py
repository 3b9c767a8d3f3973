"""GPU: la_rope_qk, the rotary embedding of the DINOv3 ViT's q and k, against fp64.

The smallest shapes at which it can go wrong: 2 images of t = 14 rows (prefix 5 + a 3 x 3 grid: rows are no multiple of anything, the
second image's prefix sits in the middle of the buffer), 2 heads, head widths 64 and 32 padded to 64, a row stride wider than 3 ea; the
64-wide case spans two workgroups.  The buffer is filled everywhere - prefix rows, padded columns, the v block, the columns beyond 3 ea -
so that a rotation of anything but the real q and k columns of the patch rows shows as a changed bit.

Bound, per element: half a unit in the last place of the EXACT value in the storage type (one rounding after fp32 arithmetic) plus 1e-6 of
the row's largest input magnitude (two fp32 products and their sum: <= 3 x 2^-24 (|x1| + |x2|) < 4e-7 of it; the fp64 reference reads the
same fp32 tables, so they add nothing).
"""
import math

import pytest
import torch

from labelanything_amd.engine import rope_table
from tests.helpers import L, check_guards, guarded  # noqa: F401  (L: fixture)

pytestmark = pytest.mark.gpu

IMAGES, PREFIX, G, HEADS, PAD_COLS = 2, 5, 3, 2, 8
T = PREFIX + G * G
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}


def half_ulp(exact: torch.Tensor, dtype) -> torch.Tensor:
    """Half the spacing of ``dtype`` at the fp64 values ``exact`` (subnormal spacing below the smallest normal)."""
    e = torch.floor(torch.log2(exact.abs().clamp_min(1e-300))).clamp_min(MIN_EXP[dtype])
    return torch.pow(2.0, e - MANT[dtype] - 1)


def make(hd, hdp, dtype, seed):
    ea = HEADS * hdp
    ld = 3 * ea + PAD_COLS
    g = torch.Generator().manual_seed(seed)
    src = (torch.randn(IMAGES * T, ld, generator=g) * 3.0).to(dtype)
    cos, sin = rope_table(G, hd, 100.0)
    return src, cos, sin, ea, ld


def reference(src, cos, sin, hd, hdp, ea):
    """fp64: x cos + (-x2 | x1) sin on the real columns of q and k of the patch rows; (exact values, mask of the rotated elements)."""
    x = src.double()
    out = x.clone()
    mask = torch.zeros_like(src, dtype=torch.bool)
    c, s = cos.double(), sin.double()
    for img in range(IMAGES):
        r0 = img * T + PREFIX
        for blk in range(2):
            for h in range(HEADS):
                c0 = blk * ea + h * hdp
                v = x[r0:r0 + G * G, c0:c0 + hd]
                rot = torch.cat([-v[:, hd // 2:], v[:, :hd // 2]], dim=1)
                out[r0:r0 + G * G, c0:c0 + hd] = v * c + rot * s
                mask[r0:r0 + G * G, c0:c0 + hd] = True
    return out, mask


def bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hd,hdp", [(64, 64), (32, 64)], ids=["hd64", "hd32pad64"])
def test_rope_qk_against_fp64_and_leaves_everything_else_bit_identical(L, hd, hdp, dtype):
    src, cos, sin, ea, ld = make(hd, hdp, dtype, seed=7 + hd)
    exact, mask = reference(src, cos, sin, hd, hdp, ea)
    buf, qkv = guarded(IMAGES * T, ld, dtype=dtype)
    qkv.copy_(src)
    L.rope_qk(qkv, T, PREFIX, HEADS, hd, hdp, cos.cuda(), sin.cuda())
    check_guards(buf, qkv)
    got = qkv.cpu()
    # prefix rows, the padded columns of every head, the v block and the columns beyond 3 ea: the same bits
    assert torch.equal(bits(got)[~mask], bits(src)[~mask])
    assert int(mask.sum()) == IMAGES * G * G * 2 * HEADS * hd
    assert not torch.equal(bits(got)[mask], bits(src)[mask])
    rowmax = src.double().abs().amax(dim=1, keepdim=True)
    err = (got.double() - exact).abs()
    bound = half_ulp(exact, dtype) + 1e-6 * rowmax
    worst = float((err / bound)[mask].max())
    print(f"[rope {hd}/{hdp} {dtype}] worst error {float(err[mask].max()):.3e}, {worst:.3f} of the bound")
    assert bool((err <= bound)[mask].all())


def test_rope_qk_graph_replay_is_bit_identical(L):
    hd, hdp, dtype = 64, 64, torch.float16
    src, cos, sin, ea, ld = make(hd, hdp, dtype, seed=3)
    src, cos, sin = src.cuda(), cos.cuda(), sin.cuda()
    eager = src.clone()
    L.rope_qk(eager, T, PREFIX, HEADS, hd, hdp, cos, sin)
    work = torch.empty_like(src)

    def launch():
        work.copy_(src)
        L.rope_qk(work, T, PREFIX, HEADS, hd, hdp, cos, sin)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()                                                  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    work.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(work), bits(eager))


def test_rope_qk_refuses_what_it_cannot_vectorise(L):
    qkv = torch.zeros(T, 3 * 2 * 64, dtype=torch.float16, device="cuda")
    cos, sin = (t.cuda() for t in rope_table(G, 24, 100.0))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        L.rope_qk(qkv, T, PREFIX, 2, 24, 64, cos, sin)
    cos, sin = (t.cuda() for t in rope_table(G, 64, 100.0))
    with pytest.raises(RuntimeError, match="whole images"):
        L.rope_qk(qkv[:T - 1], T, PREFIX, 2, 64, 64, cos, sin)
    with pytest.raises(ValueError, match="columns"):
        L.rope_qk(qkv[:, :128], T, PREFIX, 2, 64, 64, cos, sin)
    assert float(qkv.abs().max()) == 0.0
    assert math.isqrt(T - PREFIX) == G
