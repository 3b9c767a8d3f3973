"""GPU: la_im2col_patch_pad, the patch gather for patch sides that are no multiple of 8 (DINOv2's 14), against
``torch.nn.functional.unfold`` on the CPU - bit for bit.

The kernel copies and rounds, it does no arithmetic: fp32 outputs are copies, fp16 / bf16 the round-to-nearest-even of the fp32 value
(what ``Tensor.to`` gives on the CPU), and the LA_F16X2 planes are ``store4_split``'s hi = rn16(v), lo = rn16(v - float(hi)) with the
subtraction in fp32 - the derivation is itself compared with la_im2col_patch's split form on the same image.  The columns K .. Kp are exact
zeros although the buffer is handed over full of NaN; the guard elements on either side keep their bits.

Geometries (two images each): (14, 28) and (14, 42): g = 2 and 3, K = 588 -> Kp = 640, chunks that straddle a patch row (14 > 8) and a
channel (196 % 8 == 4), a last data chunk that is half padding, 6 workgroups at g = 3; (10, 30): K = 300 -> 320, 100 % 8 == 4;
(6, 24): K = 108 -> Kp = 128, the minimum.  Kp = 704 for p = 14: a whole chunk row of slack.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import L, check_guards, guarded  # noqa: F401  (L: fixture)

pytestmark = pytest.mark.gpu

IMAGES = 2
GEOMETRIES = [(14, 28, 640), (14, 42, 640), (10, 30, 320), (6, 24, 128), (14, 28, 704)]
FORMS = ["f32", "f16", "bf16", "f16x2"]
DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f16x2": torch.float16}


def images(p, s):
    g = torch.Generator().manual_seed(100 * p + s)
    return torch.randn(IMAGES, 3, s, s, generator=g) * 3.0


def unfolded(img, p, kp):
    """[Bn g g, kp] fp32 on the CPU: column k = c p p + ky p + kx, zeros from K on."""
    cols = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p)
    return F.pad(cols, (0, kp - cols.shape[1]))


def expected(vals, form):
    """The storage form of the fp32 values: a copy, one rounding, or store4_split's [hi | lo] planes."""
    if form != "f16x2":
        return vals.to(DTYPE[form])
    hi = vals.to(torch.float16)
    lo = (vals - hi.float()).to(torch.float16)
    return torch.cat([hi, lo], dim=1)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("p,s,kp", GEOMETRIES, ids=[f"p{p}s{s}kp{kp}" for p, s, kp in GEOMETRIES])
def test_gather_is_bit_exact_and_pads_with_zeros(L, p, s, kp, form):
    img = images(p, s)
    k, rows, split = 3 * p * p, IMAGES * (s // p) ** 2, form == "f16x2"
    want = expected(unfolded(img, p, kp), form)
    buf, out = guarded(rows, 2 * kp if split else kp, dtype=DTYPE[form])          # NaN everywhere
    L.im2col_patch_pad(img.cuda(), p, kp, out, split=split)
    check_guards(buf, out)
    got = out.cpu()
    assert torch.equal(bits(got), bits(want))
    for plane in range(2 if split else 1):
        pad = got[:, plane * kp + k:(plane + 1) * kp]
        assert pad.numel() == rows * (kp - k) and bool((bits(pad) == 0).all())             # +0.0, not merely == 0
    assert bool((got[:, :k] != 0).any(dim=0).all())          # every data column carries data


def test_split_derivation_is_the_old_gather_s_split_form(L):
    """la_im2col_patch (patch 8) on the 24 px images: its [hi | lo] planes are ``expected(..., "f16x2")`` of the same values."""
    img = images(6, 24)
    vals = unfolded(img, 8, 192)
    out = torch.empty(vals.shape[0], 384, dtype=torch.float16, device="cuda")
    L.im2col_patch(img.cuda(), 8, out, split=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(expected(vals, "f16x2")))
    assert bool((out[:, 192:] != 0).any())                   # the lo plane is not trivially zero


def test_refusals_come_before_the_library(L):
    img = images(14, 28).cuda()
    out = torch.full((8, 640), float("nan"), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="even"):
        L.im2col_patch_pad(images(7, 28).cuda(), 7, 192, torch.empty(32, 192, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="multiple of 64"):
        L.im2col_patch_pad(img, 14, 600, torch.empty(8, 600, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match=">= 3 patch"):
        L.im2col_patch_pad(img, 14, 576, torch.empty(8, 576, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match=">= 128"):
        L.im2col_patch_pad(images(4, 8).cuda(), 4, 64, torch.empty(8, 64, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="divide"):
        L.im2col_patch_pad(images(14, 30).cuda(), 14, 640, out)
    with pytest.raises(ValueError, match="out must be"):
        L.im2col_patch_pad(img, 14, 640, out.to(torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        L.im2col_patch_pad(img, 14, 640, out[:7])
    with pytest.raises(ValueError, match="out must be"):
        L.im2col_patch_pad(img, 14, 640, out, split=True)                 # plane pairs need 2 kp columns
    with pytest.raises(ValueError, match="out must be"):
        L.im2col_patch_pad(img, 14, 640, torch.empty(8, 1280, dtype=torch.float16, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="fp16 plane pairs"):
        L.im2col_patch_pad(img, 14, 640, torch.empty(8, 1280, dtype=torch.bfloat16, device="cuda"), split=True)
    with pytest.raises(ValueError, match="img must be"):
        L.im2col_patch_pad(img.double(), 14, 640, out)
    with pytest.raises(RuntimeError, match="device tensors"):
        L.im2col_patch_pad(img.cpu(), 14, 640, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                      # nothing was launched


def test_graph_replay_is_bit_identical(L):
    p, s, kp = 14, 42, 640
    img = images(p, s).cuda()
    rows = IMAGES * (s // p) ** 2
    eager = torch.empty(rows, 2 * kp, dtype=torch.float16, device="cuda")
    L.im2col_patch_pad(img, p, kp, eager, split=True)
    work = torch.empty_like(eager)

    def launch():
        L.im2col_patch_pad(img, p, kp, work, split=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    work.fill_(float("nan"))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(work), bits(eager))
