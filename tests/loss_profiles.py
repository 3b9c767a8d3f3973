"""Ill-conditioned inputs of the loss kernels and of the AdamW step, their fp64 references per component, fp32 restatements of each
kernel's arithmetic and the error measures, for tests/test_loss_profiles_cpu.py and tests/test_loss_conditioning_gpu.py.  No kernel code.

la_focal_loss (csrc/loss.hip), la_logits_objective and la_prompt_contrastive (csrc/loss_components.hip) were tested on ``randn * 4``
logits under ONE global bound on the composite gradient.  That leaves the small components (dice, false positive, the negative pairs of
the contrastive term) unchecked, and says nothing about logits with a common offset, confident or confidently wrong pixels, ties or a
gamma other than 2.  The builders below make fp32 inputs with stated properties; ``check_profile`` / ``check_pattern`` /
``check_emb_profile`` measure those properties in fp64 and raise when one is missing.  fp64 references: tests/loss_components_ref.py.

Logit profiles, [B, C, H, W] (built FOR a target: two of them are defined by it):
    random        randn * 4, the baseline
    confident     the target class leads every other class by >= 30 on >= 90 % of the valid pixels (15 of every 16; the rest stay random)
    wrong         the target class trails the best other class by >= 30 on the same pixels: ce ~ 30
    ties          even pixels: all classes equal; odd pixels: two classes tie at the maximum; multiples of 1 / 4 throughout
    offset_K      K in {64, 1024, 8192}: random rounded to the 2^-10 grid inside +-8, plus K: (x + K) - K == x bit for bit, so the fp64
                  answer is that of K = 0
    padded        the last min(3, H // 2) rows hold -inf on the classes >= 1 and 0 on class 0, and their targets are ignored
Target patterns, [B, H, W] (``base`` is the baseline the gamma sweep and the edge shapes use):
    base                    randint with 10 % ignored pixels
    no_ignore               no ignored pixel at all
    class_in_one_image      class C - 1 occurs in image 0 and not in image 1 (batch-wide class weight, per-image fp "absent")
    no_class0_with_ignore   class 0 absent from image 0 while it has ignored pixels (fp: ignored targets read as class 0)
    image_ignored           image 1 fully ignored, image 0 not
    single_pixel_class      class C - 1 has exactly one pixel in the whole batch
    one_class_image         image 1 holds class 1 only and no ignored pixel: A_b = C - 1
    all_classes             every class occurs in every image: A_b = 0, the fp value and gradient are 0
Embedding profiles, [b, m, c, d] with t', bias (every one carries a row below F.normalize's eps, an exact zero row and a row with
norm 1.5e-12, all flagged, in image 0):
    default       randn rows, t' = log 10, bias = -10
    balanced      randn rows, t' = 0, bias = 0: the positive- and negative-pair parts of d emb are within 10x of each other
    saturated     rows +-g + 0.05 noise, t' = log 30, bias = -7: |z| up to 37, u = -y z beyond +-20 on both sides
Flag patterns: all_on, no_flag_image (image 1 has none), single_flag_image (image 1 has one), most_on (85 %).

Error measures (``image_ratio``, ``row_ratio``, ``adamw_ratio``) and tolerances: the fp32 restatements below are measured against
fp64 under the same measure - never against a kernel - which gives one constant per (component, profile) and, for the logits, per
shape; a kernel is held to MARGIN = 4 times that constant, for every profile alike (the kernels sum pixels per 256-thread tile and per
wave butterfly where the restatement uses torch's sums: another reduction error of the same order).  A constant is never taken below
u = 2^-24, the rounding of the fp32 result itself.  ``image_ratio`` with the whole batch as one image is held beside the per-image
measure: on the four-pixel images of (2049, 2, 2, 2) it is the one that still says something (``logits_constants``).
"""
from __future__ import annotations

import functools
import math

import torch

from tests import loss_components_ref as R

U = 2.0 ** -24
MARGIN = 4.0
IGNORE = R.IGNORE
F32 = torch.float32

LOGIT_PROFILES = ("random", "confident", "wrong", "ties", "offset_64", "offset_1024", "offset_8192", "padded")
TARGET_PATTERNS = ("base", "no_ignore", "class_in_one_image", "no_class0_with_ignore", "image_ignored", "single_pixel_class",
                   "one_class_image", "all_classes")
# the smallest shapes that reach every launch form of lo_layout and of the vector switch (tests/test_loss_conditioning_gpu.py)
MAIN_SHAPES = ((2, 5, 32, 36), (2, 6, 33, 35))
EDGE_SHAPES = ((1, 2, 8, 8), (3, 64, 24, 44), (2049, 2, 2, 2))
GAMMAS = (0.0, 1.0, 1.5, 2.0, 5.0)
WEIGHTS = {"focal": 0.75, "dice": 1.5, "fp": 2.0}               # they enter squared; all three squares are fp32 numbers
MASK_NAME = {1: "focal", 2: "dice", 4: "fp", 3: "focal+dice", 5: "focal+fp", 6: "dice+fp", 7: "focal+dice+fp"}
MASK_PARTS = {m: tuple(k for k, bit in (("focal", 1), ("dice", 2), ("fp", 4)) if m & bit) for m in MASK_NAME}

EMB_PROFILES = {"default": (math.log(10.0), -10.0), "balanced": (0.0, 0.0), "saturated": (math.log(30.0), -7.0)}
FLAG_PATTERNS = ("all_on", "no_flag_image", "single_flag_image", "most_on")
EMB_SHAPES = ((3, 7, 48), (5, 61, 64), (2, 8, 1000))            # n = 21: no multiple of 4; n = 305: past a 256 stride; D: 4th slice + tail
EMB_BATCH = 2
SPECIAL_ROWS = {"below_eps": 1, "zero": 3, "above_eps": 6}      # flat row m * c of image 0 (n >= 16 at every shape)

ADAMW_N = (1, 255, 257, 4096 * 256 + 3)
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def _seed(*parts) -> torch.Generator:
    h = 0
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(h)


def pad_rows(h: int) -> int:
    return min(3, h // 2)


# ---- targets -----------------------------------------------------------------------------------------------------------------------
def build_target(pattern: str, shape, seed: int = 0) -> torch.Tensor:
    b, c, h, w = shape
    g = _seed("target", pattern, shape, seed)
    t = torch.randint(0, c, (b, h, w), generator=g)
    ign = torch.rand(b, h, w, generator=g) < 0.1
    if pattern != "no_ignore":
        t[ign] = IGNORE
    flat = t.view(b, -1)
    if pattern in ("base", "no_ignore"):
        pass
    elif pattern == "class_in_one_image":
        flat[1][flat[1] == c - 1] = 0
        flat[0, 0] = c - 1
    elif pattern == "no_class0_with_ignore":
        flat[0][flat[0] == 0] = 1
        flat[0, 1] = IGNORE
    elif pattern == "image_ignored":
        flat[1] = IGNORE
        flat[0, 0] = 0
    elif pattern == "single_pixel_class":
        flat[flat == c - 1] = 0
        flat[0, w + 2] = c - 1
    elif pattern == "one_class_image":
        flat[1] = 1
    elif pattern == "all_classes":
        flat[:, :c] = torch.arange(c)
    else:
        raise ValueError(pattern)
    return t


def check_pattern(pattern: str, t: torch.Tensor, c: int) -> dict:
    b = t.shape[0]
    flat = t.reshape(b, -1)
    cnt = torch.stack([(flat == k).sum(1) for k in range(c)], 1)        # [b, c]
    ign = (flat == IGNORE).sum(1)
    assert bool(((flat == IGNORE) | ((flat >= 0) & (flat < c))).all())
    tz = torch.where(flat == IGNORE, torch.zeros_like(flat), flat)
    absent = torch.stack([((tz == k).sum(1) == 0) for k in range(c)], 1).sum(1)
    fig = {"ignored": ign.tolist() if b <= 4 else int(ign.sum()), "absent": absent.tolist() if b <= 4 else int(absent.max())}
    if pattern == "base":
        assert int(ign.sum()) > 0 or flat.numel() < 64
    elif pattern == "no_ignore":
        assert int(ign.sum()) == 0, "no_ignore: an ignored pixel"
    elif pattern == "class_in_one_image":
        assert int(cnt[0, c - 1]) > 0 and int(cnt[1, c - 1]) == 0, "class_in_one_image: class C - 1 not in image 0 only"
    elif pattern == "no_class0_with_ignore":
        assert int(cnt[0, 0]) == 0 and int(ign[0]) > 0, "no_class0_with_ignore: class 0 present or nothing ignored"
    elif pattern == "image_ignored":
        assert int(ign[1]) == flat.shape[1] and int(ign[0]) < flat.shape[1], "image_ignored: image 1 not fully ignored, or image 0 is"
    elif pattern == "single_pixel_class":
        assert int(cnt[:, c - 1].sum()) == 1, "single_pixel_class: class C - 1 has not exactly one pixel"
    elif pattern == "one_class_image":
        assert int((cnt[1] > 0).sum()) == 1 and int(ign[1]) == 0 and int(absent[1]) == c - 1, "one_class_image: A_b != C - 1"
    elif pattern == "all_classes":
        assert bool((cnt > 0).all()) and int(absent.max()) == 0, "all_classes: a class is missing from an image"
    else:
        raise ValueError(pattern)
    return fig


# ---- logits ------------------------------------------------------------------------------------------------------------------------
def _grid(x: torch.Tensor, bound: float) -> torch.Tensor:
    return (torch.round(x.double() * 1024.0) / 1024.0).clamp(-bound, bound)


def _chosen(t: torch.Tensor) -> torch.Tensor:
    """15 of every 16 pixels (by flat index), valid ones only: where confident / wrong apply"""
    idx = torch.arange(t[0].numel()).view(t.shape[1:])
    return ((idx % 16) != 0)[None] & (t != IGNORE)


def build_logits(profile: str, shape, target: torch.Tensor, seed: int = 0):
    """-> (fp32 logits [B, C, H, W], the target to use with them: ``padded`` ignores its rows)"""
    b, c, h, w = shape
    g = _seed("logits", profile, shape, seed)
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64) * 4
    t = target.clone()
    if profile == "random":
        pass
    elif profile in ("confident", "wrong"):
        x = _grid(x, 16.0)
        tt = torch.where(t == IGNORE, torch.zeros_like(t), t)
        oh = torch.zeros(b, c, h, w, dtype=torch.bool).scatter_(1, tt[:, None], True)
        other = x.masked_fill(oh, -math.inf).amax(1)
        val = other + (30.0 if profile == "confident" else -30.0)
        x = torch.where(oh & _chosen(t)[:, None], val[:, None], x)
    elif profile == "ties":
        idx = torch.arange(h * w).view(1, 1, h, w)
        cls = torch.arange(c).view(1, c, 1, 1)
        level = torch.tensor([0.0, 1.5, -3.25, 12.0], dtype=torch.float64)[(idx // 2) % 4]
        two = (cls == idx % c) | (cls == (idx + 1) % c)
        lower = level - 2.5 - 0.25 * cls
        x = torch.where((idx % 2 == 0) | two, level.expand(1, c, h, w), lower).expand(b, c, h, w).clone()
    elif profile.startswith("offset_"):
        x = _grid(x, 8.0) + float(profile[7:])
    elif profile == "padded":
        n = pad_rows(h)
        x[:, 1:, h - n:, :] = -math.inf
        x[:, 0, h - n:, :] = 0.0
        t[:, h - n:, :] = IGNORE
    else:
        raise ValueError(profile)
    return x.float().contiguous(), t


def check_profile(profile: str, x: torch.Tensor, t: torch.Tensor) -> dict:
    """Measure the stated properties in fp64 on the fp32 values; AssertionError when one is missing.  -> figures."""
    b, c, h, w = x.shape
    assert x.dtype == F32 and not bool(torch.isnan(x).any())
    xd = x.double()
    valid = t != IGNORE
    tt = torch.where(valid, t, torch.zeros_like(t))
    oh = torch.zeros(b, c, h, w, dtype=torch.bool).scatter_(1, tt[:, None], True)
    if profile == "random":
        assert bool(torch.isfinite(x).all())
        return {"max |x|": float(xd.abs().max())}
    if profile in ("confident", "wrong"):
        xt = xd.gather(1, tt[:, None]).squeeze(1)
        other = xd.masked_fill(oh, -math.inf).amax(1)
        lead = (xt - other) if profile == "confident" else (other - xt)
        share = float(((lead >= 30.0) & valid).sum()) / max(1, int(valid.sum()))
        assert share >= 0.9, f"{profile}: the margin of 30 holds on {share:.3f} of the valid pixels only"
        ce = -torch.log_softmax(xd, 1).gather(1, tt[:, None]).squeeze(1)[valid]
        if profile == "wrong":
            assert 30.0 <= float(ce.median()) <= 30.0 + math.log(c) + 1e-9
        else:
            assert float(ce.median()) <= c * math.exp(-30.0)
        return {"share": share, "median ce": float(ce.median())}
    if profile == "ties":
        assert bool((xd * 4 == torch.round(xd * 4)).all()), "ties: values are no multiples of 1 / 4"
        at_max = (xd == xd.amax(1, keepdim=True)).sum(1)
        assert bool((at_max >= 2).all()), "ties: a pixel with a single maximum"
        all_eq = float((at_max == c).float().mean())
        assert all_eq >= 0.4 and (c == 2 or float((at_max == 2).float().mean()) >= 0.4), "ties: all-equal and two-way pixels both needed"
        return {"all equal": all_eq}
    if profile.startswith("offset_"):
        k = float(profile[7:])
        base = x - torch.tensor(k, dtype=F32)                         # fp32 arithmetic
        assert torch.equal(base + torch.tensor(k, dtype=F32), x), "offset: (x + K) - K != x"
        assert torch.equal(base.double(), xd - k) and bool((base.double() * 1024 == torch.round(base.double() * 1024)).all())
        assert float(base.abs().max()) <= 8.0 and float(xd.mean()) >= k - 1.0, "offset: not within +-8 of K"
        assert float(base.double().std()) > 2.0
        return {"K": k, "max |x - K|": float(base.abs().max())}
    if profile == "padded":
        n = pad_rows(h)
        assert n >= 1 and bool((x[:, 1:, h - n:, :] == -math.inf).all()) and bool((x[:, 0, h - n:, :] == 0).all()), "padded: rows not padded"
        assert bool((t[:, h - n:, :] == IGNORE).all()), "padded: the padded rows are not ignored"
        assert bool(torch.isfinite(x[:, :, : h - n, :]).all())
        return {"rows": n}
    raise ValueError(profile)


def patterns_for(profile: str, shape) -> tuple:
    """Target patterns a profile runs with: all of them at the main shapes (``padded`` ignores its rows, so it cannot run with
    no_ignore and one_class_image), the baseline at the edge shapes."""
    if tuple(shape) not in MAIN_SHAPES:
        return ("base",)
    if profile == "padded":
        return tuple(p for p in TARGET_PATTERNS if p not in ("no_ignore", "one_class_image"))
    return TARGET_PATTERNS


def profiles_for(shape) -> tuple:
    return LOGIT_PROFILES if tuple(shape) in MAIN_SHAPES else ("random", "padded")


def runs_for(pattern: str):
    """(mask, gamma, class_weighting) of every launch of one (profile, pattern): each component alone with class weighting on and off,
    the combined masks, and at the baseline pattern every gamma.  gamma in (0, 1) is left out: the derivative is unbounded as pt -> 1."""
    out = [(1, 2.0, True), (1, 2.0, False), (2, 2.0, True), (2, 2.0, False), (4, 2.0, True), (3, 2.0, True), (5, 2.0, True), (6, 2.0, True),
           (7, 2.0, True)]
    if pattern == "base":
        out += [(1, gm, True) for gm in GAMMAS if gm != 2.0]
    return out


@functools.lru_cache(maxsize=None)
def inputs(shape, profile: str, pattern: str):
    """(logits, target) of one case, checked; built once per process and never written to."""
    t = build_target(pattern, shape)
    x, t = build_logits(profile, shape, t)
    if tuple(shape) in MAIN_SHAPES:
        check_pattern(pattern, t, shape[1])
    check_profile(profile, x, t)
    return x, t


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def _grad64(fn, x: torch.Tensor):
    xd = x.double().requires_grad_(True)
    val = fn(xd)
    (g,) = torch.autograd.grad(val, xd)
    return float(val.detach()), g


@functools.lru_cache(maxsize=None)
def _ref_part(shape, profile: str, pattern: str, part: str, gamma: float, cwt: bool):
    x, t = inputs(shape, profile, pattern)
    if part == "fp":
        return _grad64(lambda v: R.false_positive(v, t), x)
    cw = R.class_weights(t, x.shape[1], cwt)
    return _grad64((lambda v: R.focal(v, t, gamma, cw)) if part == "focal" else (lambda v: R.dice(v, t, cw)), x)


def reference(shape, profile: str, pattern: str, mask: int, gamma: float, cwt: bool) -> dict:
    """The weighted fp64 answer of one launch: {"parts": {name: w^2 dL}, "components": [w L] * 3, "value": sum w^2 L}; every part is
    computed once per process and shared."""
    parts, comps, value = {}, [0.0, 0.0, 0.0], 0.0
    for i, name in enumerate(("focal", "dice", "fp")):
        if name in MASK_PARTS[mask]:
            l, g = _ref_part(shape, profile, pattern, name, gamma if name == "focal" else 0.0, cwt if name != "fp" else False)
            w = WEIGHTS[name]
            parts[name], comps[i], value = g * (w * w), w * l, value + w * w * l
    return {"parts": parts, "components": comps, "value": value}


# ---- error measures ----------------------------------------------------------------------------------------------------------------
def image_ratio(g: torch.Tensor, parts) -> float:
    """max over the images of max |g - sum parts| / scale, scale = the smallest non-zero per-image maximum among the parts' own
    gradients; where every part is 0 over an image, g must be 0 there too.  A non-finite g gives inf."""
    parts = list(parts)
    gd = g.detach().double().cpu()
    if not bool(torch.isfinite(gd).all()):
        return math.inf
    b = gd.shape[0]
    err = (gd - sum(parts)).abs().reshape(b, -1).amax(1)
    tops = torch.stack([p.abs().reshape(b, -1).amax(1) for p in parts])
    scale = torch.where(tops > 0, tops, torch.full_like(tops, math.inf)).amin(0)
    dead = torch.isinf(scale)
    if bool((err[dead] != 0).any()):
        return math.inf
    return float((err[~dead] / scale[~dead]).max()) if bool((~dead).any()) else 0.0


def pair_ratio(a: torch.Tensor, b: torch.Tensor, ref: torch.Tensor) -> float:
    """two kernels against each other: max over the images of max |a - b| / max |ref|"""
    n = ref.shape[0]
    err = (a.detach().double().cpu() - b.detach().double().cpu()).abs().reshape(n, -1).amax(1)
    top = ref.abs().reshape(n, -1).amax(1)
    if not bool(torch.isfinite(err).all()) or bool((err[top == 0] != 0).any()):
        return math.inf
    return float((err[top > 0] / top[top > 0]).max()) if bool((top > 0).any()) else 0.0


def rel(got: float, ref: float) -> float:
    if ref == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(got - ref) / abs(ref) if math.isfinite(got) else math.inf


def row_ratio(g: torch.Tensor, ref: torch.Tensor) -> float:
    """max over the rows of max |g_row - ref_row| / max |ref_row|; a row whose reference is 0 must be exactly 0."""
    gd = g.detach().double().cpu().reshape(-1, g.shape[-1])
    rd = ref.reshape(-1, ref.shape[-1])
    if not bool(torch.isfinite(gd).all()):
        return math.inf
    err, top = (gd - rd).abs().amax(1), rd.abs().amax(1)
    dead = top == 0
    if bool((err[dead] != 0).any()):
        return math.inf
    return float((err[~dead] / top[~dead]).max()) if bool((~dead).any()) else 0.0


# ---- fp32 restatement of la_logits_objective / la_focal_loss -------------------------------------------------------------------------
def _f(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=F32)


def logits32(x: torch.Tensor, t: torch.Tensor, mask: int, gamma: float, cwt: bool, *, stable: bool = True, mutate: str = "",
             weights=None) -> dict:
    """lo_hist -> lo_dice_sums -> lo_coef -> lo_fused -> lo_fold in fp32 torch arithmetic (fp64 where the kernels hold fp64), with the
    weights of ``WEIGHTS`` (or ``weights``).  stable: ce = log(se) - (x_t - mx), sm = exp(x - mx) / se; otherwise the lse form of focal_fwd_bwd_kernel
    (ce = (mx + log se) - x_t, sm = exp(x - lse)).  focal_fwd_bwd_kernel itself takes sm as exp((x - mx) - log se): as
    shift-stable, and inside the tolerance this restatement gives (profiles/loss_conditioning.md).  ``mutate`` names one deliberately wrong variant (test_loss_profiles_cpu.py)."""
    b, c, h, w = x.shape
    hw, n = h * w, b * h * w
    x = x.reshape(b, c, hw)
    t = t.reshape(b, hw)
    notign = t != IGNORE
    ok = notign & (t >= 0) & (t < c)
    tc = torch.where(ok, t, torch.zeros_like(t))
    oh = torch.zeros(b, c, hw, dtype=torch.bool).scatter_(1, tc[:, None], ok[:, None])
    cnt = oh.sum(2)
    ign = (~notign).sum(1)
    mx = x.amax(1)
    se = torch.zeros_like(mx)
    for k in range(c):
        se = se + torch.exp(x[:, k] - mx)
    p = torch.exp(x - mx[:, None]) / se[:, None]
    wf, wd, wp = ((weights or WEIGHTS)[k] if k in MASK_PARTS[mask] else 0.0 for k in ("focal", "dice", "fp"))
    # class weights of the batch
    if mutate == "cw_per_image":
        wc = torch.where(cnt > 0, 1.0 / torch.log(_f(1.1) + cnt.float() / _f(float(hw))), _f(1.0))
    else:
        tot = cnt.sum(0)
        wc = torch.where(tot > 0, 1.0 / torch.log(_f(1.1) + tot.float() / _f(float(n))), _f(1.0))[None].expand(b, c)
    if not cwt:
        wc = torch.ones(b, c)
    # focal
    fk = torch.zeros(b, hw)
    sm = p
    lf = 0.0
    if mask & 1:
        xt = x.gather(1, tc[:, None]).squeeze(1)
        if stable:
            ce = torch.log(se) - (xt - mx)
        else:
            lse = mx + torch.log(se)
            ce = lse - xt
            sm = torch.exp(x - lse[:, None])
        pt = torch.exp(-ce)
        om = 1.0 - pt
        pw = torch.pow(om, gamma)
        wt = wc.gather(1, tc)
        lf = float(torch.where(ok, pw * wt * ce, _f(0.0)).double().sum() / n)
        gg = pw + torch.where(om > 0, gamma * ce * pt * torch.pow(om, gamma - 1.0), _f(0.0))
        fk = torch.where(ok, (_f(wf) * _f(wf) / _f(float(n))) * wt * gg, _f(0.0))
    # dice coefficients
    al, be, ld = torch.zeros(b, c), torch.zeros(b, c), 0.0
    if mask & 2:
        sp = (p * notign[:, None] if mutate == "dice_u_no_ignored" else p).double().sum(2)
        si = (p * oh).double().sum(2)
        u, num = sp + cnt.double() + 1e-6, 2.0 * si + 1e-6
        k2 = float(_f(wd)) ** 2 * wc.double() / (float(b) * float(c))
        al, be = (k2 * num / (u * u)).float(), (k2 * 2.0 / u).float()
        ld = float((wc.double() * (1.0 - num / u)).sum(1).div(c).sum() / b)
    # false positive coefficients
    fg, fv, lp = torch.zeros(b, c), torch.zeros(b, c), 0.0
    if mask & 4:
        a = cnt == 0
        if mutate != "fp_no_exception":
            a = a & ~((ign > 0)[:, None] & (torch.arange(c) == 0)[None])
        r = 1.0 / (a.sum(1).float() + _f(1e-6))
        fv = torch.where(a, r[:, None].expand(b, c), _f(0.0))
        nvalid = n - int(ign.sum())
        if nvalid > 0:
            fg = (float(_f(wp)) ** 2 * fv.double() / float(nvalid)).float()
        if mutate == "fp_scale":
            fg = fg * 1.02
    fpm = notign.float()
    grad = fk[:, None] * (sm - oh.float())
    if mask & 6:
        g = al[:, :, None] + fg[:, :, None] * fpm[:, None]
        if mutate != "dice_no_beta":
            g = g - torch.where(oh, be[:, :, None].expand(b, c, hw), _f(0.0))
        s, fps = torch.zeros(b, hw), torch.zeros(b, hw)
        for k in range(c):
            s = s + p[:, k] * g[:, k]
            fps = fps + p[:, k] * fv[:, k, None]
        grad = grad + p * (g - s[:, None])
        if mask & 4:
            lp = float((fps * fpm).double().sum() / float(n - int(ign.sum()))) if n > int(ign.sum()) else math.nan
    comps = [float(_f(float(_f(wf)) * lf)), float(_f(float(_f(wd)) * ld)), float(_f(float(_f(wp)) * lp))]
    value = float(_f(float(_f(wf)) ** 2 * lf + float(_f(wd)) ** 2 * ld + float(_f(wp)) ** 2 * lp))
    return {"grad": grad.reshape(b, c, h, w), "components": comps, "value": value}


def logits_figures(shape, profile: str, pattern: str, mask: int, gamma: float, cwt: bool, got: dict) -> dict:
    """The error figures of one launch's outputs ({"grad", "components", "value"}) against the fp64 reference."""
    ref = reference(shape, profile, pattern, mask, gamma, cwt)
    parts = [ref["parts"][k] for k in MASK_PARTS[mask]]
    fig = {"grad": image_ratio(got["grad"], parts), "batch": image_ratio(got["grad"].reshape(1, -1), [p.reshape(1, -1) for p in parts]),
           "value": rel(got["value"], ref["value"])}
    for i, name in enumerate(("focal", "dice", "fp")):
        if name in MASK_PARTS[mask]:
            fig["value"] = max(fig["value"], rel(got["components"][i], ref["components"][i]))
        elif got["components"][i] != 0.0:
            fig["value"] = math.inf
    return fig


@functools.lru_cache(maxsize=None)
def logits_constants() -> dict:
    """{(kind, component, profile, shape): constant}: the largest figure of the stable fp32 restatement over every target pattern, gamma
    and class-weighting switch the GPU tests run at that shape, floored at u.  kind: "grad" the per-image measure, "batch" the same
    measure with the whole batch as one image, "value".  (Per shape, because the per-image measure is ill-conditioned on the 2 x 2
    images of (2049, 2, 2, 2): four pixels that are all confident leave an image whose largest gradient is itself a rounding
    residue.  That shape is there for its launch geometry; the whole-batch measure is what holds the kernel there.)"""
    out = {}
    for shape in MAIN_SHAPES + EDGE_SHAPES:
        for profile in profiles_for(shape):
            for pattern in patterns_for(profile, shape):
                x, t = inputs(shape, profile, pattern)
                for mask, gamma, cwt in runs_for(pattern):
                    fig = logits_figures(shape, profile, pattern, mask, gamma, cwt, logits32(x, t, mask, gamma, cwt))
                    for kind in ("grad", "batch", "value"):
                        key = (kind, MASK_NAME[mask], profile, tuple(shape))
                        out[key] = max(out.get(key, U), fig[kind])
    return out


def logits_tol(kind: str, mask: int, profile: str, shape) -> float:
    return MARGIN * logits_constants()[(kind, MASK_NAME[mask], profile, tuple(shape))]


# ---- embeddings --------------------------------------------------------------------------------------------------------------------
def build_emb(profile: str, mcd, flag_pattern: str, seed: int = 0) -> dict:
    m, c, d = mcd
    b, n = EMB_BATCH, m * c
    g = _seed("emb", profile, mcd, flag_pattern, seed)
    noise = torch.randn(b, m, c, d, generator=g, dtype=torch.float64)
    if profile == "default":
        e = noise
    elif profile == "balanced":
        e = noise
    elif profile == "saturated":
        sign = torch.where(torch.rand(b, m, c, 1, generator=g) < 0.5, -1.0, 1.0).double()
        e = sign * torch.randn(b, 1, 1, d, generator=g, dtype=torch.float64) + 0.05 * noise
    else:
        raise ValueError(profile)
    rows = e.reshape(b, n, d)
    rows[0, SPECIAL_ROWS["below_eps"]] *= 1e-14
    rows[0, SPECIAL_ROWS["zero"]] = 0.0
    r = rows[0, SPECIAL_ROWS["above_eps"]]
    rows[0, SPECIAL_ROWS["above_eps"]] = r / r.norm() * 1.5e-12
    flags = torch.ones(b, n, dtype=torch.uint8)
    if flag_pattern == "all_on":
        pass
    elif flag_pattern == "no_flag_image":
        flags[1] = 0
    elif flag_pattern == "single_flag_image":
        flags[1] = 0
        flags[1, n // 2] = 1
    elif flag_pattern == "most_on":
        flags = (torch.rand(b, n, generator=g) < 0.85).to(torch.uint8)
        flags[:, 0] = 0
        flags[0, list(SPECIAL_ROWS.values())] = 1
    else:
        raise ValueError(flag_pattern)
    tp, bs = EMB_PROFILES[profile]
    return {"emb": rows.reshape(b, m, c, d).float().contiguous(), "flags": flags.reshape(b, m, c), "t_prime": torch.tensor([tp], dtype=F32),
            "bias": torch.tensor([bs], dtype=F32)}


def contrastive64(case: dict, y=None) -> dict:
    """fp64 loss and gradients of R.prompt_contrastive, plus the positive- and negative-pair parts of d emb."""
    e = case["emb"].double().requires_grad_(True)
    tp, bs = case["t_prime"].double().requires_grad_(True), case["bias"].double().requires_grad_(True)
    pr = R.prompt_contrastive_pairs(e, case["flags"], tp, bs, y)
    gpos = torch.autograd.grad(pr["positive"], e, retain_graph=True)[0]
    gneg = torch.autograd.grad(pr["negative"], e, retain_graph=True)[0]
    loss = pr["positive"] + pr["negative"]
    dt, db = torch.autograd.grad(loss, (tp, bs))
    return {"loss": float(loss.detach()), "demb": gpos + gneg, "demb_pos": gpos, "demb_neg": gneg, "dt": float(dt), "db": float(db),
            "u": pr["u"].detach(), "y": pr["y"]}


def check_emb_profile(profile: str, flag_pattern: str, case: dict) -> dict:
    emb, flags = case["emb"], case["flags"]
    b, m, c, d = emb.shape
    n = m * c
    assert emb.dtype == F32 and bool(torch.isfinite(emb).all())
    assert (float(case["t_prime"]), float(case["bias"])) == tuple(float(_f(v)) for v in EMB_PROFILES[profile]), f"{profile}: t' / bias"
    nrm = emb.double().reshape(b, n, d).norm(dim=-1)
    f = flags.reshape(b, n) != 0
    sp = {k: float(nrm[0, r]) for k, r in SPECIAL_ROWS.items()}
    assert 0 < sp["below_eps"] < 1e-12 and sp["zero"] == 0.0 and 1e-12 < sp["above_eps"] < 2e-12, f"special rows missing: {sp}"
    assert all(bool(f[0, r]) for r in SPECIAL_ROWS.values()), "a special row is not flagged"
    others = torch.ones(b, n, dtype=torch.bool)
    others[0, list(SPECIAL_ROWS.values())] = False
    assert float(nrm[others].min()) > 1e-3
    cnt = f.sum(1)
    if flag_pattern == "all_on":
        assert int(cnt.min()) == n
    elif flag_pattern == "no_flag_image":
        assert int(cnt[1]) == 0 and int(cnt[0]) > 1
    elif flag_pattern == "single_flag_image":
        assert int(cnt[1]) == 1 and int(cnt[0]) > 1
    elif flag_pattern == "most_on":
        assert 0.7 * n <= int(cnt.min()) and int(cnt.max()) < n, "most_on: not ~85 % of the flags"
    else:
        raise ValueError(flag_pattern)
    ref = contrastive64(case)
    live = others.clone().reshape(b, n)
    fig = {"flags": cnt.tolist()}
    if profile == "balanced":
        pos = float(ref["demb_pos"].reshape(b, n, d)[live].abs().max())
        neg = float(ref["demb_neg"].reshape(b, n, d)[live].abs().max())
        assert 0.1 <= pos / neg <= 10.0, f"balanced: positive / negative pair gradients {pos:.3g} / {neg:.3g}"
        fig["pos / neg"] = pos / neg
    if profile == "saturated":
        u = ref["u"]
        assert float(u.max()) > 20.0 and float(u.min()) < -20.0, "saturated: u does not pass +-20 on both sides"
        assert float(u.abs().max()) <= 38.0
        fig["u range"] = (float(u.min()), float(u.max()))
    return fig


@functools.lru_cache(maxsize=None)
def emb_case(profile: str, mcd, flag_pattern: str):
    """(inputs, fp64 reference) of one contrastive case, checked; built once per process."""
    case = build_emb(profile, mcd, flag_pattern)
    check_emb_profile(profile, flag_pattern, case)
    return case, contrastive64(case)


def contrastive32(case: dict, mutate: str = "") -> dict:
    """pc_normalize -> pc_pairs -> pc_fold in fp32 torch arithmetic (the pair sums in fp64, as the kernel holds them)."""
    emb, flags = case["emb"], case["flags"]
    b, m, c, d = emb.shape
    n = m * c
    e = emb.reshape(b, n, d)
    f = flags.reshape(b, n) != 0
    nrm = torch.sqrt((e * e).sum(-1))
    dd = torch.maximum(nrm, _f(1e-12))
    eh = e / dd[..., None]
    s = eh @ eh.transpose(1, 2)
    et, bs = torch.exp(case["t_prime"][0]), case["bias"][0]
    cls = torch.arange(n) % c
    y = torch.where(cls[:, None] == cls[None, :], 1.0, -1.0)
    if mutate == "y_flip":
        y = flipped_labels(n, c).float()
    pair = f[:, :, None] & f[:, None, :] & ~torch.eye(n, dtype=torch.bool)[None]
    valid = f.sum(1).float()
    inv = torch.where(valid > 0, 1.0 / (valid * _f(float(b))), _f(0.0))[:, None, None]
    z = s * et + bs
    u = -y * z
    dz = torch.where(pair, -y * torch.sigmoid(u) * inv, _f(0.0))
    gm = dz * et
    upper = torch.triu(pair, diagonal=1)
    loss = float(torch.where(upper, torch.nn.functional.softplus(u) * inv, _f(0.0)).double().sum())
    dt = float(torch.where(upper, dz * s * et, _f(0.0)).double().sum())
    db = float(torch.where(upper, dz, _f(0.0)).double().sum())
    gi = gm @ eh
    dot = (eh * gi).sum(-1, keepdim=True)
    through = (nrm >= _f(1e-12))[..., None]
    if mutate == "clamp_all":
        through = torch.zeros_like(through)
    demb = torch.where(through, (gi - eh * dot) / nrm[..., None], gi / dd[..., None])
    return {"loss": float(_f(loss)), "demb": demb.reshape(b, m, c, d), "dt": float(_f(dt)), "db": float(_f(db))}


def flipped_labels(n: int, c: int) -> torch.Tensor:
    """the class rule with y flipped on the negative pairs whose i + j is a multiple of 10 (10 % of them)"""
    cls = torch.arange(n) % c
    same = cls[:, None] == cls[None, :]
    ij = torch.arange(n)[:, None] + torch.arange(n)[None, :]
    return torch.where(same | (ij % 10 == 0), 1.0, -1.0).double()


def contrastive_figures(ref: dict, got: dict) -> dict:
    return {"demb": row_ratio(got["demb"], ref["demb"]), "loss": rel(got["loss"], ref["loss"]), "dt": rel(got["dt"], ref["dt"]),
            "db": rel(got["db"], ref["db"])}


@functools.lru_cache(maxsize=None)
def contrastive_constants() -> dict:
    """{(figure, profile): constant} of contrastive32 over every (m, c, d) and flag pattern, floored at u."""
    out = {}
    for profile in EMB_PROFILES:
        for mcd in EMB_SHAPES:
            for fp in FLAG_PATTERNS:
                case, ref = emb_case(profile, mcd, fp)
                for k, v in contrastive_figures(ref, contrastive32(case)).items():
                    out[(k, profile)] = max(out.get((k, profile), U), v)
    return out


def contrastive_tol(figure: str, profile: str) -> float:
    return MARGIN * contrastive_constants()[(figure, profile)]


# ---- AdamW -------------------------------------------------------------------------------------------------------------------------
def adamw_inputs(n: int, zero: bool = False, seed: int = 0):
    """(p, g, m, v) fp32: parameters over four orders of magnitude, so that the update is the larger term on some and the smaller on
    others; ``zero``: an all-zero gradient on zero moments."""
    gen = _seed("adamw", n, seed)
    p = torch.randn(n, generator=gen) * torch.pow(10.0, -4.0 * torch.rand(n, generator=gen))
    if zero:
        return p, torch.zeros(n), torch.zeros(n), torch.zeros(n)
    g = torch.randn(n, generator=gen) * torch.pow(10.0, -3.0 * torch.rand(n, generator=gen))
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    return p, g, m, v


def _hyper32(weight_decay: float) -> dict:
    """the hyper-parameters as the fp32 numbers the entry point is handed"""
    return {k: float(_f(v)) for k, v in dict(ADAMW_HYPER, wd=weight_decay).items()}


def adamw64(p, g, m, v, step: int, weight_decay: float, grad_scale: float) -> dict:
    """The update order documented above adamw_kernel, in fp64 on the fp32 inputs and hyper-parameters:
    p *= 1 - lr wd;  m += (g - m) (1 - b1);  v = v b2 + (1 - b2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
    -> new p, m, v and the element-wise scales of their rounding errors (the magnitudes of the terms each is put together from)."""
    hp = _hyper32(weight_decay)
    gd = g.double() * float(_f(grad_scale))
    pd = p.double() * (1.0 - hp["lr"] * hp["wd"])
    md = m.double() + (gd - m.double()) * (1.0 - hp["beta1"])
    vd = v.double() * hp["beta2"] + (1.0 - hp["beta2"]) * gd * gd
    bc1, bc2 = 1.0 - hp["beta1"] ** step, 1.0 - hp["beta2"] ** step
    upd = (hp["lr"] / bc1) * (md / (vd.sqrt() / math.sqrt(bc2) + hp["eps"]))
    # m + (g - m)(1 - b1) can cancel: the rounding of the new moment, and of the update it drives, scales with its two terms
    scale_m = m.double().abs() + (gd - m.double()).abs() * (1.0 - hp["beta1"])
    scale_upd = (hp["lr"] / bc1) * (scale_m / (vd.sqrt() / math.sqrt(bc2) + hp["eps"]))
    return {"p": pd - upd, "m": md, "v": vd, "scale_p": pd.abs() + scale_upd, "scale_m": scale_m, "scale_v": vd}


def adamw32(p, g, m, v, step: int, weight_decay: float, grad_scale: float) -> dict:
    """adamw_kernel and the host part of la_adamw_step in fp32 torch arithmetic."""
    hp = {k: _f(val) for k, val in dict(ADAMW_HYPER, wd=weight_decay).items()}
    bc1 = 1.0 - torch.pow(hp["beta1"], _f(float(step)))
    bc2_sqrt = torch.sqrt(1.0 - torch.pow(hp["beta2"], _f(float(step))))
    step_size = hp["lr"] / bc1
    gi = g * _f(grad_scale)
    pi = p * (1.0 - hp["lr"] * hp["wd"])
    mi = m + (gi - m) * (1.0 - hp["beta1"])
    vi = v * hp["beta2"] + ((1.0 - hp["beta2"]) * gi) * gi
    pi = pi - step_size * (mi / (torch.sqrt(vi) / bc2_sqrt + hp["eps"]))
    return {"p": pi, "m": mi, "v": vi}


def adamw_ratio(got: dict, ref: dict) -> dict:
    """max element-wise |got - ref| / scale for p, m and v; where the scale is 0 the error must be 0."""
    out = {}
    for k in ("p", "m", "v"):
        gd, scale = got[k].detach().double().cpu(), ref["scale_" + k]
        if not bool(torch.isfinite(gd).all()):
            out[k] = math.inf
            continue
        err, dead = (gd - ref[k]).abs(), scale == 0
        out[k] = math.inf if bool((err[dead] != 0).any()) else (float((err[~dead] / scale[~dead]).max()) if bool((~dead).any()) else 0.0)
    return out


def adamw_cases():
    for n in ADAMW_N:
        for step in (1, 1000):
            for wd in (0.0, 0.01):
                for gs in (1.0, 0.25):
                    yield n, step, wd, gs


@functools.lru_cache(maxsize=None)
def adamw_constants() -> dict:
    """{"p" | "m" | "v": constant} of adamw32 over every case of the GPU test - the same buffers, the long one included: the largest of
    a million element-wise errors is larger than the largest of a few thousand - floored at u."""
    out = {"p": U, "m": U, "v": U}
    for n, step, wd, gs in adamw_cases():
        args = adamw_inputs(n)
        for k, val in adamw_ratio(adamw32(*args, step, wd, gs), adamw64(*args, step, wd, gs)).items():
            out[k] = max(out[k], val)
    return out


def adamw_tol(which: str) -> float:
    return MARGIN * adamw_constants()[which]
