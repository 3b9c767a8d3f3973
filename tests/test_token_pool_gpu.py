"""GPU: la_mask_embed_pooled (csrc/dec.hip), the dense-prompt kernel of the TokenPool prompt encoder, called directly on guarded buffers
against a float64 torch reference on the CPU built from the same fp32 inputs.  Helpers, the three kinds of assertion and the guard
convention are those of tests/test_decoder_ops_gpu.py.

Definition (prompt_encoder.py:880-896): src[s, pix, :] = support[s, pix, :] + sum_c (dense[s, c, pix, :] + class_enc[c, :]) with dense[s, c]
the resampled mask embedding of pair (s, c), not_a_mask where flags[s, c] == 0, no_mask without mask prompts.  The reference below keeps
that order (1x1 convolution, then resample, then the class sum on the D-wide maps); the kernel sums the 16-channel hidden maps of the valid
classes first - the commutation is what is checked.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import lam_oracle as O
from tests import test_decoder_ops_gpu as T
from tests.helpers import GUARD, L, NAN, check_guards, guarded, untouched

pytestmark = pytest.mark.gpu

MD = T.MD
#          Hm   g    D  S  C
SHAPES = {
    "identity_c1": (64, 16, 64, 2, 1),        # identity resample; C = 1 is la_mask_embed
    "identity": (64, 16, 256, 3, 3),
    "reduce30": (256, 30, 64, 2, 5),          # 64 -> 30, hw = 900 = 28 pixel blocks + a tail of 4
    "ratio15": (32, 15, 320, 1, 4),           # 8 -> 15 (non-integer ratio), D above one 256-thread pass
}
PATTERNS = ("valid", "mixed", "zero")
_inputs = {}
_refs = {}


def flags_of(pattern, s, c):
    if pattern == "valid":
        return torch.ones(s, c, dtype=torch.int32)
    if pattern == "zero":
        return torch.zeros(s, c, dtype=torch.int32)
    return ((torch.arange(s).view(s, 1) + torch.arange(c).view(1, c)) % 2).to(torch.int32)      # mixed: (s + c) odd is valid


def inputs(name):
    """fp32 CPU inputs of a shape (built once)."""
    if name in _inputs:
        return _inputs[name]
    hm, g, d, s, c = SHAPES[name]
    gen = torch.Generator().manual_seed(900 + sorted(SHAPES).index(name))

    def r(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale

    w = {MD + ".0.weight": r(4, 1, 2, 2, scale=0.7), MD + ".0.bias": r(4, scale=0.5),
         MD + ".1.weight": 1.0 + r(4, scale=0.1), MD + ".1.bias": r(4, scale=0.1),
         MD + ".3.weight": r(16, 4, 2, 2, scale=0.25), MD + ".3.bias": r(16, scale=0.5),
         MD + ".4.weight": 1.0 + r(16, scale=0.1), MD + ".4.bias": r(16, scale=0.1),
         MD + ".6.weight": r(d, 16, 1, 1, scale=0.25), MD + ".6.bias": r(d, scale=0.5),
         "not_a_mask": r(d), "no_mask": r(d)}
    masks = (torch.rand(s * c, hm, hm, generator=gen) < 0.5).float()
    masks[0, :, : hm // 2] = 1.0
    masks[-1] = 0.0
    masks[-1, hm - 1, hm - 1] = 1.0
    inp = {"w": w, "masks": masks, "support": r(s, g * g, d), "class_enc": r(c, d), "pe": r(g * g, d)}
    _inputs[name] = inp
    return inp


def wlist_of(w):
    wl = [w[MD + ".0.weight"], w[MD + ".0.bias"], w[MD + ".1.weight"], w[MD + ".1.bias"], w[MD + ".3.weight"], w[MD + ".3.bias"],
          w[MD + ".4.weight"], w[MD + ".4.bias"], w[MD + ".6.weight"].flatten(1), w[MD + ".6.bias"], w["not_a_mask"], w["no_mask"]]
    return [t.contiguous().cuda() for t in wl]


def pooled_ref(name, pattern, has_masks, has_support, has_class, dtype):
    """The definition, in its own order -> [S, hw, D].  Computed once per (shape, flags, variant, dtype) and shared."""
    key = (name, pattern, has_masks, has_support, has_class, dtype)
    if key in _refs:
        return _refs[key]
    hm, g, d, s, c = SHAPES[name]
    inp = inputs(name)
    w = {k: v.to(dtype) for k, v in inp["w"].items()}
    p = s * c
    if has_masks:
        dkey = (name, dtype)
        if dkey not in _refs:                                       # the mask embedding of every pair does not depend on the flags
            _refs[dkey] = O.mask_downscale(w, inp["masks"].to(dtype).unsqueeze(1))
        dense = _refs[dkey]
        missing = (flags_of(pattern, s, c).reshape(p) == 0).view(p, 1, 1, 1)
        dense = torch.where(missing, w["not_a_mask"].view(1, d, 1, 1).expand_as(dense), dense)
        if dense.shape[-1] != g:
            dense = F.interpolate(dense, size=(g, g), mode="bilinear", align_corners=False)
    else:
        dense = w["no_mask"].view(1, d, 1, 1).expand(p, d, g, g)
    dense = dense.permute(0, 2, 3, 1).reshape(s, c, g * g, d)
    if has_class:
        dense = dense + inp["class_enc"].to(dtype).view(1, c, 1, d)
    out = dense.sum(dim=1)
    if has_support:
        out = inp["support"].to(dtype) + out
    _refs[key] = out
    return out


def call(L, name, pattern, *, has_masks=True, has_support=True, has_class=True, with16=True, dt="f16", sup=None):
    """One launch on guarded outputs -> (src32 [S, hw, D], src16, srcpe16, pe).  sup: run support ``sup`` alone (S = 1)."""
    hm, g, d, s, c = SHAPES[name]
    hw = g * g
    inp = inputs(name)
    flags = flags_of(pattern, s, c)
    masks, support = inp["masks"], inp["support"]
    if sup is not None:
        masks, flags, support, s = masks[sup * c:(sup + 1) * c], flags[sup:sup + 1], support[sup:sup + 1], 1
    code, tdt = getattr(L, T.DTS[dt][0]), T.DTS[dt][1]
    cols16 = 2 * d if dt == "f16x2" else d
    b32, src32 = guarded(s * hw, d)
    b16, src16 = guarded(s * hw, cols16, dtype=tdt) if with16 else (None, None)
    bpe, srcpe16 = guarded(s * hw, cols16, dtype=tdt) if with16 else (None, None)
    pe = inp["pe"].cuda()
    L.mask_embed_pooled(masks.contiguous().cuda() if has_masks else None, flags.reshape(-1).contiguous().cuda() if has_masks else None, s, c,
                        hm if has_masks else 0, g, d, wlist_of(inp["w"]), support.contiguous().cuda() if has_support else None,
                        inp["class_enc"].cuda() if has_class else None, pe, src32, src16, srcpe16, code)
    check_guards(b32, src32)
    if with16:
        check_guards(b16, src16)
        check_guards(bpe, srcpe16)
    return src32.view(s, hw, d), src16, srcpe16, pe


def run(L, name, pattern, **kw):
    hm, g, d, s, c = SHAPES[name]
    hw = g * g
    has_masks, has_support, has_class = kw.get("has_masks", True), kw.get("has_support", True), kw.get("has_class", True)
    dt = kw.get("dt", "f16")
    src32, src16, srcpe16, pe = call(L, name, pattern, **kw)
    label = f"mask_embed_pooled {name} flags={pattern} masks={has_masks} support={has_support} class={has_class} dt={dt}"
    T.check_measured(label, src32, pooled_ref(name, pattern, has_masks, has_support, has_class, torch.float64),
                     pooled_ref(name, pattern, has_masks, has_support, has_class, torch.float32))
    if src16 is not None:
        assert T.sixteen_ok(src16, src32.reshape(s * hw, d), dt, d), "src16 is not the stored form of src32"
        assert T.sixteen_ok(srcpe16, (src32 + pe).view(s * hw, d), dt, d), "srcpe16 is not the stored form of src32 + pe"
    # supports without a valid class: C x the learned row, + the class rows in ascending c, + support: the kernel's fp32 order, bit for bit
    inp = inputs(name)
    flags = flags_of(pattern, s, c)
    base = (inp["w"]["not_a_mask"] if has_masks else inp["w"]["no_mask"]).cuda()
    rows = [i for i in range(s) if not has_masks or int(flags[i].sum()) == 0]
    assert rows or pattern != "zero"
    for i in rows:
        v = float(c) * base
        if has_class:
            for k in range(c):
                v = v + inp["class_enc"][k].cuda()
        v = v.unsqueeze(0) + inp["support"][i].cuda() if has_support else v.unsqueeze(0).expand(hw, d)
        assert torch.equal(src32[i], v), f"support {i} is not C x not_a_mask / no_mask + class rows + support"
    return src32


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_geometries_and_flag_patterns(L, name, pattern):
    """la_mask_embed_pooled at every resample regime (identity, reduction with an hw % 32 tail, non-integer ratio, D above one 256-thread
    pass) with all classes valid, mixed flags and no valid class, against the fp64 definition."""
    run(L, name, pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_class_is_la_mask_embed(L, pattern):
    """C = 1: the pooled kernel and la_mask_embed on the same inputs agree to within 1 ulp, element by element."""
    name = "identity_c1"
    hm, g, d, s, c = SHAPES[name]
    hw = g * g
    inp = inputs(name)
    got, _, _, pe = call(L, name, pattern, with16=False)
    b32, plain = guarded(s * hw, d)
    L.mask_embed(inp["masks"].cuda(), flags_of(pattern, s, c).reshape(-1).cuda(), s, 1, hm, g, d, wlist_of(inp["w"]), inp["support"].cuda(),
                 inp["class_enc"].cuda(), pe, plain, None, None, L.LA_F16)
    check_guards(b32, plain)
    a, b = got.reshape(-1).cpu(), plain.reshape(-1).cpu()
    inf = torch.full_like(b, float("inf"))
    ok = (a == b) | (a == torch.nextafter(b, inf)) | (a == torch.nextafter(b, -inf))
    print(f"[1 ulp] pooled C = 1 vs la_mask_embed, flags={pattern}: {int((a != b).sum())} of {a.numel()} elements differ")
    assert bool(ok.all())


@pytest.mark.parametrize("variant", ["no_masks", "no_support", "no_class", "no_16", "f32", "f16", "bf16", "f16x2"])
@pytest.mark.parametrize("name", ["identity", "ratio15"])
def test_variants(L, name, variant):
    """la_mask_embed_pooled without masks (C x no_mask), without support, without class encoding, without the 16-bit operands and in every
    storage type of the 16-bit operands (the ``sixteen_ok`` property), on mixed flags."""
    kw = {"no_masks": dict(has_masks=False), "no_support": dict(has_support=False), "no_class": dict(has_class=False), "no_16": dict(with16=False),
          "f32": dict(dt="f32"), "f16": dict(dt="f16"), "bf16": dict(dt="bf16"), "f16x2": dict(dt="f16x2")}[variant]
    run(L, name, "mixed", **kw)


def test_counting_is_exact(L):
    """W6 = 0, b6 = 0, support = 0, not_a_mask = 1, class_enc[c] = 8 (c + 1): every output of support s is n_invalid(s) + 8 C (C + 1) / 2 bit
    for bit - a class counted twice, dropped or taken from another support is a whole-integer error."""
    hm, g, d, s, c = 64, 16, 64, 4, 5
    hw = g * g
    inp = inputs("identity_c1")
    w = dict(inp["w"])
    w[MD + ".6.weight"] = torch.zeros(d, 16, 1, 1)
    w[MD + ".6.bias"] = torch.zeros(d)
    w["not_a_mask"] = torch.ones(d)
    flags = torch.tensor([[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 0, 0, 0, 0], [0, 1, 1, 1, 1]], dtype=torch.int32)
    masks = (torch.rand(s * c, hm, hm, generator=torch.Generator().manual_seed(77)) < 0.5).float().cuda()
    class_enc = (8.0 * (torch.arange(c) + 1)).view(c, 1).expand(c, d).contiguous().cuda()
    b32, src32 = guarded(s * hw, d)
    L.mask_embed_pooled(masks, flags.reshape(-1).cuda(), s, c, hm, g, d, wlist_of(w), torch.zeros(s, hw, d, device="cuda"), class_enc,
                        torch.zeros(hw, d, device="cuda"), src32, None, None, L.LA_F32)
    check_guards(b32, src32)
    want = ((flags == 0).sum(dim=1).float() + 8.0 * c * (c + 1) / 2).view(s, 1, 1).expand(s, hw, d)
    assert torch.equal(src32.view(s, hw, d).cpu(), want)


def test_a_support_alone_gives_the_bits_of_the_batch_and_runs_repeat(L):
    name = "identity"
    s = SHAPES[name][3]
    batch = run(L, name, "mixed").clone()
    again = call(L, name, "mixed")[0]
    assert torch.equal(batch, again), "two runs differ"
    for i in range(s):
        alone = call(L, name, "mixed", sup=i)[0]
        assert torch.equal(alone[0], batch[i]), f"support {i} alone differs from the batch"


@pytest.mark.parametrize("bad", ["S=0", "C=0", "C<0", "g=0", "D=0", "Hm%4", "Hm=0", "dtype", "null_pe", "null_out", "S>65535"])
def test_refused_arguments_write_nothing(L, bad):
    hm, g, d, s, c = SHAPES["identity_c1"]
    hw = g * g
    inp = inputs("identity_c1")
    buf = torch.full((s * hw * d + 2 * GUARD,), NAN, device="cuda")
    b16 = torch.full((s * hw * d + 2 * GUARD,), NAN, device="cuda", dtype=torch.float16)
    out = buf[GUARD:GUARD + s * hw * d].view(s * hw, d)
    o16 = b16[GUARD:GUARD + s * hw * d].view(s * hw, d)
    a = dict(masks=inp["masks"].cuda(), flags=flags_of("valid", s, c).reshape(-1).cuda(), s=s, c=c, hm=hm, g=g, d=d, pe=inp["pe"].cuda(), out=out,
             dt=L.LA_F16)
    a.update({"S=0": dict(s=0), "C=0": dict(c=0), "C<0": dict(c=-1), "g=0": dict(g=0), "D=0": dict(d=0), "Hm%4": dict(hm=30), "Hm=0": dict(hm=0),
              "dtype": dict(dt=99), "null_pe": dict(pe=None), "null_out": dict(out=None), "S>65535": dict(s=65536)}[bad])
    with pytest.raises(RuntimeError, match="la_mask_embed_pooled"):
        L.mask_embed_pooled(a["masks"], a["flags"], a["s"], a["c"], a["hm"], a["g"], a["d"], wlist_of(inp["w"]), inp["support"].cuda(),
                            inp["class_enc"].cuda(), a["pe"], a["out"], o16, None, a["dt"])
    assert untouched(buf) and bool(torch.isnan(b16).all())
