"""Ill-conditioned LayerNorm rows, plain fp64 references and fp32 restatements of both variance forms, for
tests/test_norm_profiles_cpu.py, tests/test_layernorm_forward_gpu.py and tests/test_normfold_conditioning_gpu.py.  No kernel code.

The direct kernels (csrc/norm.hip: layernorm_kernel, norm_stats_kernel) take the variance in two passes - mean first, then centred
squares.  The folded form ("LayerNorm folded into the GEMMs") takes it in ONE pass from the producer GEMM's partial sums:
var = max(sum x^2 / E - mean^2, 0), relative error eps32 (1 + mean^2 / sigma^2).  Rows drawn from N(0, 1) never leave the corner where
both forms are exact to a few ulp; the builders below make fp32 rows [m, E] with stated properties, ``check_profile`` measures those
properties in fp64 on the fp32 values and raises when one is missing.

Notation: u = 2^-24; per row mu, sigma^2 in fp64 of the fp32 row actually normalised (with x2 that is fl32(x + x2): the add is not in the
budget); s = sqrt(sigma^2 + eps); rho = mu^2 / s^2; z = (t - mu) / s.

    centred     mu ~ 0, sigma in {1e-3, 1, 300} (row i has sigma CENTRED_SIGMA[i % 3]): sigma^2 = 1e-6 makes eps = 1e-6 matter
    offset      |mu| / sigma in {1, 8, 32, 128, 512}, both signs, sigma = 1: the in-domain range, rho <= 2^18
    offset_out  |mu| / sigma in {2048, 8192}, both signs: out of the one-pass form's domain
    outlier     sigma = 1 noise, one channel at 200 and one at -500, placed (row by row) at columns 0, 63, 64, E - 1 and inside the last
                64-column slot: slot placement of the producer partials, tail predicate of the direct kernel
    two_level   half the channels at +a, half at -a, a with few mantissa bits: mu = 0 and sigma^2 = a^2 EXACTLY; output +-gamma + beta
    constant    every channel c, c in {0, 1, 0.3, 1000.3}: sigma^2 = 0, the true rstd is 1 / sqrt(eps)
    near_range  magnitudes up to 6e4, the neighbourhood of the fp16 saturation of the stream's 16-bit copy (sum x^2 ~ 3e12: harmless in fp32)
    mixed       row i is a row of KINDS[i % 7]: neighbours inside one 4-, 128- or 256-row tile differ by ten orders of magnitude
"""
from __future__ import annotations

import functools
import math

import torch

U = 2.0 ** -24
SLOT = 64
EPS_VALUES = (1e-6, 1e-12)
KINDS = ("centred", "offset", "offset_out", "outlier", "two_level", "constant", "near_range")
IN_DOMAIN = ("centred", "offset", "outlier", "two_level", "near_range")
OUT_OF_DOMAIN = ("offset_out", "constant")
ALL_KINDS = KINDS + ("mixed",)

CENTRED_SIGMA = (1e-3, 1.0, 300.0)
OFFSET_RATIO = tuple(s * r for r in (1.0, 8.0, 32.0, 128.0, 512.0) for s in (1.0, -1.0))
OFFSET_OUT_RATIO = (2048.0, -2048.0, 8192.0, -8192.0)
TWO_LEVEL_A = (0.75, 3.0, 2.0 ** -6, 1536.0)
CONSTANT_C = (0.0, 1.0, 0.3, 1000.3)
OUTLIER_HI, OUTLIER_LO = 200.0, -500.0

# every E of the direct-kernel case table (tests/test_layernorm_forward_gpu.py) and of the folded form
E_DIRECT = (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 1284, 2044, 2048)
E_FOLD = (512, 768, 1280)


def ln_instance(e: int):
    """(LPR, NVT, EXACT) of layernorm_kernel that launch_ln (csrc/norm.hip) picks for row width e."""
    nv = e >> 2
    lpr = 64
    while lpr > 1 and (lpr >> 1) >= nv:
        lpr >>= 1
    if lpr < 64:
        return lpr, 1, nv == lpr
    nvt = (nv + 63) // 64
    nvt = nvt if nvt <= 5 else 8
    return 64, nvt, nv == 64 * nvt


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _gen(kind: str, m: int, e: int, seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(7919 * (ALL_KINDS.index(kind) + 1) + 31 * e + 1000003 * seed + m)


def _unit_noise(m: int, e: int, gen: torch.Generator) -> torch.Tensor:
    """fp64 rows with mean 0 and (biased) variance 1 exactly up to fp64 rounding."""
    z = torch.randn(m, e, generator=gen, dtype=torch.float64)
    z = z - z.mean(1, keepdim=True)
    return z / z.pow(2).mean(1, keepdim=True).sqrt()


def outlier_columns(e: int):
    cand = [0, 63, 64, e - 1, e - SLOT + 17 if e >= 2 * SLOT else e // 2]
    out = []
    for c in cand:
        if 0 <= c < e and c not in out:
            out.append(c)
    return out


def build(kind: str, m: int, e: int, seed: int = 0) -> torch.Tensor:
    """fp32 rows [m, e] of profile ``kind``; row i takes the i-th parameter of the kind's list, cyclically."""
    gen = _gen(kind, m, e, seed)
    i = torch.arange(m)
    if kind == "centred":
        x = _unit_noise(m, e, gen) * torch.tensor(CENTRED_SIGMA, dtype=torch.float64)[i % 3, None]
    elif kind == "offset":
        x = _unit_noise(m, e, gen) + torch.tensor(OFFSET_RATIO, dtype=torch.float64)[i % len(OFFSET_RATIO), None]
    elif kind == "offset_out":
        x = _unit_noise(m, e, gen) + torch.tensor(OFFSET_OUT_RATIO, dtype=torch.float64)[i % 4, None]
    elif kind == "outlier":
        x = _unit_noise(m, e, gen)
        cols = outlier_columns(e)
        for r in range(m):
            x[r, cols[r % len(cols)]] = OUTLIER_HI
            x[r, cols[(r + 1) % len(cols)]] = OUTLIER_LO
    elif kind == "two_level":
        sign = torch.ones(m, e, dtype=torch.float64)
        for r in range(m):
            sign[r, torch.randperm(e, generator=gen)[: e // 2]] = -1.0
        x = sign * torch.tensor(TWO_LEVEL_A, dtype=torch.float64)[i % 4, None]
    elif kind == "constant":
        x = torch.tensor(CONSTANT_C, dtype=torch.float32)[i % 4, None].expand(m, e).double()
    elif kind == "near_range":
        x = (torch.rand(m, e, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * 6.0e4
        x[:, 0] = torch.where(i % 2 == 0, 6.0e4, -6.0e4).double()
    elif kind == "mixed":
        x = torch.empty(m, e, dtype=torch.float64)
        for k, name in enumerate(KINDS):
            rows = i[i % len(KINDS) == k]
            if rows.numel():
                x[rows] = build(name, rows.numel(), e, seed).double()
    else:
        raise ValueError(kind)
    return x.float().contiguous()


def kinds_of_rows(kind: str, m: int):
    """profile name of every row of ``build(kind, m, e)``"""
    return [KINDS[i % len(KINDS)] for i in range(m)] if kind == "mixed" else [kind] * m


def rows_of_kind(kind: str, m: int, name: str) -> torch.Tensor:
    return torch.tensor([i for i, k in enumerate(kinds_of_rows(kind, m)) if k == name], dtype=torch.long)


def moments64(x: torch.Tensor):
    """(mu, sigma^2) per row in fp64 of the values x holds (sigma^2 two-pass: no cancellation)."""
    xd = x.double()
    mu = xd.mean(-1)
    return mu, (xd - mu[..., None]).pow(2).mean(-1)


def check_profile(kind: str, x: torch.Tensor) -> dict:
    """Measure the stated properties of ``build(kind, ...)`` rows in fp64; AssertionError when one is missing.  -> figures."""
    m, e = x.shape
    assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    if kind == "mixed":
        fig = {}
        for name in KINDS:
            rows = rows_of_kind("mixed", m, name)
            if rows.numel():
                fig[name] = check_profile(name, x[rows])
        scale = x.double().abs().amax(1).clamp_min(1e-30)
        assert m < 14 or float(scale.max() / scale[scale > 1e-30].min()) >= 1e7, "mixed: rows of one tile do not differ in scale"
        return fig
    mu, var = moments64(x)
    sd = var.sqrt()
    i = torch.arange(m)
    if kind == "centred":
        want = torch.tensor(CENTRED_SIGMA, dtype=torch.float64)[i % 3]
        assert bool((mu.abs() <= 1e-6 * sd).all()), "centred: mean not ~ 0"
        assert bool(((sd / want - 1).abs() <= 1e-6).all()), "centred: sigma off"
        return {"max |mu| / sigma": float((mu.abs() / sd).max())}
    if kind in ("offset", "offset_out"):
        ratios = OFFSET_RATIO if kind == "offset" else OFFSET_OUT_RATIO
        want = torch.tensor(ratios, dtype=torch.float64)[i % len(ratios)]
        got = mu / sd
        # (the fp32 rounding of a row around 8192 moves sigma by ~ ulp / sqrt 12 = 3e-4 of it)
        assert bool(((got / want - 1).abs() <= 1e-2).all()), f"{kind}: mu / sigma off"
        lo, hi = (1.0, 512.0 * 1.01) if kind == "offset" else (2048.0 * 0.99, 8192.0 * 1.01)
        assert bool(((got.abs() >= lo * 0.99) & (got.abs() <= hi)).all())
        if kind == "offset":
            assert float((mu * mu / var).max()) <= 2.0 ** 18 * 1.03
        return {"max mu^2 / sigma^2": float((mu * mu / var).max()), "min": float((mu * mu / var).min())}
    if kind == "outlier":
        cols = outlier_columns(e)
        for r in range(m):
            a, b = cols[r % len(cols)], cols[(r + 1) % len(cols)]
            assert float(x[r, a]) == OUTLIER_HI and float(x[r, b]) == OUTLIER_LO, "outlier: channel not in place"
            rest = x[r].clone()
            rest[[a, b]] = 0.0
            assert float(rest.abs().max()) < 8.0, "outlier: the noise is not small"
        return {"columns": cols}
    if kind == "two_level":
        a = torch.tensor(TWO_LEVEL_A, dtype=torch.float64)[i % 4]
        assert bool((mu == 0).all()) and bool((var == a * a).all()), "two_level: mu = 0, sigma^2 = a^2 exactly"
        assert bool((x.double().abs() == a[:, None]).all())
        return {"a": list(TWO_LEVEL_A)}
    if kind == "constant":
        assert bool((x == x[:, :1]).all()), "constant: channels differ"
        want = torch.tensor(CONSTANT_C, dtype=torch.float32)[i % 4]
        assert bool((x[:, 0] == want).all())
        return {"c": list(CONSTANT_C)}
    if kind == "near_range":
        top = x.abs().amax(1)
        assert bool((top == 6.0e4).all()), "near_range: no magnitude at 6e4"
        assert e < 64 or bool((mu * mu / var <= 0.5).all())
        return {"max sum x^2": float(x.double().pow(2).sum(1).max())}
    raise ValueError(kind)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def stats64(x: torch.Tensor, eps: float):
    """(mu, 1 / s) per row, fp64."""
    mu, var = moments64(x)
    return mu, (var + eps).rsqrt()


def row_figures(x: torch.Tensor, eps: float) -> dict:
    """mu, sigma, rstd = 1 / s, rho = mu^2 / s^2 per row, fp64."""
    mu, var = moments64(x)
    return {"mu": mu, "sigma": var.sqrt(), "rstd": (var + eps).rsqrt(), "rho": mu * mu / (var + eps)}


def gelu64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def window_rows(rows: int, h: int, w: int, ws: int) -> torch.Tensor:
    """destination row of image-order row (b, y, x) in the window-partitioned layout (windows padded to ws x ws)"""
    r = torch.arange(rows)
    x, y, b = r % w, (r // w) % h, r // (w * h)
    nwx, nwy = -(-w // ws), -(-h // ws)
    return ((b * nwy + y // ws) * nwx + x // ws) * ws * ws + (y % ws) * ws + (x % ws)


def window_rows_total(rows: int, h: int, w: int, ws: int) -> int:
    return rows // (h * w) * (-(-w // ws)) * (-(-h // ws)) * ws * ws


def padded_rows(rows: int, h: int, w: int) -> torch.Tensor:
    """row of pixel (b, y, x) in zero-bordered [B, H + 2, W + 2] maps"""
    r = torch.arange(rows)
    x, y, b = r % w, (r // w) % h, r // (w * h)
    return (b * (h + 2) + y + 1) * (w + 2) + x + 1


def layernorm64(x, gamma, beta, eps, *, x2=None, x2_group=0, gelu=False, pe=None, pe_mod=0, window=0, H=0, W=0) -> dict:
    """la_layernorm / la_layernorm_g in fp64 on CPU tensors.  x: fp32 rows (window == -2: the padded maps, un-padded row count from H, W).
    -> xin   the fp32 rows actually normalised (fl32(x + x2): one IEEE add, the same on every machine)
       out   [rows, E] in ROW order (what out32 holds), z, rho, rstd, mu per row
       pe    out + pe rows (row % pe_mod), when pe is given
       dest  destination row of every row in the 16-bit outputs (window > 0: partitioned; -1: padded maps; else the row itself)"""
    if window == -2:
        rows = x.shape[0] // ((H + 2) * (W + 2)) * H * W
        x = x[padded_rows(rows, H, W)]
    rows = x.shape[0]
    xin = x.float()
    if x2 is not None:
        xin = xin + (x2.float()[torch.arange(rows) // x2_group] if x2_group > 0 else x2.float())      # fp32 add
    f = row_figures(xin, eps)
    z = (xin.double() - f["mu"][:, None]) * f["rstd"][:, None]
    out = z * gamma.double() + beta.double()
    if gelu:
        out = gelu64(out)
    res = dict(f, xin=xin, z=z, out=out, dest=torch.arange(rows))
    if pe is not None:
        res["pe"] = out + pe.double()[torch.arange(rows) % pe_mod if pe_mod else torch.arange(rows)]
    if window > 0:
        res["dest"] = window_rows(rows, H, W, window)
    elif window == -1:
        res["dest"] = padded_rows(rows, H, W)
    return res


def split16(v32: torch.Tensor):
    """The LA_F16X2 pair of fp32 values: hi = rn16(v), lo = rn16(v - hi)."""
    hi = v32.half()
    return hi, (v32 - hi.float()).half()


def consumer64(x16, wf16, ncol, bf, mean, rstd, gelu=False) -> torch.Tensor:
    """The documented consumer formula rstd (x16 W'^T - mean c) + b' in fp64 on the given rounded operands."""
    pre = rstd.double()[:, None] * (x16.double() @ wf16.double().t() - mean.double()[:, None] * ncol.double()[None, :]) + bf.double()[None, :]
    return gelu64(pre) if gelu else pre


def consumer_scale64(x16, wf16, ncol, mean, rstd) -> torch.Tensor:
    """rstd (sum_k |x_k| |w_jk| + |mean c_j|): what the consumer's rounding errors are proportional to."""
    return rstd.double()[:, None] * (x16.double().abs() @ wf16.double().abs().t() + (mean.double()[:, None] * ncol.double()[None, :]).abs())


def fold_operands(w, b, gamma, beta):
    """(W' = rn16(W diag gamma), c = fp32 row sums of the ROUNDED W', b' = b + W beta in fp32) from fp32 CPU tensors."""
    wf = (w.double() * gamma.double()).to(torch.float16)
    ncol = wf.double().sum(1).float()
    bf = (b.double() + w.double() @ beta.double()).float()
    return wf, ncol, bf


def fold_chain64(res, add, gamma, beta, eps, w, b, gelu=False) -> torch.Tensor:
    """residual add -> LayerNorm -> Linear, all in fp64: the function the folded chain stands for."""
    x = res.double() + (add.double() if add is not None else 0.0)
    mu, rstd = stats64(x, eps)
    y = ((x - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()) @ w.double().t() + b.double()
    return gelu64(y) if gelu else y


# ---- fp32 restatements of the two variance forms -----------------------------------------------------------------------------------
def twopass32(x: torch.Tensor, eps: float):
    """(mean, rstd) in fp32, two passes: mean first, then centred squares (layernorm_kernel, norm_stats_kernel)."""
    e = x.shape[1]
    mean = x.sum(1) / e
    d = x - mean[:, None]
    var = (d * d).sum(1) / e
    return mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def _tree64(v: torch.Tensor) -> torch.Tensor:
    """fp32 sums of groups of 64 consecutive columns by a balanced pairwise tree: the producer epilogue's order (eight columns in a
    lane as ((0+1)+(2+3))+((4+5)+(6+7)), then the eight lanes of the row folded by lane ^ 1, lane ^ 2 and the half mirror)."""
    m, e = v.shape
    v = v.reshape(m, e // SLOT, SLOT)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def slot_sums32(x: torch.Tensor):
    """(sum x, sum x^2) per 64-column slot in fp32, squares rounded before they are added: [m, E / 64] each."""
    return _tree64(x), _tree64(x * x)


def finalize32(s1: torch.Tensor, s2: torch.Tensor, e: int, eps: float, clamp: bool = True):
    """norm_finalize_kernel's documented order: slots added in index order, var = max(s2 / E - mean^2, 0)."""
    a, b = torch.zeros_like(s1[:, 0]), torch.zeros_like(s2[:, 0])
    for j in range(s1.shape[1]):
        a = a + s1[:, j]
        b = b + s2[:, j]
    mean = a / e
    var = b / e - mean * mean
    if clamp:
        var = var.clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def onepass32(x: torch.Tensor, eps: float):
    """(mean, rstd) in fp32 from 64-column slot sums of x and x^2 (E % 64 == 0)."""
    s1, s2 = slot_sums32(x)
    return finalize32(s1, s2, x.shape[1], eps)


def _ratio(err: torch.Tensor, scale: torch.Tensor) -> float:
    """max err / scale; where scale is 0 the error must be 0 too"""
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "an error where the model allows none"
    return float((err[~zero] / scale[~zero]).max()) if bool((~zero).any()) else 0.0


def measure_constants(m: int = 140) -> dict:
    """The error constants of the fp32 restatements over every profile:
       C_mean   max |d mu| / (u (|mu| + sigma))            both forms, every profile, every E
       C_two    max relative rstd error of twopass32 / u    every profile, every E: the error of the rstd of the variance ABOUT THE COMPUTED
                MEAN, sigma^2 + (mu - mean32)^2 - the two-pass form is exact in that up to rounding, whatever the mean's error
       C_one    max relative rstd error of onepass32 / (u (1 + rho))   in-domain profiles, E in E_FOLD
       C_slot   max slot-sum error / (64 u sum |terms|)     the 64-column partial sums of x and of x^2
       left_model  per |mu| / sigma of offset_out: the largest relative rstd error of onepass32, E in E_FOLD
    eps is the fp32 value the kernels are handed (1e-6 and 1e-12 are not fp32 numbers)."""
    c_mean = c_two = c_one = c_slot = 0.0
    left = {}
    for eps in EPS_VALUES:
        eps32 = float(torch.tensor(eps, dtype=torch.float32))
        for e in sorted(set(E_DIRECT) | set(E_FOLD)):
            for kind in KINDS:
                x = build(kind, m, e)
                f = row_figures(x, eps32)
                mean, rstd = twopass32(x, eps)
                c_mean = max(c_mean, _ratio((mean.double() - f["mu"]).abs(), U * (f["mu"].abs() + f["sigma"])))
                about = (f["sigma"] ** 2 + (f["mu"] - mean.double()) ** 2 + eps32).rsqrt()
                c_two = max(c_two, float((rstd.double() / about - 1).abs().max()) / U)
                if e % SLOT:
                    continue
                s1, s2 = slot_sums32(x)
                xd = x.double().view(m, e // SLOT, SLOT)
                c_slot = max(c_slot, _ratio((s1.double() - xd.sum(2)).abs(), SLOT * U * xd.abs().sum(2)),
                             _ratio((s2.double() - xd.pow(2).sum(2)).abs(), SLOT * U * xd.pow(2).sum(2)))
                mean, rstd = onepass32(x, eps)
                c_mean = max(c_mean, _ratio((mean.double() - f["mu"]).abs(), U * (f["mu"].abs() + f["sigma"])))
                rel = (rstd.double() / f["rstd"] - 1).abs()
                if kind in IN_DOMAIN and e in E_FOLD:
                    c_one = max(c_one, float((rel / (U * (1 + f["rho"]))).max()))
                if kind == "offset_out" and e in E_FOLD:
                    for j, r in enumerate(OFFSET_OUT_RATIO):
                        key = abs(r)
                        left[key] = max(left.get(key, 0.0), float(rel[j::4].max()))
    return {"C_mean": c_mean, "C_two": c_two, "C_one": c_one, "C_slot": c_slot, "left_model": left}


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    return measure_constants()


# ---- element-wise allowances of the GPU tests --------------------------------------------------------------------------------------
def ulp32(v: torch.Tensor) -> torch.Tensor:
    """spacing of fp32 at |v| (fp64 tensor in, fp64 out)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def ulp16(v: torch.Tensor, dtype) -> torch.Tensor:
    """spacing of the 16-bit (or fp32) output type at |v|"""
    if dtype == torch.float32:
        return ulp32(v)
    if dtype == torch.float16:
        return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10)
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


def allow_out32(ref: dict, gamma, gelu: bool = False) -> torch.Tensor:
    """2 max(C_mean, C_two) u |gamma_i| (|z_i| + sqrt rho + 1) (x 1.13 with GELU, the largest slope of erf-GELU) + 2 ulp32(ref)."""
    c = constants()
    first = 2.0 * max(c["C_mean"], c["C_two"]) * U * gamma.double().abs()[None, :] * (ref["z"].abs() + ref["rho"].sqrt()[:, None] + 1.0)
    return first * (1.13 if gelu else 1.0) + 2.0 * ulp32(ref["out"])


def allow_out16(ref64: torch.Tensor, allow32: torch.Tensor, dtype) -> torch.Tensor:
    """+ half an ulp of the output type at the largest fp32 value the allowance admits, + one ulp32 (double rounding)."""
    if dtype == torch.float32:
        return allow32
    return allow32 + 0.5 * ulp16(ref64.abs() + allow32, dtype) + ulp32(ref64)


def worst(got: torch.Tensor, ref64: torch.Tensor, allow: torch.Tensor):
    """(max err / allowance, index of the first element beyond it or not finite - None when all are inside)"""
    g = got.detach().double().cpu()
    bad = ~torch.isfinite(g)
    ratio = torch.where(bad, torch.full_like(allow, math.inf), (g - ref64).abs() / allow)
    over = torch.nonzero(ratio > 1.0)
    return float(ratio.max()), (tuple(int(v) for v in over[0]) if over.numel() else None)

