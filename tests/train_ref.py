"""The training-step kernels of csrc/train.hip, csrc/gemm_tn16.hip and the optimizer step of csrc/loss.hip in float64, their derived
error allowances, the integer-exact references of the accumulating kernels, and the data every case of
tests/test_train_kernels_gpu.py runs on.

Plain torch, no device code: everything here runs on CPU and GPU tensors alike.  tests/test_train_ref_cpu.py proves the references
against torch (autograd of F.layer_norm / F.gelu, torch.optim.AdamW), the allowances against an fp32 restatement of each kernel
(inside half of them, in two summation orders) and against planted faults (each must exceed them).  No number here is fitted to
what a kernel returns: every term is a count of fp32 roundings times u = 2^-24 times the magnitude it is relative to, the stated
error of a library function, or half an ulp of a 16-bit type.
"""
import math

import torch

from tests.gemm_ref import HALF_ULP, U24, gelu_abs_err, gelu_grad64

NAN = float("nan")
U = U24
RSQRT_REL = 2.0 ** -23           # rsqrtf: 1 ulp (HIP math API), relative to the result
POW_REL = 2.0 ** -22             # powf: 2 ulp allowed (HIP states 1), relative to the power
GELU_GRAD_LIPSCHITZ = 0.8        # max |gelu''| = phi(z) |2 - z^2| at z = 0: 2 / sqrt(2 pi) = 0.798
INT_LO, INT_HI = -8, 8           # helpers.rint's range: a product is at most 64 in magnitude
MAX_REDUCTION = 8200             # the longest reduction of an integer-exact case


def gn(n):
    """gamma_n = n u / (1 - n u): the forward error factor of n fp32 roundings in a row (Higham 3.1); for a sum of n terms in ANY order
    every term passes through at most n - 1 additions, so |error| <= gamma_n sum |terms|."""
    return n * U / (1.0 - n * U)


def f32(v):
    """A Python float rounded to fp32: what a ``float`` argument of the C ABI holds."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------
def _ln64(x, dy, gamma, beta, eps, gelu, add, dt16, dgamma0, dbeta0, bound):
    """Values (and allowances when ``bound``) of la_layernorm_bwd(_res), float64.  Formulas: the header comment of layernorm_bwd_kernel,
    y = [GELU](xhat gamma + beta), xhat = (x - mu) rstd;  dz = dy [gelu'(z)];  dgamma = sum_r dz xhat;  dbeta = sum_r dz;  g = dz gamma;
    dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ add];  out16 = dx before its rounding."""
    x, dy = x.double(), dy.double()
    gm, bt = gamma.double()[None, :], beta.double()[None, :]
    rows, e = x.shape
    mean = lambda t: t.mean(1, keepdim=True)
    mu = mean(x)
    d = x - mu
    var = mean(d * d)
    rstd = (var + eps).rsqrt()
    xh = d * rstd
    if gelu:
        z = xh * gm + bt
        gg = gelu_grad64(z)
        dz = dy * gg
    else:
        dz = dy
    g = dz * gm
    s1 = mean(g)
    t = g * xh
    s2 = mean(t)
    xs = xh * s2
    inner = g - s1 - xs
    o = rstd * inner
    dx = o + add.double() if add is not None else o
    tg = dz * xh
    val = dict(dx=dx, dgamma=tg.sum(0), dbeta=dz.sum(0), out16=dx if dt16 is not None else None)
    if not bound:
        return val, None
    c = gn(e + 2)                                            # an E-term sum in any order, the product with 1 / E, and 1 / E itself
    dmu = c * mean(x.abs())
    dd = dmu + U * d.abs()                                   # x - mu: the error of mu and one rounding
    # variance + eps: the E squares (one rounding each), their sum, 1 / E, the added eps: E + 4 roundings relative to var + eps;
    # what the error of d moves it by: mean(2 |d| dd) = 2 mean|d| dmu + 2 u var
    dv = gn(e + 4) * (var + eps) + 2.0 * mean(d.abs()) * dmu + 2.0 * U * var
    drstd = 0.5 * rstd ** 3 * dv + RSQRT_REL * rstd          # |d rsqrt(V) / dV| = rstd^3 / 2 (relative: rstd^2 / 2), and rsqrtf itself
    dxh = rstd * dd + d.abs() * drstd + U * xh.abs()
    if gelu:
        dzz = gm.abs() * dxh + U * ((xh * gm).abs() + z.abs())      # z = xhat gamma + beta: two roundings (or one, as an fma)
        # gelu_grad = 0.5 (1 + erff) + z phi(z) with __expf: erff within 4 ulp of a value <= 1 (2.4e-7 on the half), z phi(z) <= 0.25
        # with __expf's few ulp - under the smallest figure gelu_abs_err returns (1.6e-6); four roundings assemble the value
        dgg = gelu_abs_err(z) + GELU_GRAD_LIPSCHITZ * dzz + 4.0 * U * gg.abs()
        ddz = dy.abs() * dgg + U * dz.abs()
    else:
        ddz = torch.zeros_like(dz)
    dg = gm.abs() * ddz + U * g.abs()
    ds1 = c * mean(g.abs()) + mean(dg)
    dt = g.abs() * dxh + xh.abs() * dg + U * t.abs()
    ds2 = c * mean(t.abs()) + mean(dt)
    # g - s1 - xhat s2: the product's rounding, two subtractions each relative to at most the sum of the magnitudes
    dinner = dg + ds1 + xh.abs() * ds2 + s2.abs() * dxh + U * xs.abs() + 2.0 * U * (g.abs() + s1.abs() + xs.abs())
    do = rstd * dinner + inner.abs() * drstd + U * o.abs()
    if add is not None:
        do = do + U * (o.abs() + add.double().abs())          # the fp32 add of the skip gradient
    allow = dict(dx=do)
    if dt16 is not None:
        allow["out16"] = do + HALF_ULP[dt16] * (dx.abs() + do) + (2.0 ** -25 if dt16 == torch.float16 else 0.0)
    # column sums over the rows in any order (per-lane partial sums, the workgroup's fold, fp32 atomics onto the pre-loaded value):
    # (rows + 8) u sum_r |term| (+ 8: the folds and the pre-loaded value's own addition) plus the terms' own allowances
    dtg = xh.abs() * ddz + dz.abs() * dxh + U * tg.abs()
    g0 = dgamma0.double().abs() if dgamma0 is not None else 0.0
    b0 = dbeta0.double().abs() if dbeta0 is not None else 0.0
    allow["dgamma"] = gn(rows + 8) * (tg.abs().sum(0) + g0) + dtg.sum(0)
    allow["dbeta"] = gn(rows + 8) * (dz.abs().sum(0) + b0) + ddz.sum(0)
    return val, allow


def layernorm_bwd64(x, dy, gamma, beta, eps, gelu, add=None, dt16=None):
    """dx, dgamma, dbeta, out16 of la_layernorm_bwd / la_layernorm_bwd_res in float64 (dgamma / dbeta: the sums alone, what the kernel ADDS
    to its destinations; out16: the exact value before its rounding, None without dt16)."""
    v, _ = _ln64(x, dy, gamma, beta, eps, gelu, add, dt16, None, None, False)
    return v["dx"], v["dgamma"], v["dbeta"], v["out16"]


def layernorm_bwd_bound64(x, dy, gamma, beta, eps, gelu, add=None, dt16=None, dgamma0=None, dbeta0=None):
    """The allowance |kernel - layernorm_bwd64| may reach per element: dict(dx, dgamma, dbeta[, out16]), float64.
       * mu, mean(g), mean(g xhat): gamma_(E + 2) mean|terms| - an E-term fp32 sum in any order (lane partials, cross-lane fold) and
         the product with the rounded 1 / E - plus the mean of the terms' own allowances;
       * x - mu: the error of mu and one rounding; var + eps: gamma_(E + 4) (var + eps) + 2 mean|x - mu| dmu + 2 u var;
       * rstd: rsqrtf is 1 ulp (2^-23 relative); the variance's error enters with |d rsqrt / dV| = rstd^3 / 2;
       * xhat = (x - mu) rstd: product rule and one rounding;
       * gelu' (erff, __expf): gelu_abs_err(z) + 0.8 dz (max |gelu''|) + 4 u |gelu'|, z = xhat gamma + beta with two roundings;
       * dx: product rule through rstd (g - s1 - xhat s2), three roundings inside, one outside, one more for ``add``;
       * out16: half an ulp of the type at |ref| + allowance (the kernel rounds ITS value) plus 2^-25, half the spacing of fp16 subnormals;
       * dgamma, dbeta: gamma_(rows + 8) (sum_r |term| + |pre-loaded value|) for the row sum in any order (atomics) plus the sum of the
         terms' allowances.
    dgamma0 / dbeta0: what the destinations held before the call (the atomics add onto it)."""
    return _ln64(x, dy, gamma, beta, eps, gelu, add, dt16, dgamma0, dbeta0, True)[1]


def layernorm_bwd_case64(x, dy, gamma, beta, eps, gelu, add=None, dt16=None, dgamma0=None, dbeta0=None):
    """(values, allowances) in one pass: dicts over dx, dgamma, dbeta, out16; dgamma / dbeta INCLUDE the pre-loaded values."""
    v, a = _ln64(x, dy, gamma, beta, eps, gelu, add, dt16, dgamma0, dbeta0, True)
    if dgamma0 is not None:
        v["dgamma"] = v["dgamma"] + dgamma0.double()
    if dbeta0 is not None:
        v["dbeta"] = v["dbeta"] + dbeta0.double()
    if dt16 is None:
        v.pop("out16")
    return v, a


def ln_scaled_rows(rows):
    """The block of rows every LayerNorm case scales by 1e-2: there eps = 1e-6 is 1 % of the variance."""
    return rows // 3, rows // 3 + max(1, rows // 8)


def ln_data(rows, e, device="cpu", seed=None):
    """x ~ N(0.3, 1) with a block of rows scaled by 1e-2, gamma = 1 + 0.3 N, beta = 0.2 N, dy ~ N(0, 1), the skip gradient ``add`` and the
    pre-loaded dgamma0 / dbeta0 ~ N(0, 1); eps = 1e-6.  Drawn on the host whatever the device: CPU and GPU tests see the same numbers."""
    g = torch.Generator().manual_seed(rows * 31 + e if seed is None else seed)
    x = 0.3 + torch.randn(rows, e, generator=g)
    lo, hi = ln_scaled_rows(rows)
    x[lo:hi] *= 1e-2
    d = dict(x=x, dy=torch.randn(rows, e, generator=g), gamma=1.0 + 0.3 * torch.randn(e, generator=g), beta=0.2 * torch.randn(e, generator=g),
             add=torch.randn(rows, e, generator=g), dgamma0=torch.randn(e, generator=g), dbeta0=torch.randn(e, generator=g))
    d = {k: v.to(device) for k, v in d.items()}
    d["eps"] = 1e-6
    return d


# ---- GELU backward on a 16-bit pre-activation --------------------------------------------------------------------------------------
def gelu_bwd64(pre16, dh):
    """dpre = dh gelu'(pre) of la_gelu_bwd16 in float64 (erf form)."""
    return dh.double() * gelu_grad64(pre16.double())


def gelu_bwd_bound64(pre16, dh, dt16=None):
    """|dh| gelu_abs_err(pre) (erff / __expf, as in layernorm_bwd_bound64; the 16-bit pre-activation converts exactly) + 4 u |gelu'| |dh| for
    the roundings that assemble gelu' + u |ref| for the product; the 16-bit output adds half an ulp at |ref| + allowance (+ 2^-25 for fp16)."""
    p, d = pre16.double(), dh.double()
    ref = d * gelu_grad64(p)
    al = d.abs() * gelu_abs_err(p) + 5.0 * U * ref.abs()
    if dt16 is not None:
        al = al + HALF_ULP[dt16] * (ref.abs() + al) + (2.0 ** -25 if dt16 == torch.float16 else 0.0)
    return al


def gelu_data(n, dt, device="cpu"):
    g = torch.Generator().manual_seed(n)
    return (1.5 * torch.randn(n, generator=g)).to(dt).to(device), torch.randn(n, generator=g).to(device)


# ---- AdamW --------------------------------------------------------------------------------------------------------------------------
def _adamw64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, bound):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gi = g * grad_scale
    decay = 1.0 - lr * wd
    p0 = p * decay
    mi = m + (gi - m) * (1.0 - b1)
    vi = v * b2 + (1.0 - b2) * gi * gi
    pw1, pw2 = b1 ** step, b2 ** step
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    bc2s = math.sqrt(bc2)
    root = vi.sqrt()
    r = root / bc2s
    denom = r + eps
    q = mi / denom
    ss = lr / bc1
    upd = ss * q
    pn = p0 - upd
    if not bound:
        return (pn, mi, vi), None
    U = 2.0 * U24       # per fp32 operation: twice the worst case of one correct rounding - the worst case itself IS reached among a million elements
    dgi = U * gi.abs()
    dp0 = 3.0 * U * p0.abs()                                  # lr wd, 1 - it, the product
    # (gi - m) (1 - b1): gi's rounding, the difference, 1 - b1, the product: relative to |gi - m| (1 - b1); then the sum
    dmi = (dgi + 3.0 * U * (gi - m).abs()) * (1.0 - b1) + U * mi.abs()
    # v b2; ((1 - b2) gi) gi: 1 - b2, two products, gi's rounding twice; the sum
    dvi = U * (v * b2).abs() + 5.0 * U * (1.0 - b2) * gi * gi + U * vi.abs()
    dbc1 = POW_REL * pw1 + U * bc1                            # 1 - powf(b1, step)
    dbc2 = POW_REL * pw2 + U * bc2
    dbc2s = 0.5 * dbc2 / bc2s + U * bc2s                      # sqrtf is correctly rounded
    droot = 0.5 * dvi / root.clamp_min(1e-300) + U * root
    dr = droot / bc2s + r * (dbc2s / bc2s) + U * r
    dden = dr + U * denom
    dq = dmi / denom + q.abs() * dden / denom + U * q.abs()
    dss = ss * (dbc1 / bc1 + U)
    dupd = ss * dq + q.abs() * dss + U * upd.abs()
    dpn = dp0 + dupd + U * pn.abs()
    return (pn, mi, vi), (dpn, dmi, dvi)


def adamw64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """New p, exp_avg, exp_avg_sq of one la_adamw_step in float64 - torch.optim.AdamW's single-tensor update on grad_scale g:
    p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g^2;  p -= (lr / (1 - b1^step)) m / (sqrt(v) / sqrt(1 - b2^step) + eps).
    The scalars are used as given: hand it the fp32-rounded values (``f32``) the kernel receives."""
    return _adamw64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, False)[0]


def adamw_bound64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """Allowances of (p, exp_avg, exp_avg_sq): 2 u per fp32 operation of adamw_kernel, each relative to its own result, carried through
    the update by the product / quotient rule; the bias corrections 1 - powf(b, step) carry powf's error (2 ulp of b^step - at step 1 and
    b2 = 0.999 that is 2.4e-4 of 1 - b2^step: the largest term of p's allowance), sqrtf is correctly rounded."""
    return _adamw64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, True)[1]


def adamw_data(n, device="cpu"):
    """Parameters, first / second moment state and three gradients (steps 1, 2, 1000)."""
    g = torch.Generator().manual_seed(n % 1000 + 7)
    p, m = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v = (0.1 * torch.randn(n, generator=g)) ** 2 + 1e-4
    grads = [4.0 * torch.randn(n, generator=g) for _ in range(3)]
    return p.to(device), m.to(device), v.to(device), [t.to(device) for t in grads]


ADAMW_HYPER = dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), wd=f32(0.01), grad_scale=f32(0.25))
ADAMW_STEPS = (1, 2, 1000)


# ---- integer-exact references -------------------------------------------------------------------------------------------------------
def ints(*shape, seed, reduce, dtype=torch.float32, device="cuda", factor=INT_HI):
    """Integers in [-8, 8] (helpers.rint's draw) as ``dtype`` - exact in fp32, fp16 and bf16 - for a reduction over ``reduce`` terms, each
    the product with a factor of magnitude <= ``factor`` (8: another such integer; 1: a plain sum): every partial sum, onto a pre-loaded
    integer of the same range, stays below 2^24 and is therefore exact in fp32 in any order."""
    assert reduce * INT_HI * factor + INT_HI < 2 ** 24, f"a reduction over {reduce} rows is not exact in fp32"
    if torch.device(device).type == "cuda":
        from tests.helpers import rint
        return rint(*shape, seed=seed).to(dtype)
    g = torch.Generator().manual_seed(seed)
    return torch.randint(INT_LO, INT_HI + 1, shape, generator=g).float().to(dtype)


def as_slice(t, off, extra, fill=NAN):
    """t as the column slice [off, off + cols) of a parent ``extra`` columns wider, the rest of it ``fill``."""
    rows, cols = t.shape
    parent = torch.full((rows, cols + extra), fill, dtype=t.dtype, device=t.device)
    parent[:, off:off + cols] = t
    return parent[:, off:off + cols]


def flat_offset(t, off):
    """A contiguous copy of t that starts ``off`` elements into its buffer (off its 16-byte alignment)."""
    buf = torch.empty(t.numel() + off + 8, dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _exact32(t64):
    t = t64.float()
    assert bool((t.double() == t64).all()) and float(t64.abs().max()) < 2 ** 24
    return t


def gemm_tn_exact(dy, x, dw0, db0=None):
    """dw0 + dy^T x and db0 + colsum(dy), exact (integer inputs)."""
    dw = _exact32(dw0.double() + dy.double().t() @ x.double())
    return dw, (_exact32(db0.double() + dy.double().sum(0)) if db0 is not None else None)


def gemm_tn16_exact(dy, x, buf0, db0=None, gsize=0, gstride=0):
    """la_gemm_tn16 onto the pre-loaded buffer buf0 [rows, K]: product row n lands in row (n // gsize) gstride + n % gsize (gsize = 0: n)."""
    n = dy.shape[1]
    prod = dy.double().t() @ x.double()
    rows = torch.arange(n, device=dy.device)
    if gsize:
        rows = (rows // gsize) * gstride + rows % gsize
    out = buf0.double().clone()
    out[rows] += prod
    return _exact32(out), (_exact32(db0.double() + dy.double().sum(0)) if db0 is not None else None)


def colsum_exact(dy, out0):
    return _exact32(out0.double() + dy.double().sum(0))


def transpose16_exact(src, dt, rp, colsum0=None):
    """dst [C, Rp] = src^T as ``dt`` with zeros behind row R, and colsum0 + the column sums of src."""
    r, c = src.shape
    dst = torch.zeros(c, rp, dtype=dt, device=src.device)
    dst[:, :r] = src.t().to(dt)
    assert torch.equal(dst[:, :r].double(), src.t().double())
    return dst, (_exact32(colsum0.double() + src.double().sum(0)) if colsum0 is not None else None)


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def check(got, ref, allowance):
    """(max err / allowance, index of the first element beyond its allowance or None).  A non-finite value in ``got`` is a failure:
    its ratio is inf."""
    got = got.double()
    ref = ref.to(got.device)
    al = allowance if torch.is_tensor(allowance) else torch.full_like(ref, float(allowance))
    ratio = (got - ref).abs() / al.to(got.device).clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    if ratio.numel() == 0:
        return 0.0, None
    over = torch.nonzero((ratio > 1.0).reshape(-1))
    first = None
    if over.numel():
        first = tuple(int(i) for i in torch.unravel_index(over[0, 0], ratio.shape)) if ratio.dim() else ()
    return float(ratio.max()), first
