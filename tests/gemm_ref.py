"""The contract of la_gemm in float64, its derived error allowance, and the harness that checks one call between guards.

Plain torch, no device code: everything here runs on CPU and GPU tensors alike.  ``gemm_ref64`` is the executable form of the header
comment of LaGemmEpilogue (include/la_hip.h): a new epilogue field or kernel family is written down HERE (and as a row of
tests/test_gemm_plan_cpu.py::TABLE) first.  ``gemm_bound64`` is the per-element allowance - every term derived, none measured.
``check_gemm_call`` runs one call with every operand and output as a view inside a larger arena (NaN around inputs, a sentinel
around outputs, a pad on every leading dimension) and asserts (a) the planned family, (b) the element-wise allowance,
(c) the suite's max-norm tolerance, (d) untouched pads / guards / unwritten rows, (e) in-place streams untouched behind row M; or,
for a call la_gemm must refuse, (r) that la_gemm_plan and la_gemm both raise the stated message and write nothing.

amap = LA_MAP_CONV3X3 is not specified here: test_implicit_3x3_convolution_on_padded_plane_pairs_equals_im2col owns that layout.
"""
import math

import torch

ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD = 0, 1, 2, 3
MAP_NONE, MAP_GROUP, MAP_WINDOW_MERGE, MAP_CONVT2X2, MAP_WINDOW_PART = 0, 1, 2, 3, 4

U24, U23 = 2.0 ** -24, 2.0 ** -23
SENT = -3.0e4                    # exact in fp16, bf16 and fp32; no output of the suite's inputs comes near it
NAN = float("nan")
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
FP16_MAX = 65504.0
TOL16 = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}       # the max-norm tolerances of tests/test_ops_gpu.py, assertion (c)
TOL32 = {torch.float16: 1e-3, torch.bfloat16: 4e-3, torch.float32: 2e-5}
# elements of each buffer's own type.  ldr, ld32 and ld16 differ from one another (a swapped output / residual leading dimension cannot
# cancel); lda and ldaux share 8, which no kernel can confuse: one is a K-wide input, the other an N-wide output plane
PADS = dict(lda=8, ldw=16, ldr=12, ld32=4, ld16=24, ldaux=8)
FRONT_IN, BACK_IN, FRONT_OUT, BACK_OUT = 64, 64, 8, 256       # guard rows around inputs / outputs
CHUNK = 8192                                                   # reference rows per step: < 1 GiB of float64 at N = 3072

_DEFAULTS = dict(bias=None, res=None, res_mod=0, out32=None, out16=None, act=ACT_NONE, map=MAP_NONE, p=(0, 0, 0, 0, 0), vt=None, vt_col0=0, vt_T=0,
                 vt_Tpad=0, vt_hd=64, vt_heads=0, vt_ws=0, amap=MAP_NONE, a_kmod=0, ksplit=0, aux16=None, nstat_out=None, rvec=None, rvec_rpg=0,
                 nstat_in=None, ncol=None, ldr=None, ld32=None, ld16=None, ldaux=None)


def _epi(epilogue):
    unknown = set(epilogue) - set(_DEFAULTS)
    assert not unknown, f"not a keyword of _lib._gemm_epilogue: {sorted(unknown)}"
    return dict(_DEFAULTS, **epilogue)


def map_rows(mode, p, r):
    """Destination row of row ``r`` (long tensor) under LaGemmEpilogue.map / amap; -1 = dropped.  For LA_MAP_CONVT2X2 the row of (ky, kx) =
    (0, 0): the column adds ky * 2 W + kx."""
    p0, p1, p2, p3, p4 = p
    if mode == MAP_GROUP:
        return (r // p0) * p1 + r % p0 + p2
    if mode == MAP_WINDOW_MERGE:
        ws, nwy, nwx, H, W = p
        tok, win = r % (ws * ws), r // (ws * ws)
        wx, wy, b = win % nwx, (win // nwx) % nwy, win // (nwx * nwy)
        y, x = wy * ws + tok // ws, wx * ws + tok % ws
        return torch.where((y < H) & (x < W), (b * H + y) * W + x, torch.full_like(r, -1))
    if mode == MAP_WINDOW_PART:
        ws, nwy, nwx, H, W = p
        x, y, b = r % W, (r // W) % H, r // (W * H)
        return ((b * nwy + y // ws) * nwx + x // ws) * ws * ws + (y % ws) * ws + x % ws
    if mode == MAP_CONVT2X2:
        W, H = p0, p1
        x, y, b = r % W, (r // W) % H, r // (W * H)
        return (b * 2 * H + 2 * y) * (2 * W) + 2 * x
    return r


def dest_rows(m, epilogue):
    """Rows an output of this call needs: 1 + the largest destination row."""
    e = _epi(epilogue)
    d = map_rows(e["map"], e["p"], torch.arange(m))
    top = int(d.max()) + 1
    return top + 2 * e["p"][0] + 1 if e["map"] == MAP_CONVT2X2 else top


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_abs_err(x):
    """Allowance of one GELU evaluation at x, from the figures la_common.h states for its three forms: libm erff (gelu_erf, line 84),
    Abramowitz-Stegun erf with |err| < 1.5e-7 (gelu_erf_fast, line 86: 0.5 |x| 1.5e-7 < 2e-7 |x|) and the packed polynomial
    (gelu_erf_pk, line 102: 1.6e-6 on |x| <= 1, 3.1e-6 on <= 2, 4.9e-6 on <= 3, 1.4e-5 on <= 4, 4.6e-5 beyond).  The largest holds for
    every family, whichever form its epilogue uses."""
    ax = x.abs()
    pk = torch.full_like(ax, 4.6e-5)
    for lim, v in ((4.0, 1.4e-5), (3.0, 4.9e-6), (2.0, 3.1e-6), (1.0, 1.6e-6)):
        pk = torch.where(ax <= lim, torch.full_like(ax, v), pk)
    return torch.maximum(2e-7 * ax, pk)


GELU_LIPSCHITZ = 1.13           # max |gelu'| = Phi(x) + x phi(x) at x = sqrt 2: 1.129


def _rows(a, w, m, n, k, r0, r1, e, cdt, bound):
    """GEMM rows r0 .. r1 of the call: values (and allowances when ``bound``) in ``cdt``, laid out [R, G, C] with G = 4, C = cout under
    LA_MAP_CONVT2X2 (the four (ky, kx) destinations of a row) and G = 1, C = N otherwise, plus the destination row of every [R, G]."""
    dev = a.device
    r = torch.arange(r0, r1, device=dev)
    R = r1 - r0
    akm = e["a_kmod"]
    ka = akm or k
    src = map_rows(e["amap"], e["p"], r) if e["amap"] else r
    A = a[src][:, :ka].to(cdt)
    W = w[:n, :k].to(cdt)
    if akm:                                         # the A columns repeat with period a_kmod: A . (sum of the W planes)^T
        kk = torch.arange(k, device=dev) % akm
        Wd = torch.zeros(n, akm, dtype=cdt, device=dev).index_add_(1, kk, W)
        Wa = torch.zeros(n, akm, dtype=cdt, device=dev).index_add_(1, kk, W.abs())
    else:
        Wd, Wa = W, W.abs()
    acc = A @ Wd.t()
    convt = e["map"] == MAP_CONVT2X2
    G, C = (4, e["p"][2]) if convt else (1, n)
    d0 = map_rows(e["map"], e["p"], r)
    if convt:
        Wg = e["p"][0]
        drow = d0[:, None] + torch.tensor([0, 1, 2 * Wg, 2 * Wg + 1], device=dev)[None, :]
    else:
        drow = d0[:, None]
    dsafe = drow.clamp_min(0)
    shape = (R, G, C)
    acc = acc.view(shape)
    zero = torch.zeros((), dtype=cdt, device=dev)
    bias = e["bias"].to(cdt)[:C].view(1, 1, C) if e["bias"] is not None else zero
    out = {"drow": drow}
    val, allow = {}, {}
    if bound:
        absacc = (A.abs() @ Wa.t()).view(shape)
        acc_allow = (k + 8) * U23 * absacc
    # ---- what is added to the product before the activation
    if e["nstat_in"] is not None:
        mean, rstd = e["nstat_in"].view(-1, 2)[r, 0].to(cdt).view(R, 1, 1), e["nstat_in"].view(-1, 2)[r, 1].to(cdt).view(R, 1, 1)
        ncol = e["ncol"].to(cdt)[:n].view(1, 1, n)
        pre = rstd * (acc - mean * ncol) + bias
        if bound:
            acc_allow = rstd.abs() * acc_allow
            epi = 4 * U24 * ((rstd * acc).abs() + (rstd * mean * ncol).abs() + bias.abs() + pre.abs())
    elif e["ksplit"]:
        o0 = e["out32"][dsafe.view(-1)][:, :C].to(cdt).view(shape)
        pre = o0 + acc
        if bound:
            acc_allow = acc_allow + max(1, k // 128) * U23 * (o0.abs() + absacc)
            epi = torch.zeros_like(pre)
    else:
        pre = acc + bias
        if bound:
            epi = 4 * U24 * (pre.abs() + bias.abs())
    # ---- activation
    act = e["act"]
    if act == ACT_GELU:
        x = gelu64(pre)
        if bound:
            acc_allow = GELU_LIPSCHITZ * acc_allow + gelu_abs_err(pre) + 4 * U24 * x.abs()
    elif act == ACT_RELU:
        x = torch.relu(pre)
    elif act == ACT_GELU_BWD:
        av = e["aux16"][r][:, :n].to(cdt).view(shape)
        x = pre * gelu_grad64(av)
        if bound:
            acc_allow = GELU_LIPSCHITZ * acc_allow + pre.abs() * gelu_abs_err(av) + 4 * U24 * x.abs()
    else:
        x = pre
    # ---- residual, group vector, the in-place plane pair
    inplace = e["nstat_out"] is not None and e["out32"] is None and e["res"] is None
    if e["res"] is not None:
        ri = dsafe % e["res_mod"] if e["res_mod"] else dsafe
        rs = e["res"][ri.view(-1)][:, :C].to(cdt).view(shape)
        x = x + rs
        if bound:
            epi = epi + 4 * U24 * rs.abs()
    if e["rvec"] is not None:
        rv = e["rvec"].view(-1, n)[r // e["rvec_rpg"]].to(cdt).view(shape)
        x = x + rv
        if bound:
            epi = epi + 4 * U24 * rv.abs()
    if inplace:
        s0 = (e["out16"][r][:, :n].to(cdt) + e["aux16"][r][:, :n].to(cdt)).view(shape)
        x = x + s0
        if bound:
            epi = epi + 4 * U24 * s0.abs()
    if bound:
        al = acc_allow + epi
        allow["_base"] = al              # the fp32 side alone: what check_gemm_call reports the 16-bit rounding's share against
    # ---- outputs
    if e["out32"] is not None:
        val["out32"] = x
        if bound:
            allow["out32"] = al
    if e["out16"] is not None:
        dt16 = e["out16"].dtype
        x16 = x.clamp(-FP16_MAX, FP16_MAX) if (e["nstat_out"] is not None and dt16 == torch.float16) else x
        val["out16"] = x16
        if bound:
            allow["out16"] = al + HALF_ULP[dt16] * (x16.abs() + al) + (2.0 ** -25 if dt16 == torch.float16 else 0.0)
    if e["aux16"] is not None and act == ACT_GELU:
        dta = e["aux16"].dtype
        val["aux16"] = pre
        if bound:
            pa = (k + 8) * U23 * absacc + epi
            allow["aux16"] = pa + HALF_ULP[dta] * (pre.abs() + pa) + (2.0 ** -25 if dta == torch.float16 else 0.0)
    if e["aux16"] is not None and e["nstat_out"] is not None:
        val["pair"] = x                     # out16 + aux16: aux16 = rn16(x - out16) depends on the hi plane the kernel chose, so the SUM is checked
        if bound:
            allow["pair"] = al + 2.0 ** -21 * x.abs() + 2.0 ** -24
    if e["nstat_out"] is not None:
        xs = x.view(R, n // 64, 64)
        val["nstat_out"] = torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=2)
        if bound:
            als = al.view(R, n // 64, 64)
            allow["nstat_out"] = torch.stack([64 * U23 * xs.abs().sum(2) + als.sum(2),
                                              64 * U23 * (xs * xs).sum(2) + ((2 * xs.abs() + als) * als).sum(2)], dim=2)
    if e["vt"] is not None:
        c0 = e["vt_col0"]
        nv = n - c0
        t = d0 % e["vt_T"]
        slot = (t // e["vt_ws"]) * 16 + t % e["vt_ws"] if e["vt_ws"] > 0 else t
        base = (d0 // e["vt_T"]) * (e["vt_heads"] * e["vt_hd"] * e["vt_Tpad"]) + slot
        idx = base[:, None] + torch.arange(nv, device=dev)[None, :] * e["vt_Tpad"]
        out["vt_idx"] = torch.where(d0[:, None] >= 0, idx, torch.full_like(idx, -1))
        val["vt"] = x.view(R, n)[:, c0:]
        if bound:
            dtv = e["vt"].dtype
            allow["vt"] = (al + HALF_ULP[dtv] * (x.abs() + al) + (2.0 ** -25 if dtv == torch.float16 else 0.0)).view(R, n)[:, c0:]
        if "out16" in val:
            val["out16"] = val["out16"][:, :, :c0]
            if bound:
                allow["out16"] = allow["out16"][:, :, :c0]
    out["val"], out["allow"] = val, allow
    return out


def _full(a, w, m, n, k, epilogue, cdt, bound, chunk=CHUNK):
    e = _epi(epilogue)
    dev = a.device
    full, written = {}, {}
    for r0 in range(0, m, chunk):
        ch = _rows(a, w, m, n, k, r0, min(m, r0 + chunk), e, cdt, bound)
        src = ch["allow"] if bound else ch["val"]
        d = ch["drow"].reshape(-1)
        keep = d >= 0
        for name, v in src.items():
            if name == "_base":
                continue
            if name == "vt":
                if name not in full:
                    full[name] = torch.zeros(e["vt"].numel(), dtype=cdt, device=dev) if bound else e["vt"].to(cdt).reshape(-1).clone()
                    written[name] = torch.zeros(e["vt"].numel(), dtype=torch.bool, device=dev)
                idx = ch["vt_idx"].reshape(-1)
                ok = idx >= 0
                full[name][idx[ok]] = v.reshape(-1)[ok]
                written[name][idx[ok]] = True
                continue
            if name == "nstat_out":
                if name not in full:
                    full[name] = torch.zeros(m, n // 64, 2, dtype=cdt, device=dev)
                full[name][r0:r0 + v.shape[0]] = v
                continue
            host = e["out16"] if name == "pair" else e[name]
            if name not in full:
                full[name] = torch.zeros(host.shape, dtype=cdt, device=dev) if bound else host.to(cdt).clone()
                written[name] = torch.zeros(host.shape[0], dtype=torch.bool, device=dev)
                if name == "pair" and not bound:
                    full[name] += e["aux16"].to(cdt)
            flat = v.reshape(-1, v.shape[-1])
            full[name][d[keep], :flat.shape[1]] = flat[keep]
            written[name][d[keep]] = True
    if "vt" in full:
        full["vt"] = full["vt"].view(e["vt"].shape)
        written["vt"] = written["vt"].view(e["vt"].shape)
    full["written"] = written
    return full


def gemm_ref64(a, w, m, n, k, **epilogue):
    """What every output of ``_lib.gemm(a, w, M=m, **epilogue)`` must hold, in float64: out = map(act(A W^T + bias) + res) with
       * bias by destination column, res by (destination row % res_mod if res_mod else destination row, destination column);
       * map GROUP / WINDOW_MERGE / CONVT2X2 / WINDOW_PART on the output rows, amap WINDOW_PART on the source rows;
       * a_kmod: the columns of A repeat with that period under all K columns of W;
       * ksplit: the bare product ADDED onto what out32 held; vt: columns >= vt_col0 go transposed into vt (slots of vt_ws-wide
         windows 16 apart) and not into out16;
       * aux16: with ACT_GELU the pre-activation, with ACT_GELU_BWD read: out16 = (A W^T) gelu'(aux16);
       * nstat_out: the stream x = A W^T + bias + res + rvec[row / rvec_rpg] (out32, out16 = its rounding, saturated at the fp16 range) and
         the sums of x and x^2 over every 64 columns; without out32 / res the stream is the plane pair out16 + aux16 itself,
         read and written back (key "pair": out16 + aux16; "out16": the hi plane);
       * nstat_in: act(rstd[row] (A W^T - mean[row] ncol[col]) + bias).
    Operands are the 16-bit / fp32 tensors the kernel gets; in-place buffers (out32 under ksplit, the plane pair, aux16 under
    ACT_GELU_BWD) carry their PRE-CALL contents, and every output keeps its pre-call contents where the call does not write.
    Returns {name: float64 tensor shaped like that output, "written": {name: bool mask over its rows (vt: its elements)}}."""
    return _full(a, w, m, n, k, epilogue, torch.float64, False)


def gemm_bound64(a, w, m, n, k, **epilogue):
    """The allowance |kernel - gemm_ref64| may reach per element, float64, same keys and shapes as gemm_ref64 (0 where nothing is written).
       * accumulation: (K + 8) 2^-23 (|A| |W|^T) - the forward bound of a K-term fp32 sum in any order (16-bit products are exact in
         fp32; fp32 products round once, inside the same factor); 2^-23 and not 2^-24 per operation because the MFMA's internal
         rounding is not documented as round-to-nearest; the + 8 covers the cross-lane folds of the split-K / VALU kernels.
       * ksplit: each of at most K / 128 chunks (a chunk is at least two 64-deep k-tiles) adds 2^-23 (|out0| + |A||W|^T): one fp32
         atomic add onto a value of at most that size.
       * epilogue: 4 2^-24 (|pre| + |bias| + |res| + |rvec|): at most four fp32 roundings (bias, residual, group vector, the final
         add), each relative to a partial sum no larger than the sum of the magnitudes.
       * GELU: gelu_abs_err(x) + 4 2^-24 |gelu(x)| (the stated error of the implementation plus the roundings of x Phi(x)); the
         allowance that arrives at the activation is scaled by max |gelu'| <= 1.13.  GELU_BWD: the same with gelu' on the saved
         pre-activation, times |A W^T|.
       * 16-bit outputs: half an ulp of the type at |ref| + allowance (2^-11 fp16, 2^-8 bf16) - the kernel rounds ITS value, which
         is within the allowance of the reference - plus 2^-25, half the spacing of fp16 subnormals.
       * the plane pair out16 + aux16 as a sum: 2^-21 |x| (two fp16 planes keep ~22 bits) + 2^-24 (the lo plane's own subnormal step).
       * nstat_out: 64 2^-23 sum|x| and 64 2^-23 sum x^2 for the 64-term fp32 sums in any order, plus what the allowance of the x
         themselves moves them by (sum of allowances; sum of (2 |x| + allowance) allowance for the squares).
       * nstat_in: the accumulation allowance scaled by |rstd[row]|, epilogue term over |rstd acc|, |rstd mean ncol|, |bias|."""
    return _full(a, w, m, n, k, epilogue, torch.float64, True)


# ---------------------------------------------------------------------------------------------------------------------------------
class GemmContractError(AssertionError):
    """One or more of the assertions (a) - (e) failed; ``failed`` holds their letters."""

    def __init__(self, failed, lines, nonfinite=False):
        self.failed, self.nonfinite = set(failed), nonfinite
        super().__init__("la_gemm contract: " + "; ".join(lines))


def _arena(rows, cols, ld, dtype, dev, front, back, fill, elem_off=0):
    """A [rows, cols] view with row stride ld inside a filled arena of front + rows + back rows (+ elem_off elements of offset)."""
    total = (front + rows + back) * ld + elem_off + 8
    buf = torch.full((total,), fill, dtype=dtype, device=dev)
    view = buf.as_strided((rows, cols), (ld, 1), front * ld + elem_off)
    return buf, view


def _place_in(t, ld, elem_off=0, front=FRONT_IN, back=BACK_IN, fill=NAN):
    """Input tensor t ([rows, cols] or a vector) inside NaN: pads, and guard rows in front of and behind it."""
    if t.dim() == 1:
        buf = torch.full((t.numel() + 2 * 64,), fill, dtype=t.dtype, device=t.device)
        buf[64:64 + t.numel()] = t
        return buf[64:64 + t.numel()]
    rows, cols = t.shape
    _, view = _arena(rows, cols, ld, t.dtype, t.device, front, back, fill, elem_off)
    view.copy_(t)
    return view


def _flat_guard(t):
    """Guard elements on either side of an output without a leading dimension (vt, nstat_out): BACK_OUT of its rows."""
    return BACK_OUT * (t.numel() // t.shape[0])


def check_gemm_call(L, a, w, m, n, k, dt, epilogue, *, pads=PADS, family=None, lds=None, a_elem_off=0, label="", input_fill=NAN, refused=None):
    """Run ``L.gemm`` on guarded, padded copies of compact operands and assert the contract.

    a [source rows, a_kmod or K], w [N, K]; ``epilogue`` as for ``_lib.gemm`` with compact tensors: inputs with their values, outputs
    with their PRE-CALL contents (only read where the call works in place: out32 under ksplit, out32 passed as res as well - the SAME
    tensor object: the residual stream updated in place -, the plane pair of an in-place nstat_out; every other output starts as the
    sentinel).  pads: elements added to each leading dimension (None = compact); lds: explicit leading
    dimensions that override them (lda, ldw, ldr, ld32, ld16, ldaux); a_elem_off: elements A is shifted off its 16-byte alignment;
    input_fill: what surrounds the inputs (NaN; a finite number models the neighbours a compact, unguarded test has).
    refused: the literal text of la_gemm's error for a call it must NOT run: then L.gemm_plan and L.gemm - each called on the real
    guarded operands - must both raise a RuntimeError holding it, and no byte of any output arena may have moved (assertion (r)).
    Raises GemmContractError naming the failed assertions among (a) - (e); returns dict(family, ratio = max err / allowance, ratios = the
    same per output, share16 = the 16-bit rounding's share of the allowance at out16's worst element, plan)."""
    e = _epi(epilogue)
    pads = dict.fromkeys(PADS, 0) if pads is None else pads
    lds = lds or {}
    dev = a.device

    def ld(name, cols):
        return lds.get(name) or cols + pads[name]

    failed, lines, nonfinite = set(), [], []

    def fail(letter, text):
        failed.add(letter)
        lines.append(f"({letter}) {text}")

    akm = e["a_kmod"]
    inplace = e["nstat_out"] is not None and e["out32"] is None and e["res"] is None
    call, pre, arenas = dict(epilogue), dict(epilogue), {}
    for key in ("ldr", "ld32", "ld16", "ldaux"):
        call.pop(key, None), pre.pop(key, None)
    av = _place_in(a, ld("lda", a.shape[1]), a_elem_off, fill=input_fill)
    wv = _place_in(w, ld("ldw", k), fill=input_fill)
    for name in ("bias", "rvec", "nstat_in", "ncol"):
        if e[name] is not None:
            call[name] = _place_in(e[name].reshape(-1), 0, fill=input_fill).view(e[name].shape)
    alias = e["res"] is not None and e["res"] is e["out32"]          # the residual stream updated in place: res and out32 are one buffer
    stream32 = bool(e["ksplit"]) or alias
    if e["res"] is not None and not alias:
        call["res"] = _place_in(e["res"], ld("ldr", e["res"].shape[1]), fill=input_fill)
    if e["aux16"] is not None and e["act"] == ACT_GELU_BWD:
        call["aux16"] = _place_in(e["aux16"], ld("ldaux", n), fill=input_fill)
    for name, ldn in (("out32", "ld32"), ("out16", "ld16"), ("aux16", "ldaux")):
        t = e[name]
        if t is None or (name == "aux16" and e["act"] == ACT_GELU_BWD):
            continue
        buf, view = _arena(t.shape[0], t.shape[1], ld(ldn, t.shape[1]), t.dtype, dev, FRONT_OUT, BACK_OUT, SENT)
        if (name == "out32" and stream32) or (inplace and name != "out32"):
            view.copy_(t)
        else:
            pre[name] = torch.full_like(t, SENT)
        arenas[name] = (buf, view)
        call[name] = view
        if name == "out32" and alias:
            call["res"] = view
    for name in ("vt", "nstat_out"):
        t = e[name]
        if t is not None:
            g = _flat_guard(t)
            buf = torch.full((t.numel() + 2 * g,), SENT, dtype=t.dtype, device=dev)
            view = buf[g:g + t.numel()].view(t.shape)
            pre[name] = torch.full_like(t, SENT)
            arenas[name] = (buf, view)
            call[name] = view
    if refused is not None:
        before = {name: buf.clone() for name, (buf, _) in arenas.items()}
        for what, fn in (("la_gemm_plan", lambda: L.gemm_plan(av, av.stride(0), wv, wv.stride(0), m, n, k, dt, 0, **call)),
                         ("la_gemm", lambda: L.gemm(av, wv, M=m, **call))):
            try:
                fn()
            except RuntimeError as err:
                if not (str(err).startswith(what + " failed") and refused in str(err)):
                    fail("r", f"{what} raised another error than '{refused}': {err}")
            else:
                fail("r", f"{what} accepted a call it must refuse with '{refused}'")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        for name, (buf, _) in arenas.items():
            if not torch.equal(buf.view(torch.uint8), before[name].view(torch.uint8)):
                fail("r", f"{name}: the refused call wrote to it")
        if failed:
            raise GemmContractError(failed, [f"{label} refusal"] + lines)
        return dict(refused=refused)
    # ---- (a) the planned family of exactly this call
    plan = L.gemm_plan(av, av.stride(0), wv, wv.stride(0), m, n, k, dt, 0, **call)
    fam = L.GEMM_KERNELS[plan.kernel]
    if family is not None and fam != family:
        fail("a", f"la_gemm_plan names {fam}, expected {family}")
    L.gemm(av, wv, M=m, **call)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    # ---- (b), (c) element by element against the float64 contract, in row chunks
    worst, ratios, share16 = 0.0, {}, 0.0
    norm = {}
    written = {name: torch.zeros(arenas[name][1].shape[0], dtype=torch.bool, device=dev) for name in ("out32", "out16", "aux16") if name in arenas}
    if "vt" in arenas:
        written["vt"] = torch.zeros(e["vt"].numel(), dtype=torch.bool, device=dev)
    ep = _epi(pre)
    for r0 in range(0, m, CHUNK):
        ch = _rows(a, w, m, n, k, r0, min(m, r0 + CHUNK), ep, torch.float64, True)
        d = ch["drow"].reshape(-1)
        keep = d >= 0
        for name, ref in ch["val"].items():
            al = ch["allow"][name]
            if name == "vt":
                idx = ch["vt_idx"].reshape(-1)
                ok = idx >= 0
                got = arenas["vt"][1].reshape(-1)[idx[ok]].double()
                ref, al = ref.reshape(-1)[ok], al.reshape(-1)[ok]
                written["vt"][idx[ok]] = True
            elif name == "nstat_out":
                got = arenas[name][1].view(m, n // 64, 2)[r0:r0 + ref.shape[0]].double()
            else:
                ref, al = ref.reshape(-1, ref.shape[-1])[keep], al.reshape(-1, al.shape[-1])[keep]
                if name == "pair":
                    got = arenas["out16"][1][d[keep]][:, :n].double() + arenas["aux16"][1][d[keep]][:, :n].double()
                else:
                    got = arenas[name][1][d[keep]][:, :ref.shape[1]].double()
                    written[name][d[keep]] = True
                    if name == "out16" and "aux16" in arenas:
                        written["aux16"][d[keep]] = True
            if not bool(torch.isfinite(got).all()):
                fail("b", f"{name}: non-finite values in rows {r0}..")
                nonfinite.append(name)
                continue
            err = (got - ref).abs()
            over = err > al
            ratio = float((err / al.clamp_min(1e-300)).max()) if err.numel() else 0.0
            if name == "out16" and ratio > ratios.get(name, 0.0):       # how much of the allowance at the worst element is the output rounding
                i = int((err / al.clamp_min(1e-300)).reshape(-1).argmax())
                base = ch["allow"]["_base"].reshape(-1, ch["allow"]["_base"].shape[-1])[keep][:, :ref.shape[1]]
                share16 = 1.0 - float(base.reshape(-1)[i] / al.reshape(-1)[i])
            ratios[name] = max(ratios.get(name, 0.0), ratio)
            worst = max(worst, ratio)
            if bool(over.any()):
                i = int(torch.nonzero(over.reshape(-1))[0])
                fail("b", f"{name}: {int(over.sum())} elements beyond the allowance from row chunk {r0} (first: got {float(got.reshape(-1)[i]):.7g} "
                          f"ref {float(ref.reshape(-1)[i]):.7g} allowance {float(al.reshape(-1)[i]):.3g}), max err / allowance {ratio:.3g}")
            if name in ("out32", "out16", "vt"):
                nm = norm.setdefault(name, [0.0, 0.0])
                if err.numel():
                    nm[0], nm[1] = max(nm[0], float(err.max())), max(nm[1], float(ref.abs().max()))
    for name, (emax, rmax) in norm.items():
        tol = TOL32[a.dtype] if name == "out32" else TOL16[arenas[name][1].dtype]
        if emax > tol * max(rmax, 1e-20):
            fail("c", f"{name}: max-norm error {emax / max(rmax, 1e-20):.3g} above {tol:g}")
    # ---- (d), (e) nothing outside the written elements moved
    for name, (buf, view) in arenas.items():
        sent = torch.tensor(SENT, dtype=buf.dtype, device=dev)
        if name in ("vt", "nstat_out"):
            g = _flat_guard(view)
            if not bool((buf[:g] == sent).all() and (buf[g + view.numel():] == sent).all()):
                fail("d", f"{name}: guard elements overwritten")
            if name == "vt" and not bool((view.reshape(-1)[~written["vt"]] == sent).all()):
                fail("d", f"{name}: slots no token maps to were written")
            continue
        rows, cols = view.shape
        ldv = view.stride(0)
        body0 = FRONT_OUT * ldv
        grid = buf[body0:body0 + rows * ldv].view(rows, ldv)
        stream = (name == "out32" and stream32) or (inplace and name != "out32")
        if not bool((buf[:body0] == sent).all()):
            fail("d", f"{name}: guard rows in front of the output overwritten")
        if not bool((buf[body0 + rows * ldv:] == sent).all()):
            fail("e" if stream else "d", f"{name}: rows behind the output overwritten")
        if ldv > cols and not bool((grid[:, cols:] == sent).all()):
            fail("d", f"{name}: pad columns overwritten")
        wcols = e["vt_col0"] if (name == "out16" and e["vt"] is not None) else cols
        if wcols < cols and not bool((view[:, wcols:] == sent).all()):
            fail("d", f"{name}: V^T columns written to out16")
        if stream:
            if not bool(torch.equal(view[~written[name]], pre[name][~written[name]])):
                fail("e", f"{name}: in-place rows the call does not own changed")
        elif not bool((view[~written[name]] == sent).all()):
            fail("d", f"{name}: rows the map never writes were written")
    if failed:
        raise GemmContractError(failed, [f"{label} {fam}"] + lines, bool(nonfinite))
    return dict(family=fam, ratio=worst, ratios=ratios, share16=share16, plan=plan)
