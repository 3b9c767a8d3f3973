"""GPU: the attention kernels on scores that MOVE the running softmax maximum (tests/softmax_profiles.py: stairs, creep, tail spike,
front spike, offset, bias-driven), against plain fp64 attention on the same 16-bit (or e4m3) values.  All three copies of the deferred
online softmax of csrc/attn_enc.hip - attn_fwd_kernel modes 0 - 5 with both head widths and the lse / cspart / row-major-V instances,
attn_window_kernel, attn_fwd_fp8_kernel - both backward kernels behind the stored lse, and the fp32 softmax kernels that merge partial
(max, sum, acc) states.  tests/test_softmax_profiles_cpu.py shows that these inputs have the profiles they are named after and that
faults in the rescale step, invisible on N(0, 1) inputs, are caught on them.

Bounds are the suite's own (TOL16 of tests/test_ops_gpu.py, the lse / gradient bounds of tests/test_encoder_train_gpu.py and
tests/test_sam_train_gpu.py, the fp8 bound of test_fp8_qk_attention_matches_torch_on_e4m3_rounded_operands); besides the max-norm every
(query row, head) is held to 4 x the bound relative to THAT row's output maximum.  Measured figures: profiles/attention_conditioning.md."""
import math

import pytest
import torch

from tests import softmax_profiles as SP
from tests.helpers import L, NAN

pytestmark = pytest.mark.gpu

FWD = SP.forward_cases()
BWD = SP.backward_cases()


def fam(cases, name):
    return [c for c in cases if c[0] == name]


def on_gpu(p):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in p.items()}


def built(case):
    """-> (the input on the device, its fp64 reference O as rows [b t, E], lse [b heads, t] in log2 units)"""
    _, kind, t, g, hd, dt, order, b, heads = case
    p = on_gpu(SP.build(kind, t, hd, dt, SP.tile_map(order, t, g), b=b, heads=heads, g=g))
    o, lse = SP.attention(p["q"], p["k"], p["v"], p["scale"], g, p.get("tabh"), p.get("tabw"))
    return p, SP.rows_of(o), lse.reshape(b * heads, t)


def check_rows(tag, got, ref_rows, heads, tol):
    """max-norm relative to the output's maximum, and every (row, head) relative to its own maximum (4 x)."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    err = (got - ref_rows).abs()
    e_all = float(err.max() / ref_rows.abs().max())
    rows = ref_rows.shape[0]
    e_row = float((err.view(rows, heads, -1).amax(-1) / ref_rows.abs().view(rows, heads, -1).amax(-1)).max())
    print(f"[cond] {tag}: out {e_all:.2e} (bound {tol:.1e})  worst row {e_row:.2e} (bound {4 * tol:.1e})")
    assert e_all <= tol, (tag, e_all)
    assert e_row <= 4 * tol, (tag, e_row)


def check_lse(tag, lse, ref_lse, t):
    err = float((lse[:, :t].double() - ref_lse).abs().max())
    print(f"[cond] {tag}: lse {err:.2e} (bound {SP.TOL_LSE:.1e})")
    assert err <= SP.TOL_LSE, (tag, err)
    assert bool(torch.isnan(lse[:, t:]).all()), f"{tag}: lse entries beyond T were written"


def v_transposed(L, qkv, b, heads, t, hd, tpad):
    e = heads * hd
    vt = torch.empty(b * heads, hd, tpad, dtype=qkv.dtype, device="cuda")
    L.head_transpose(qkv, 2 * e, b, heads * (hd // 64), t, tpad, vt)
    return vt


def v_slot_order(qkv, b, heads, g, hd, tpad):
    e = heads * hd
    vt = torch.zeros(b * heads, hd, tpad, dtype=qkv.dtype, device="cuda")
    vt.view(b, heads, hd, tpad)[..., :16 * g].unflatten(-1, (g, 16))[..., :g] = qkv[:, 2 * e:].view(b, g, g, heads, hd).permute(0, 3, 4, 1, 2)
    return vt


# =========================================================================================================================
# forward: attn_fwd_kernel MODE 0 with its lse / cspart / row-major-V instances
# =========================================================================================================================
@pytest.mark.parametrize("case", fam(FWD, "plain"), ids=SP.case_id)
def test_plain_attention_all_forms(L, case):
    """LA_ATTN_PLAIN through la_attn_fwd, la_attn_fwd_rows (no V^T copy), la_attn_fwd_cs (column sums of the stored rows) and
    la_attn_fwd_lse; head width 64 and 128 (the profile dimension in the upper 64 columns)."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, ref_lse = built(case)
    dtype, tol, tag = SP.TORCH_DT[dt], SP.TOL16[dt], SP.case_id(case)
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd(qkv, vt, out, None, None, b, heads, t, tpad, 0, e, sc, L.ATTN_PLAIN)
    check_rows(tag + " la_attn_fwd", out, ref, heads, tol)
    out_r = torch.full_like(out, NAN)
    L.attn_fwd_rows(qkv, out_r, b, heads, t, tpad, 0, e, sc, L.ATTN_PLAIN)
    check_rows(tag + " la_attn_fwd_rows", out_r, ref, heads, tol)
    nq = (t + 127) // 128
    out_c = torch.full_like(out, NAN)
    part = torch.full((b * nq, e), NAN, device="cuda")
    L.attn_fwd_cs(qkv, vt, out_c, None, None, b, heads, t, tpad, 0, e, sc, L.ATTN_PLAIN, part)
    check_rows(tag + " la_attn_fwd_cs", out_c, ref, heads, tol)
    stored = torch.zeros(b, nq * 128, e, dtype=torch.float64, device="cuda")
    stored[:, :t] = out_c.double().view(b, t, e)
    want = stored.view(b * nq, 128, e).sum(1)
    slack = 128 * 2.0 ** -24 * stored.abs().view(b * nq, 128, e).sum(1) + 1e-30        # 128 fp32 additions of exactly-held 16-bit values
    cs_err = float(((part.double() - want).abs() / slack).max())
    print(f"[cond] {tag} la_attn_fwd_cs: column sums at {cs_err:.2f} of the fp32 summation bound")
    assert cs_err <= 1.0
    out_l = torch.full_like(out, NAN)
    lse = torch.full((b * heads, tpad), NAN, device="cuda")
    L.attn_fwd_lse(qkv, vt, out_l, lse, b, heads, t, tpad, e, sc)
    check_rows(tag + " la_attn_fwd_lse", out_l, ref, heads, tol)
    check_lse(tag + " la_attn_fwd_lse", lse, ref_lse, t)
    if kind.startswith("offset"):
        base = dict(p, q=p["q"].clone())
        base["q"][..., SP.profile_channel(hd)[1]] = 0.0
        _, lse0 = SP.attention(base["q"], base["k"], base["v"], sc)
        shift = float((ref_lse - lse0.reshape(b * heads, t)).mean())
        assert abs(shift - p["offset_log2"]) <= 1e-9 and abs(shift) >= 64.0


# =========================================================================================================================
# forward: rel-pos modes 1 - 4 and attn_window_kernel
# =========================================================================================================================
@pytest.mark.parametrize("case", fam(FWD, "terms"), ids=SP.case_id)
def test_relpos_attention_with_terms_from_la_relpos_terms(L, case):
    """MODE 1 (generic grid, terms from la_relpos_terms in per-wave LDS tables): la_attn_fwd and la_attn_fwd_relpos_lse."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, ref_lse = built(case)
    dtype, tol, tag = SP.TORCH_DT[dt], SP.TOL16[dt], SP.case_id(case)
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    tabh, tabw = p["tabh"].to(dtype), p["tabw"].to(dtype)
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    relh = torch.full((b * heads, t, g), NAN, device="cuda")
    relw = torch.full_like(relh, NAN)
    L.relpos_terms(qkv, b, heads, g, e, tabh, tabw, relh, relw)
    rh64, rw64 = SP.relpos_terms(p["q"], p["tabh"], p["tabw"], g)
    assert float((relh.double() - rh64).abs().max()) <= 1e-5 * max(1.0, float(rh64.abs().max()))
    assert float((relw.double() - rw64).abs().max()) <= 1e-5 * max(1.0, float(rw64.abs().max()))
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd(qkv, vt, out, relh, relw, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS)
    check_rows(tag + " la_attn_fwd", out, ref, heads, tol)
    out_l = torch.full_like(out, NAN)
    lse = torch.full((b * heads, tpad), NAN, device="cuda")
    L.attn_fwd_relpos_lse(qkv, vt, out_l, relh, relw, lse, b, heads, t, tpad, g, e, sc)
    check_rows(tag + " la_attn_fwd_relpos_lse", out_l, ref, heads, tol)
    check_lse(tag + " la_attn_fwd_relpos_lse", lse, ref_lse, t)


@pytest.mark.parametrize("case", fam(FWD, "tables"), ids=SP.case_id)
def test_window_grids_with_the_terms_computed_in_the_kernel(L, case):
    """LA_ATTN_RELPOS with the 16-bit tables and G <= 16: head width 64 runs attn_window_kernel (one wave per query tile, operands
    straight from global memory), head width 128 the LDS-staged MODE 3 of attn_fwd_kernel."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, _ = built(case)
    dtype, tol, tag = SP.TORCH_DT[dt], SP.TOL16[dt], SP.case_id(case)
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd(qkv, vt, out, None, None, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS, tabh=p["tabh"].to(dtype), tabw=p["tabw"].to(dtype))
    check_rows(tag + " la_attn_fwd", out, ref, heads, tol)


@pytest.mark.parametrize("case", fam(FWD, "global"), ids=SP.case_id)
def test_global_grid_64_all_three_routes(L, case):
    """G = 64, T = 4096, one image, one head: MODE 2 (relh / relw from la_relpos_terms; the row term is added AFTER the tile maximum),
    MODE 4 (terms in the kernel, the second half of the row terms refilled at tile 32) and MODE 4 through la_attn_fwd_rows."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, _ = built(case)
    dtype, tol, tag = SP.TORCH_DT[dt], SP.TOL16[dt], SP.case_id(case)
    e, tpad, sc = heads * hd, t, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    tabh, tabw = p["tabh"].to(dtype), p["tabw"].to(dtype)
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    relh = torch.full((b * heads, t, g), NAN, device="cuda")
    relw = torch.full_like(relh, NAN)
    L.relpos_terms(qkv, b, heads, g, e, tabh, tabw, relh, relw)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd(qkv, vt, out, relh, relw, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS)
    check_rows(tag + " mode 2", out, ref, heads, tol)
    out4 = torch.full_like(out, NAN)
    L.attn_fwd(qkv, vt, out4, None, None, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS, tabh=tabh, tabw=tabw)
    check_rows(tag + " mode 4", out4, ref, heads, tol)
    out4r = torch.full_like(out, NAN)
    L.attn_fwd_rows(qkv, out4r, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS, tabh=tabh, tabw=tabw)
    check_rows(tag + " mode 4 la_attn_fwd_rows", out4r, ref, heads, tol)


# =========================================================================================================================
# forward: LA_ATTN_RELPOS_WIN16 (MODE 5), 16-wide slot order
# =========================================================================================================================
@pytest.mark.parametrize("case", fam(FWD, "win16"), ids=SP.case_id)
def test_windows_in_slot_order_both_v_layouts(L, case):
    """A tile is four key rows; G = 14 leaves two padded columns in every key row and a half-empty last tile.  V^T in slot order
    (la_attn_fwd) and row-major V (la_attn_fwd_rows)."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, _ = built(case)
    dtype, tol, tag = SP.TORCH_DT[dt], SP.TOL16[dt], SP.case_id(case)
    e, tpad, sc = heads * hd, (16 * g + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    tabh, tabw = p["tabh"].to(dtype), p["tabw"].to(dtype)
    vt = v_slot_order(qkv, b, heads, g, hd, tpad)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd(qkv, vt, out, None, None, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw)
    check_rows(tag + " la_attn_fwd", out, ref, heads, tol)
    out_r = torch.full_like(out, NAN)
    L.attn_fwd_rows(qkv, out_r, b, heads, t, tpad, g, e, sc, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw)
    check_rows(tag + " la_attn_fwd_rows", out_r, ref, heads, tol)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_windows_in_image_order_with_a_spike_on_the_pad_row(L, dt):
    """la_attn_fwd_rows, LA_ATTN_RELPOS_WIN16 on one 20 x 27 image in 14 x 14 windows: three of the four windows are padded, and the pad
    row's key stands >= 9 log2 above every real key for the loud rows - the pad row takes part in the softmax as the reference's
    pad-after-norm token does.  Reference: fp64 attention over the windows cut out explicitly."""
    iw = SP.build_image_windows(dt)
    win = on_gpu(iw["win"])
    g, ih, iwid, sc = iw["g"], iw["ih"], iw["iw"], iw["scale"]
    nwin, heads, t, hd = win["q"].shape
    dtype, tol, e = SP.TORCH_DT[dt], SP.TOL16[dt], heads * hd
    o, _ = SP.attention(win["q"], win["k"], win["v"], sc, g, win["tabh"], win["tabw"])
    ref_w = SP.rows_of(o)                                                              # [windows * t, E]
    q, k, v = iw["img"]
    qkv = SP.pack_qkv({"q": q, "k": k, "v": v}, dtype, "cuda")
    padrow = torch.cat([z.reshape(-1) for z in iw["pad"]]).to(dtype).cuda().contiguous()
    tpad = (16 * g + 63) // 64 * 64
    out = torch.full((ih * iwid, e), NAN, dtype=dtype, device="cuda")
    L.attn_fwd_rows(qkv, out, nwin, heads, t, tpad, g, e, sc, L.ATTN_RELPOS_WIN16, tabh=win["tabh"].to(dtype), tabw=win["tabw"].to(dtype),
                    img_hw=(ih, iwid), padrow=padrow)
    rows = iw["rows"].reshape(-1).cuda()
    ins = rows >= 0
    check_rows(f"win16-image-order-padspike-G{g}-{dt} la_attn_fwd_rows", out[rows[ins]], ref_w[ins], heads, tol)


# =========================================================================================================================
# forward: fp8 QK^T
# =========================================================================================================================
@pytest.mark.parametrize("case", fam(FWD, "fp8"), ids=SP.case_id)
def test_fp8_scores_attention(L, case):
    """la_qk_fp8 + la_attn_fwd_fp8 (attn_fwd_fp8_kernel: the third copy of the online softmax).  q and k hold e4m3 values, so the
    conversion is exact and the reference is the fp64 attention on the same operands."""
    _, kind, t, g, hd, dt, order, b, heads = case
    p, ref, _ = built(case)
    tag = SP.case_id(case)
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, torch.float16, "cuda")
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    qk8 = torch.empty(b * t, 2 * e, dtype=torch.uint8, device="cuda")
    L.qk_fp8(qkv, e, qk8)
    assert torch.equal(qk8.view(torch.float8_e4m3fn).float(), qkv[:, :2 * e].float())
    out = torch.full((b * t, e), NAN, dtype=torch.float16, device="cuda")
    L.attn_fwd_fp8(qk8, vt, out, b, heads, t, tpad, e, sc)
    check_rows(tag + " la_attn_fwd_fp8", out, ref, heads, SP.TOL_FP8)


# =========================================================================================================================
# backward behind the stored lse
# =========================================================================================================================
def _grad_check(tag, got, gref, e, bounds, loose, model=None):
    """model: the same gradients from SP.backward_rounding_model (rows).  Where 16-bit rounding ALONE already uses more than 0.9 of the
    project's bound - a statement about the reference, not about the kernel - the bound becomes 2 x the model's error."""
    for i, ((name, c0), bound) in enumerate(zip((("dq", 0), ("dk", e), ("dv", 2 * e)), bounds)):
        ref = gref[:, c0:c0 + e]
        err = float((got[:, c0:c0 + e] - ref).abs().max() / ref.abs().max())
        limit, note = loose * bound, ""
        if model is not None:
            e_model = float((model[i] - ref).abs().max() / ref.abs().max())
            note = f", 16-bit rounding model {e_model:.2e}"
            if e_model > 0.9 * limit:
                limit = 2.0 * e_model
        print(f"[cond] {tag}: {name} {err:.2e} (bound {limit:.1e}{note})")
        assert err <= limit, (tag, name, err)


@pytest.mark.parametrize("case", fam(BWD, "plain"), ids=SP.case_id)
def test_plain_attention_backward_from_the_stored_lse(L, case):
    """la_attn_fwd_lse -> la_attn_bwd against fp64 autograd on stairs / offset inputs: a wrong lse (m_run c2 + log2 l from the deferred
    state) shows as wrong P in dq / dk / dv.  Bounds: 4e-3 (tests/test_encoder_train_gpu.py), bf16 x 8.

    One case cannot meet it: offset, hd 64, fp16, dq.  The offset dimension gives every key the same k = +-22.25; in exact arithmetic its
    share of dq is scale * 22.25 * sum_k dS_k = 0, but dS reaches the MFMA rounded to 16 bits and the rounding errors do not cancel.
    SP.backward_rounding_model - fp64 with only the 16-bit roundings of O, P, dS and the stored results - gives 3.72e-3 of the largest
    entry for that case on its own (0.93 of the bound), so there the bound is 2 x the model's error = 7.4e-3; measured on the MI355X
    4.03e-3.  (The model reproduces the kernel's other figures to three digits: stairs hd 64 dq 1.97e-3, offset hd 128 dq 3.31e-3.)"""
    _, kind, t, g, hd, dt, b, heads = case
    p = on_gpu(SP.build(kind, t, hd, dt, SP.tiles_linear(t), b=b, heads=heads))
    dtype, loose, tag = SP.TORCH_DT[dt], (8.0 if dt == "bf16" else 1.0), SP.case_id(case) + " bwd"
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    dout = torch.randn(b * t, e, generator=torch.Generator().manual_seed(t + hd)).to(dtype).cuda()
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    lse = torch.full((b * heads, tpad), NAN, device="cuda")
    L.attn_fwd_lse(qkv, vt, out, lse, b, heads, t, tpad, e, sc)
    x = torch.stack([p["q"], p["k"], p["v"]]).requires_grad_(True)
    o, ref_lse = SP.attention(x[0], x[1], x[2], sc)
    check_lse(tag, lse, ref_lse.detach().reshape(b * heads, t), t)
    SP.rows_of(o).backward(dout.double())
    gref = torch.cat([SP.rows_of(x.grad[i]) for i in range(3)], 1)
    dvec = torch.full((b * heads, tpad), NAN, device="cuda")
    dqkv = torch.zeros(b * t, 3 * e, dtype=dtype, device="cuda")
    L.attn_bwd(qkv, out, dout, None, None, None, lse, dvec, dqkv, b, heads, t, tpad, e, sc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv).all())
    do4 = dout.double().view(b, t, heads, hd).permute(0, 2, 1, 3)
    model = [SP.rows_of(z) for z in SP.backward_rounding_model(p["q"], p["k"], p["v"], do4, sc, dt)]
    _grad_check(tag, dqkv.double(), gref, e, (4e-3, 4e-3, 4e-3), loose, model)


@pytest.mark.parametrize("case", fam(BWD, "relpos"), ids=SP.case_id)
def test_relpos_attention_backward_from_the_stored_lse(L, case):
    """la_attn_fwd_relpos_lse -> la_attn_bwd_relpos + la_relpos_bwd against fp64 autograd: G = 14 (matrix-pipe bias), 20 (LDS tables),
    64 (registers; one image, one head)."""
    _, kind, t, g, hd, dt, b, heads = case
    p = on_gpu(SP.build(kind, t, hd, dt, SP.tiles_linear(t), b=b, heads=heads, g=g))
    dtype, loose, tag = SP.TORCH_DT[dt], (8.0 if dt == "bf16" else 1.0), SP.case_id(case) + " bwd"
    e, tpad, sc = heads * hd, (t + 63) // 64 * 64, p["scale"]
    qkv = SP.pack_qkv(p, dtype, "cuda")
    tabh, tabw = p["tabh"].to(dtype), p["tabw"].to(dtype)
    dout = torch.randn(b * t, e, generator=torch.Generator().manual_seed(t + hd)).to(dtype).cuda()
    vt = v_transposed(L, qkv, b, heads, t, hd, tpad)
    relh = torch.full((b * heads, t, g), NAN, device="cuda")
    relw = torch.full_like(relh, NAN)
    L.relpos_terms(qkv, b, heads, g, e, tabh, tabw, relh, relw)
    out = torch.full((b * t, e), NAN, dtype=dtype, device="cuda")
    lse = torch.full((b * heads, tpad), NAN, device="cuda")
    L.attn_fwd_relpos_lse(qkv, vt, out, relh, relw, lse, b, heads, t, tpad, g, e, sc)
    x = torch.stack([p["q"], p["k"], p["v"]]).requires_grad_(True)
    rh, rw = p["tabh"].clone().requires_grad_(True), p["tabw"].clone().requires_grad_(True)
    o, ref_lse = SP.attention(x[0], x[1], x[2], sc, g, rh, rw)
    check_lse(tag, lse, ref_lse.detach().reshape(b * heads, t), t)
    SP.rows_of(o).backward(dout.double())
    gref = torch.cat([SP.rows_of(x.grad[i]) for i in range(3)], 1)
    dvec = torch.full((b * heads, tpad), NAN, device="cuda")
    dqkv = torch.zeros(b * t, 3 * e, dtype=dtype, device="cuda")
    drelh = torch.full((b * heads, t, g), NAN, device="cuda")
    drelw = torch.full_like(drelh, NAN)
    L.attn_bwd_relpos(qkv, out, dout, None, None, None, lse, dvec, dqkv, relh, relw, drelh, drelw, b, heads, t, tpad, g, e, sc)
    dtabh = torch.zeros(2 * g - 1, hd, device="cuda")
    dtabw = torch.zeros_like(dtabh)
    L.relpos_bwd(qkv, dqkv, drelh, drelw, tabh.float(), tabw.float(), dtabh, dtabw, b, heads, g, e)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(drelh).all()) and bool(torch.isfinite(drelw).all())
    _grad_check(tag, dqkv.double(), gref, e, (5e-3, 5e-3, 5e-3), loose)
    for name, mine, ref in (("dRh", dtabh, rh.grad), ("dRw", dtabw, rw.grad)):
        err = float((mine.double() - ref).abs().max() / ref.abs().max())
        print(f"[cond] {tag}: {name} {err:.2e} (bound {loose * 3e-3:.1e})")
        assert err <= loose * 3e-3, (tag, name, err)


# =========================================================================================================================
# the fp32 softmax kernels that merge partial (max, sum, acc) states
# =========================================================================================================================
HW, NT, D, GROUPS, HEADS = 200, 5, 256, 2, 8


def _spread_levels(n, block, order):
    """one level per block of ``block`` consecutive positions, evenly from -12 to +12 nat (ascending) or back"""
    nb = -(-n // block)
    lv = torch.linspace(-12.0, 12.0, nb) if nb > 1 else torch.zeros(1)
    if order == "descending":
        lv = lv.flip(0)
    return lv[torch.arange(n) // block]


def _block_maxima_ok(s_nat, n, block, order):
    """s_nat [..., n] reference scores: |s| <= 16 nat; block maxima monotone, first and last >= 20 log2 units apart"""
    assert float(s_nat.abs().max()) <= 16.0, float(s_nat.abs().max())
    nb = -(-n // block)
    bm = torch.stack([s_nat[..., j * block:(j + 1) * block].amax(-1) for j in range(nb)], -1) * SP.LOG2E
    step = bm[..., 1:] - bm[..., :-1]
    assert bool((step > 0).all()) if order == "ascending" else bool((step < 0).all())
    spread = float((bm[..., -1] - bm[..., 0]).abs().min())
    assert spread >= 20.0, spread
    return spread, float(step.abs().min())


def _small_bwd_bounds(q, k, v, do, scale):
    """First-order fp32 error budget of softmax-attention gradients, per element, from fp64 quantities ([b, heads, n, hd] tensors).
    U = 2^-24.  A score is an hd-term fmaf chain times the scale: |ds| <= (hd + 2) U scale sum_f |q_f k_f| =: dl; with DL = its row
    maximum, P = exp(s - m) / l is off by rho P, rho = 4 DL + 4 eps_e + 2 (nk + 3) U (score and maximum move by DL each, numerator and
    denominator are nk-term sums, expf at 1 ulp: the budget of tests/test_cross_extract_gpu.py).  dP = do . v and D = do . o are hd-term
    sums (o itself off by rho sum P |v|), dS = P (dP - D), and dq = scale dS k, dk = scale dS^T q, dv = P^T do are nk- / nq-term sums."""
    u, eps_e = 2.0 ** -24, 2.0 ** -23
    hd, nq, nk = q.shape[-1], q.shape[-2], k.shape[-2]
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    p = torch.softmax(scale * (q @ kt), -1)
    dl = (hd + 2) * u * scale * (q.abs() @ kt.abs())
    rho = 4 * dl.amax(-1, keepdim=True) + 4 * eps_e + 2 * (nk + 3) * u
    o, dp = p @ v, do @ vt
    e_o = rho * (p @ v.abs()) + (nk + 1) * u * (p @ v.abs())
    e_dp = (hd + 1) * u * (do.abs() @ vt.abs())
    dd = (do * o).sum(-1, keepdim=True)
    e_dd = (hd + 1) * u * (do.abs() * o.abs()).sum(-1, keepdim=True) + (do.abs() * e_o).sum(-1, keepdim=True)
    ds = p * (dp - dd)
    e_ds = rho * ds.abs() + p * (e_dp + e_dd) + 2 * u * p * (dp.abs() + dd.abs())
    b_dq = scale * (e_ds @ k.abs() + (nk + 2) * u * (ds.abs() @ k.abs()))
    b_dk = scale * (e_ds.transpose(-1, -2) @ q.abs() + (nq + 2) * u * (ds.abs().transpose(-1, -2) @ q.abs()))
    b_dv = (rho * p).transpose(-1, -2) @ do.abs() + (nq + 2) * u * (p.transpose(-1, -2) @ do.abs())
    tiny = 1e-30
    return b_dq + tiny, b_dk + tiny, b_dv + tiny


def _small_bwd_fp32_torch(q, k, v, w, b, nq, nk, heads, hd):
    """The same gradients from plain torch in fp32 on the same inputs, two ways: autograd of softmax(q k^T / sqrt(hd)) v, and the
    formulas la_attn_small_bwd uses (P = exp(s - lse), delta = dO . O, dS = P (dP - delta)).  -> [(dq, dk, dv), (dq, dk, dv)] as rows."""
    e, sc = heads * hd, 1.0 / math.sqrt(hd)
    qg, kg, vg = (z.detach().float().clone().requires_grad_(True) for z in (q, k, v))
    q4, k4, v4 = (z.view(b, n, heads, hd).transpose(1, 2) for z, n in ((qg, nq), (kg, nk), (vg, nk)))
    o = (torch.softmax(q4 @ k4.transpose(-1, -2) * sc, -1) @ v4).transpose(1, 2).reshape(b * nq, e)
    (o * w.float()).sum().backward()
    with torch.no_grad():
        do = w.float().view(b, nq, heads, hd).transpose(1, 2)
        s = q4 @ k4.transpose(-1, -2) * sc
        p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
        ds = p * (do @ v4.transpose(-1, -2) - (do * (p @ v4)).sum(-1, keepdim=True)) * sc
        flash = [z.transpose(1, 2).reshape(-1, e) for z in (ds @ k4, ds.transpose(-1, -2) @ q4, p.transpose(-1, -2) @ do)]
    return [(qg.grad, kg.grad, vg.grad), tuple(flash)]


@pytest.mark.parametrize("kind", ["ascending", "descending", "offset+", "offset-"])
@pytest.mark.parametrize("long_side", ["keys", "queries"])
def test_small_attention_forward_lse_and_both_backward_forms(L, kind, long_side):
    """la_attn_small + la_attn_small_lse + la_attn_small_bwd, 8 heads of 16: 5 queries over 200 keys (backward with the row statistics of
    la_attn_small_lse) and 200 queries over 5 keys (the few-keys backward).  spread: the maxima of the 64-key blocks (of the single keys
    on the short side) rise or fall monotonically over >= 20 log2 units, |score| <= 16 nat; offset: every score moved by +-12 nat.
    Bounds: 2e-6 forward (tests/test_decoder_ops_gpu.py), lse 1e-5 absolute at |lse| <= 24.

    Backward, max-norm relative to max(1, largest entry): the project's 5e-6 (tests/test_train_gpu.py) wherever plain fp32 reaches it.
    It belongs to scores ~ N(0, 1): at |score| = 12 torch's own fp32 misses it on these inputs (up to 3.3e-5 on dk, queries long), so
    the bound is max(5e-6, 2 x the larger error of two plain torch fp32 evaluations of the same inputs: autograd, and the kernel's
    formulas P = exp(s - lse), delta = dO . O), computed in the test.  The few-queries form (keys long) also inherits the forward
    kernel's own tolerance through delta (derivation at ``fwd_share`` below), which matters for the ascending spread, where
    sum_k P k sits at the top level 12.  Measured on the MI355X: dq 1.33e-5 there against torch fp32 5.0e-6 - the forward output is
    1.0e-6 off (fast exponential over a 24 nat range), inside its 2e-6; every other figure is within max(5e-6, 2 x torch).
    Second check, per element: the worst-case first-order fp32 budget of ``_small_bwd_bounds`` (measured at most 0.044 of it)."""
    from labelanything_amd import autograd_ops as A
    b, heads, hd = GROUPS, HEADS, D // 2 // HEADS
    nq, nk = (NT, HW) if long_side == "keys" else (HW, NT)
    e = heads * hd
    gen = torch.Generator().manual_seed(nq * 3 + nk)
    q = 0.3 * torch.randn(b * nq, e, generator=gen)
    k = 0.3 * torch.randn(b * nk, e, generator=gen)
    v = torch.randn(b * nk, e, generator=gen)
    w = torch.randn(b * nq, e, generator=gen)
    q.view(b, nq, heads, hd)[..., 0] = math.sqrt(hd)                                  # score = k[.., 0] + noise
    if kind.startswith("offset"):
        k.view(b, nk, heads, hd)[..., 0] = 12.0 if kind == "offset+" else -12.0
    else:
        k.view(b, nk, heads, hd)[..., 0] = _spread_levels(nk, 64 if nk > 64 else 1, kind)[None, :, None]
    qd, kd, vd = (z.double().cuda().requires_grad_(True) for z in (q, k, v))
    q4, k4, v4 = (z.view(b, n, heads, hd).transpose(1, 2) for z, n in ((qd, nq), (kd, nk), (vd, nk)))
    s = q4 @ k4.transpose(-1, -2) / math.sqrt(hd)
    if kind.startswith("offset"):
        assert float(s.detach().abs().max()) <= 16.0 and float(s.detach().abs().min()) >= 8.0
    else:
        print(f"[cond] attn_small {long_side} {kind}: block maxima spread / smallest step (log2)", _block_maxima_ok(s.detach(), nk, 64 if nk > 64 else 1, kind))
    ref = (torch.softmax(s, -1) @ v4).transpose(1, 2).reshape(b * nq, e)
    (ref * w.double().cuda()).sum().backward()
    qg, kg, vg = (z.cuda().requires_grad_(True) for z in (q, k, v))
    o = A.attention(qg, kg, vg, b, nq, nk, heads)
    (o * w.cuda()).sum().backward()
    lse = torch.full((b * nq * heads,), NAN, device="cuda")
    L.attn_small_lse(qg.detach(), kg.detach(), b, nq, nk, heads, hd, lse)
    torch.cuda.synchronize()
    ref_lse = torch.logsumexp(s.detach(), -1).permute(0, 2, 1).reshape(-1)             # index (b nq + q) heads + h
    e_o = float((o.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max())
    e_l = float((lse.double() - ref_lse).abs().max())
    print(f"[cond] attn_small {long_side} {kind}: out {e_o:.2e} (2e-6)  lse {e_l:.2e} (1e-5)")
    assert bool(torch.isfinite(o).all()) and e_o <= 2e-6
    assert e_l <= 1e-5
    # few-queries form: delta_q = dO_q . O_q is formed from the STORED forward output, which la_attn_small may miss by 2e-6 of max |O|
    # (its own bound); with the hd component errors adding in quadrature delta_q moves by 2e-6 max|O| |dO_q|_2, and since
    # dS = P (dP - delta), dq_q moves by scale |sum_k P_qk k_k| and dk_k by scale sum_q P_qk |q_q| times that.
    fwd_share = [0.0, 0.0, 0.0]
    if long_side == "keys":
        pm = torch.softmax(s.detach(), -1)
        d_delta = 2e-6 * float(ref.detach().abs().max()) * w.double().cuda().view(b, nq, heads, hd).transpose(1, 2).norm(dim=-1, keepdim=True)
        sc_ = 1.0 / math.sqrt(hd)
        fwd_share = [float((sc_ * (pm @ k4.detach()).abs() * d_delta).max()), float((sc_ * (pm * d_delta).transpose(-1, -2) @ q4.detach().abs()).max()), 0.0]
    models = _small_bwd_fp32_torch(q.cuda(), k.cuda(), v.cuda(), w.cuda(), b, nq, nk, heads, hd)
    bounds = _small_bwd_bounds(q4.detach(), k4.detach(), v4.detach(), w.double().cuda().view(b, nq, heads, hd).transpose(1, 2), 1.0 / math.sqrt(hd))
    for i, ((name, mine, r), bound) in enumerate(zip((("dq", qg.grad, qd.grad), ("dk", kg.grad, kd.grad), ("dv", vg.grad, vd.grad)), bounds)):
        err = (mine.double() - r).abs()
        den = max(1.0, float(r.abs().max()))
        e_torch = max(float((mdl[i].double() - r).abs().max()) for mdl in models) / den
        limit = max(5e-6, 2.0 * e_torch) + fwd_share[i] / den
        print(f"[cond] attn_small {long_side} {kind}: {name} {float(err.max()) / den:.2e} (bound {limit:.1e} = max(5e-6, 2 x torch fp32 {e_torch:.2e})"
              f" + forward tolerance through delta {fwd_share[i] / den:.1e})")
        n_rows = mine.shape[0] // b
        ratio = float((err / bound.transpose(1, 2).reshape(b * n_rows, e)).max())
        print(f"[cond] attn_small {long_side} {kind}: {name} {float(err.max()) / max(1.0, float(r.abs().max())):.2e} of the largest entry, "
              f"worst ratio to the fp32 error budget {ratio:.3f}")
        assert bool(torch.isfinite(mine).all()) and ratio <= 1.0, name
        assert float(err.max()) / den <= limit, (name, float(err.max()) / den, limit)


def _planes(w):
    hi = w.to(torch.float16)
    return hi.contiguous(), (w - hi.float()).to(torch.float16).contiguous()


@pytest.mark.parametrize("kind", ["ascending", "descending", "offset+", "offset-"])
def test_twoway_tokens_to_image_merges_tile_partials(L, kind):
    """la_twoway_t2i (groups 2, hw 200 = four 64-row tiles, 5 tokens, D 256): every 64-row tile leaves (max, sum, acc) partials that are
    merged with exp(p - M).  W_k = [I | 0] + small noise, so the keys follow the first D / 2 stream channels and channel 0 of every head
    carries one level per tile: tile maxima monotone over >= 20 log2 units (weights 2^-20 .. 1 both ways), |score| <= 16 nat.
    Bound: 2e-5, as tests/test_ops_gpu.py::test_fused_twoway_image_side_kernels (split-precision operands, ~21 mantissa bits; the
    derived ceiling max |score| 2^-21 x 2 = 1.5e-5 lies below it)."""
    g, hw, nt, d, heads = GROUPS, HW, NT, D, HEADS
    di, hd = d // 2, d // 16
    gen = torch.Generator().manual_seed(91)
    x = torch.randn(g * hw, d, generator=gen)
    pe = 0.3 * torch.randn(hw, d, generator=gen)
    wk = torch.eye(di, d) + torch.randn(di, d, generator=gen) / 256
    wv = torch.randn(di, d, generator=gen) / 16
    bk, bv = 0.1 * torch.randn(di, generator=gen), torch.randn(di, generator=gen)
    qt = 0.3 * torch.randn(g * nt, di, generator=gen)
    qt.view(g, nt, heads, hd)[..., 0] = math.sqrt(hd)
    lvl = torch.full((hw,), 12.0 if kind == "offset+" else -12.0) if kind.startswith("offset") else _spread_levels(hw, 64, kind)
    x.view(g, hw, d)[..., :di].view(g, hw, heads, hd)[..., 0] = lvl[None, :, None]
    pe.view(hw, d)[:, :di].view(hw, heads, hd)[..., 0] = 0.0
    x, pe, wk, wv, bk, bv, qt = (z.cuda() for z in (x, pe, wk, wv, bk, bv, qt))
    x64, pe64, wk64, wv64, bk64, bv64, q64 = (z.double() for z in (x, pe, wk, wv, bk, bv, qt))

    def heads_of(z, n):
        return z.view(g, n, heads, hd).transpose(1, 2)

    kk = ((x64.view(g, hw, d) + pe64).reshape(g * hw, d)) @ wk64.t() + bk64
    vv = x64 @ wv64.t() + bv64
    s = heads_of(q64, nt) @ heads_of(kk, hw).transpose(-1, -2) / math.sqrt(hd)
    if kind.startswith("offset"):
        assert float(s.abs().max()) <= 16.0 and float(s.abs().min()) >= 8.0
    else:
        print(f"[cond] twoway_t2i {kind}: tile maxima spread / smallest step (log2)", _block_maxima_ok(s, hw, 64, kind))
    ref = (torch.softmax(s, -1) @ heads_of(vv, hw)).transpose(1, 2).reshape(g * nt, di)
    part = torch.full((L.twoway_part_size(g, hw, nt, d),), NAN, device="cuda")
    out = torch.full((g * nt, di), NAN, device="cuda")
    L.twoway_t2i(x, _planes(wk), _planes(wv), L.twoway_pe_layout((pe @ wk.t() + bk).contiguous()), bv, qt, g, hw, nt, heads, part, out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[cond] twoway_t2i {kind}: out {err:.2e} (2e-5)")
    assert err <= 2e-5


@pytest.mark.parametrize("kind", ["ascending", "descending", "offset+", "offset-"])
def test_extract_pool_merges_waves_and_pieces(L, kind):
    """la_extract_pool, three slabs of hw 200 at D 256, 8 queries per pair: la_extract_pool_plan must cut the 600 rows into >= 2 pieces,
    so both the merge of the waves inside a piece and the merge of the pieces run.  Channel 0 of the stream carries one level per PIECE
    (maxima monotone over >= 20 log2 units) plus a ramp of 1.5 nat inside each piece, so the waves of a piece differ as well.  Bound:
    the derived one of tests/test_cross_extract_gpu.py (fmaf chain of the scores, expf at 1 ulp, L-term fp32 sums)."""
    b, m, c, hw, d, n = 1, 3, 2, HW, D, 1
    r, lrows = 8 * n, m * hw
    split, ns, per = L.extract_pool_plan(m, hw, d, r)
    assert ns >= 2, (split, ns)
    gen = torch.Generator().manual_seed(17)
    xp = torch.randn(b * c, lrows, d, generator=gen)                                   # (pair, row, D)
    qt = torch.randn(b * c, r, d, generator=gen) * (0.4 / math.sqrt(d))
    qt[..., 0] = 1.0
    if kind.startswith("offset"):
        xp[..., 0] = 12.0 if kind == "offset+" else -12.0
    else:
        pos = torch.arange(lrows)
        xp[..., 0] = (_spread_levels(lrows, split, kind) + 1.5 * (pos % split) / split)[None]
    x = xp.view(b, c, m, hw, d).permute(0, 2, 1, 3, 4).reshape(b * m * c, hw, d).contiguous()
    s = qt.double() @ xp.double().transpose(1, 2)
    if kind.startswith("offset"):
        assert float(s.abs().max()) <= 16.0 and float(s.abs().min()) >= 8.0
    else:
        print(f"[cond] extract_pool {kind}: pieces {ns} of {split} rows, piece maxima spread / smallest step (log2)", _block_maxima_ok(s, lrows, split, kind))
    p = torch.softmax(s, -1)
    ref = p @ xp.double()
    u, eps_e = 2.0 ** -24, 2.0 ** -23
    delta = (d + 1) * u * (qt.double().abs() @ xp.double().abs().transpose(1, 2)).max(-1, keepdim=True).values
    bound = (4 * delta + 4 * eps_e + 2 * (lrows + 3) * u) * (p @ xp.double().abs())
    scratch = torch.full((b * c * per,), NAN, device="cuda")
    out = torch.full((b * c, r, d), NAN, device="cuda")
    L.extract_pool(x.cuda(), qt.cuda(), b, m, c, hw, d, n, scratch, out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    err = (out.double().cpu() - ref).abs()
    print(f"[cond] extract_pool {kind}: err {float(err.max()):.2e}, worst ratio to the derived bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
