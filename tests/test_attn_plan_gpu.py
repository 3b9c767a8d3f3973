"""GPU: la_attn_fwd_plan / la_attn_bwd_plan asked with the very tensors of a call, next to the call itself.

tests/test_attn_plan_cpu.py pins the plan to the launches of the commit before csrc/attn_plan.h on placeholder addresses.  Here the plan is
asked with device tensors: it must not depend on where the buffers lie, every launch it names must fit the part (a workgroup of at most
1024 threads, at most the 160 KiB of LDS the launchers raise the limit to), and the entry point that launches it must give the attention
of the fp64 reference (tests/softmax_profiles.py) within the suite's bounds - TOL16 forward, 5e-3 per gradient block as
tests/test_sam_train_gpu.py.  One small shape per kernel family; the conditioning suite covers the numerics in depth.
"""
import math

import pytest
import torch

from labelanything_amd import _lib as L
from tests import softmax_profiles as SP

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024
FWD, WINDOW, DQ, DKV, RB_ROWS, RB = range(6)
B, HEADS, G, HD = 2, 2, 14, 64
T, TPAD, E = G * G, 256, HEADS * HD


def inputs(dt="f16"):
    gen = torch.Generator().manual_seed(14)
    p = {n: SP.round_to(torch.randn(B, HEADS, T, HD, generator=gen, dtype=torch.float64), dt).cuda() for n in ("q", "k", "v")}
    tabs = [SP.round_to(0.1 * torch.randn(2 * G - 1, HD, generator=gen, dtype=torch.float64), dt).cuda() for _ in range(2)]
    return p, tabs, SP.pack_qkv(p, SP.TORCH_DT[dt], "cuda")


def fields(plan):
    return [tuple(getattr(plan.launch[i], f) for f, _ in L.LaAttnLaunch._fields_) for i in range(plan.n)] + [(plan.n, plan.repeat, plan.ry)]


def fits(plan):
    for i in range(plan.n):
        l = plan.launch[i]
        assert 0 < l.grid and 0 < l.block <= 1024 and 0 <= l.lds_bytes <= LDS_LIMIT, (l.kernel, l.grid, l.block, l.lds_bytes)


def close(got, ref, tol):
    assert bool(torch.isfinite(got).all())
    assert float((got.double() - ref).abs().max()) <= tol * float(ref.abs().max())


def test_forward_plans_of_real_tensors_fit_and_their_launches_compute_attention():
    p, (tabh, tabw), qkv = inputs()
    sc, tol = 1.0 / math.sqrt(HD), SP.TOL16["f16"]
    shape = dict(B=B, heads=HEADS, T=T, Tpad=TPAD, E=E, dt=L.LA_F16)
    out = torch.full((B * T, E), float("nan"), dtype=torch.float16, device="cuda")
    # la_attn_fwd_rows, plain: the tile kernel in its V-row form
    plan = L.attn_fwd_plan("attn_fwd_rows", qkv=qkv, out16=out, G=0, mode=L.ATTN_PLAIN, **shape)
    assert fields(plan) == fields(L.attn_fwd_plan("attn_fwd_rows", qkv=0x1000, out16=0x2000, G=0, mode=L.ATTN_PLAIN, **shape))
    assert (plan.launch[0].kernel, plan.launch[0].vrow) == (FWD, 1)
    fits(plan)
    L.attn_fwd_rows(qkv, out, B, HEADS, T, TPAD, 0, E, sc, L.ATTN_PLAIN)
    close(out, SP.rows_of(SP.attention(p["q"], p["k"], p["v"], sc)[0]), tol)
    # la_attn_fwd, rel-pos with the tables on a 14 x 14 grid of 64-wide heads: the no-LDS window kernel
    vt = torch.empty(B * HEADS, HD, TPAD, dtype=torch.float16, device="cuda")
    L.head_transpose(qkv, 2 * E, B, HEADS, T, TPAD, vt)
    th, tw = tabh.half(), tabw.half()
    plan = L.attn_fwd_plan("attn_fwd", qkv=qkv, vt=vt, out16=out, tabh=th, tabw=tw, G=G, mode=L.ATTN_RELPOS, **shape)
    assert fields(plan) == fields(L.attn_fwd_plan("attn_fwd", qkv=8, vt=16, out16=24, tabh=32, tabw=40, G=G, mode=L.ATTN_RELPOS, **shape))
    assert plan.launch[0].kernel == WINDOW
    fits(plan)
    out.fill_(float("nan"))
    L.attn_fwd(qkv, vt, out, None, None, B, HEADS, T, TPAD, G, E, sc, L.ATTN_RELPOS, tabh=th, tabw=tw)
    close(out, SP.rows_of(SP.attention(p["q"], p["k"], p["v"], sc, G, tabh, tabw)[0]), tol)


def test_backward_plans_of_real_tensors_fit_and_their_launches_compute_the_gradients():
    p, (tabh, tabw), qkv = inputs()
    sc = 1.0 / math.sqrt(HD)
    th, tw = tabh.half(), tabw.half()
    vt = torch.empty(B * HEADS, HD, TPAD, dtype=torch.float16, device="cuda")
    L.head_transpose(qkv, 2 * E, B, HEADS, T, TPAD, vt)
    relh = torch.empty(B * HEADS, T, G, device="cuda")
    relw = torch.empty_like(relh)
    L.relpos_terms(qkv, B, HEADS, G, E, th, tw, relh, relw)
    out = torch.empty(B * T, E, dtype=torch.float16, device="cuda")
    lse = torch.full((B * HEADS, TPAD), float("nan"), device="cuda")
    L.attn_fwd_relpos_lse(qkv, vt, out, relh, relw, lse, B, HEADS, T, TPAD, G, E, sc)
    dout = torch.randn(B * T, E, generator=torch.Generator().manual_seed(3)).half().cuda()
    dvec = torch.empty(B * HEADS, TPAD, device="cuda")
    dqkv = torch.zeros(B * T, 3 * E, dtype=torch.float16, device="cuda")
    drelh, drelw = torch.empty_like(relh), torch.empty_like(relh)
    dtabh = torch.zeros(2 * G - 1, HD, device="cuda")
    dtabw = torch.zeros_like(dtabh)
    shape = dict(B=B, heads=HEADS, G=G, E=E, dt=L.LA_F16)
    plan = L.attn_bwd_plan("attn_bwd_relpos", qkv=qkv, out16=out, dout16=dout, lse=lse, dvec=dvec, dqkv=dqkv, relh=relh, relw=relw, drelh=drelh,
                           drelw=drelw, T=T, Tpad=TPAD, **shape)
    assert [plan.launch[i].kernel for i in range(plan.n)] == [DQ, DKV]
    fits(plan)
    tplan = L.attn_bwd_plan("relpos_bwd", qkv=qkv, dqkv=dqkv, drelh=drelh, drelw=drelw, tabh=tabh.float(), tabw=tabw.float(), dtabh=dtabh, dtabw=dtabw,
                            **shape)
    assert (tplan.n, tplan.launch[0].kernel, tplan.repeat) == (1, RB_ROWS, 1)
    fits(tplan)
    L.attn_bwd_relpos(qkv, out, dout, None, None, None, lse, dvec, dqkv, relh, relw, drelh, drelw, B, HEADS, T, TPAD, G, E, sc)
    L.relpos_bwd(qkv, dqkv, drelh, drelw, tabh.float(), tabw.float(), dtabh, dtabw, B, HEADS, G, E)
    x = torch.stack([p["q"], p["k"], p["v"]]).requires_grad_(True)
    rh, rw = tabh.clone().requires_grad_(True), tabw.clone().requires_grad_(True)
    SP.rows_of(SP.attention(x[0], x[1], x[2], sc, G, rh, rw)[0]).backward(dout.double())
    for i in range(3):
        close(dqkv[:, i * E:(i + 1) * E], SP.rows_of(x.grad[i]), 5e-3)
    close(dtabh, rh.grad, 3e-3)
    close(dtabw, rw.grad, 3e-3)
