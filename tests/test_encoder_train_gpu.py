"""GPU: backward through the image encoder (HF ViT stack) - the kernels one by one against torch autograd, then the whole encoder
and the whole training step against the CPU oracle's autograd with EVERY parameter trainable, which is what the reference trains with
parameters/trainval/coco20i/mae_noembs.yaml (no freeze_backbone -> Lam.get_learnable_params returns self.parameters(),
models/lam.py:321-347)."""
import math

import pytest
import torch

from labelanything_amd import _lib as L
from tests.helpers import NAN, check_guards, guarded, make_gt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 2, 197), (1, 3, 64), (3, 1, 130), (1, 2, 901), (2, 2, 197, 128), (1, 1, 901, 128), (3, 1, 64, 128)])
def test_attention_forward_lse_and_backward_match_torch(shape):
    """4th entry: head width 128 (two 64-wide halves in every kernel; SAM ViT-H's 80-wide heads run zero-padded to it)."""
    b, heads, t = shape[:3]
    hd = shape[3] if len(shape) > 3 else 64
    e = heads * hd
    tpad = (t + 63) // 64 * 64
    g = torch.Generator().manual_seed(b * 1000 + t)
    qkv = (torch.randn(b * t, 3 * e, generator=g) * 0.7).half().cuda()
    dout = torch.randn(b * t, e, generator=g).half().cuda()
    scale = 1.0 / math.sqrt(hd)

    def heads_t(src, col0):
        dst = torch.empty(b * heads, hd, tpad, dtype=torch.float16, device="cuda")
        L.head_transpose(src, col0, b, heads * (hd // 64), t, tpad, dst)          # (a 128-wide head = two 64-row blocks)
        return dst

    vt = heads_t(qkv, 2 * e)
    ref_vt = qkv[:, 2 * e:].view(b, t, heads, hd).permute(0, 2, 3, 1).reshape(b * heads, hd, t)
    assert torch.equal(vt[:, :, :t], ref_vt) and float(vt[:, :, t:].abs().max() if tpad > t else 0) == 0.0
    out = torch.empty(b * t, e, dtype=torch.float16, device="cuda")
    lse = torch.full((b * heads, tpad), 1e30, device="cuda")
    L.attn_fwd_lse(qkv, vt, out, lse, b, heads, t, tpad, e, scale)
    # torch reference on the same (16-bit valued) inputs in fp64
    x = qkv.double().cpu().view(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4).requires_grad_(True)       # (3, b, heads, t, hd)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * scale
    o = torch.softmax(s, -1) @ v                                                                        # (b, heads, t, 64)
    o_rows = o.permute(0, 2, 1, 3).reshape(b * t, e)
    assert float((out.double().cpu() - o_rows.detach()).abs().max()) <= 2e-3 * float(o_rows.abs().max())
    ref_lse = torch.logsumexp(s.detach(), -1).reshape(b * heads, t) * 1.4426950408889634
    assert float((lse[:, :t].double().cpu() - ref_lse).abs().max()) <= 2e-3
    assert bool((lse[:, t:] == 1e30).all())
    o_rows.backward(dout.double().cpu())
    gref = x.grad.permute(1, 3, 0, 2, 4).reshape(b * t, 3 * e)                                          # rows (b, t), cols (q|k|v, head, d)
    kt = qt = dot = None                                     # (unused since round 5: LDS transpose reads)
    # the C entry point is self-contained: an uninitialised workspace (NaN) and garbage in the padded LSE entries must not reach dK
    dvec = torch.full((b * heads, tpad), float("nan"), device="cuda")
    lse[:, t:] = float("nan")
    dqkv = torch.zeros(b * t, 3 * e, dtype=torch.float16, device="cuda")
    L.attn_bwd(qkv, out, dout, kt, qt, dot, lse, dvec, dqkv, b, heads, t, tpad, e, scale)
    torch.cuda.synchronize()
    got = dqkv.double().cpu()
    for name, c0 in (("dq", 0), ("dk", e), ("dv", 2 * e)):
        ref = gref[:, c0:c0 + e]
        err = float((got[:, c0:c0 + e] - ref).abs().max()) / float(ref.abs().max())
        assert err <= 4e-3, (name, err)                      # P, dS and the outputs are rounded to fp16 (2^-11) once each
    dref = (dout.double().cpu() * o_rows.detach()).view(b, t, heads, hd).sum(-1).permute(0, 2, 1).reshape(b * heads, t)
    assert float((dvec[:, :t].double().cpu() - dref).abs().max()) <= 3e-3 * float(dref.abs().max())
    assert bool((dvec[:, t:] == 0).all()) and bool((lse[:, t:] == 1e30).all()) and bool(torch.isfinite(dqkv).all())


def _hf_cfg(size=240, encoder="hf_tiny"):
    from labelanything_amd.config import LamConfig
    return LamConfig(encoder=encoder, image_size=size, image_embed_dim=128, embed_dim=64, spatial_convs=3, example_class_attention=False,
                     custom_preprocess=False)


@pytest.mark.parametrize("size", [240, 224, (224, "hf_hd32_tiny")])      # 240: position embeddings bicubically resampled 14 -> 15; 224: used as stored
def test_encoder_gradients_of_a_linear_functional_match_oracle_autograd(size):
    """HfEncoderGraph alone: L = sum(R * encoder(images)) for a fixed random R, every encoder parameter's gradient against torch
    autograd of the CPU oracle's fp32 encoder (pinned on the reference).  16-bit MFMA operands forward and backward: the bound is the
    measured level x 2 (the error-budget statement VERDICT r2 asks for: gradients through 16-bit operands do not reach 3e-4)."""
    from labelanything_amd.models import Lam
    from labelanything_amd.train_encoder import HfEncoderGraph
    from labelanything_amd.weights import init_state_dict
    from oracle import lam_oracle as O
    from tests.cases import geometry_for
    import tests.cases  # noqa: F401  (registers hf_tiny)
    encoder = "hf_tiny"
    if isinstance(size, tuple):                      # 32-wide heads: zero-padded to 64 columns per head, forward and backward (VERDICT r4 missing 2)
        size, encoder = size
    cfg = _hf_cfg(size, encoder)
    g = torch.Generator().manual_seed(size)
    images = torch.randn(3, 3, size, size, generator=g)
    sd = init_state_dict(cfg, 31)
    wref = {k: (v.clone().requires_grad_(True) if k.startswith("image_encoder.") and v.is_floating_point() else v) for k, v in sd.items()}
    out_ref = O.hf_vit_encoder(wref, geometry_for(cfg), images)                      # (Bn, C, g, g)
    r = torch.randn(out_ref.shape, generator=g)
    (out_ref * r).sum().backward()
    lam = Lam(cfg, seed=31).cuda()
    names = [k for k, p in lam.named_parameters() if k.startswith("image_encoder.")]
    grads = {k: torch.zeros_like(dict(lam.named_parameters())[k]) for k in names}
    graph = HfEncoderGraph(lam, grads)
    out = graph.forward(images.cuda())
    bn, c, gg, _ = out_ref.shape
    ref_rows = out_ref.detach().permute(0, 2, 3, 1).reshape(bn * gg * gg, c)
    assert float((out.cpu() - ref_rows).abs().max()) <= 1e-3 * float(ref_rows.abs().max())
    graph.backward(r.permute(0, 2, 3, 1).reshape(bn * gg * gg, c).contiguous().cuda())
    torch.cuda.synchronize()
    gmax = max(float(wref[k].grad.abs().max()) for k in names)
    worst = {}
    for k in names:
        ref = wref[k].grad
        worst[k] = float((grads[k].cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-2 * gmax)
    order = sorted(worst.items(), key=lambda kv: -kv[1])
    print(f"encoder gradients (linear functional, size {size}, loss scale {graph.last_scale:g}): worst", [(k[14:], f"{v:.2e}") for k, v in order[:6]])
    assert order[0][1] <= 1e-2, order[:6]


def test_encoder_backward_loss_scale_retry_and_non_finite_gradients():
    """The encoder backward scales the incoming gradient by a power of two (largest entry near TARGET_MAX), checks that every scaled
    gradient is finite with ONE min / max reduction over its scratch and repeats with 1 / 256 of the scale when a 16-bit intermediate
    overflowed.  A target far above what fp16 holds forces that retry: the gradients must equal the normal run's to 16-bit accuracy and
    ``last_scale`` must be smaller than the first scale tried.  A NaN or an infinity in the incoming gradient raises instead of training on."""
    from labelanything_amd.models import Lam
    from labelanything_amd.train_encoder import HfEncoderGraph
    import tests.cases  # noqa: F401  (registers hf_tiny)
    import math
    cfg = _hf_cfg(224)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 224, 224, generator=g).cuda()
    lam = Lam(cfg, seed=31).cuda()
    names = [k for k, p in lam.named_parameters() if k.startswith("image_encoder.")]

    def run(target):
        grads = {k: torch.zeros_like(dict(lam.named_parameters())[k]) for k in names}
        graph = HfEncoderGraph(lam, grads)
        if target is not None:
            graph.TARGET_MAX = target
        out = graph.forward(images)
        r = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).cuda()
        graph.backward(r)
        torch.cuda.synchronize()
        first = 2.0 ** math.floor(math.log2(graph.TARGET_MAX / float(r.abs().max())))
        return grads, graph, out, first

    base, graph0, out, first0 = run(None)
    assert graph0.last_scale == first0                                   # the normal run needs no retry
    big, graph1, _, first1 = run(float(HfEncoderGraph.TARGET_MAX) * 2.0 ** 14)
    assert graph1.last_scale < first1, (graph1.last_scale, first1)      # the first scale overflowed a 16-bit intermediate
    gmax = max(float(v.abs().max()) for v in base.values())
    for k in names:
        assert bool(torch.isfinite(big[k]).all()), k
        err = float((big[k] - base[k]).abs().max()) / max(float(base[k].abs().max()), 1e-2 * gmax)
        assert err <= 1e-2, (k, err)
    for bad in (float("nan"), float("inf"), float("-inf")):
        grads = {k: torch.zeros_like(dict(lam.named_parameters())[k]) for k in names}
        graph = HfEncoderGraph(lam, grads)
        graph.forward(images)
        r = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).cuda()
        r[3, 5] = bad
        with pytest.raises(FloatingPointError):
            graph.backward(r)


def test_training_step_with_trainable_encoder_matches_oracle_autograd():
    """LamTrainer(train_encoder=True) on the hf_tiny episode: loss, logits and EVERY parameter's gradient (encoder included) against
    the oracle's autograd.  The decoder of a random-weight model amplifies the encoder's 16-bit operand error (the frozen-encoder
    test holds the decoder gradients behind a HIP encoder to 1e-1 for the same reason); the encoder tensors sit behind it too."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from labelanything_amd.weights import init_state_dict
    from oracle import lam_oracle as O
    from oracle import loss_oracle as LO
    from tests.cases import CASES, geometry_for
    case = CASES["hf_tiny_1w1s_masks"]
    cfg = case["cfg"]
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    w = {k: v.clone().requires_grad_(v.is_floating_point() and "gaussian" not in k) for k, v in init_state_dict(cfg, case["weight_seed"]).items()}
    out = O.lam_forward(w, geometry_for(cfg), batch)
    loss, _ = LO.focal_objective(out["logits"], gt)
    loss.backward()
    ref_g = {k: v.grad for k, v in w.items() if v.requires_grad and v.grad is not None}
    lam = Lam(cfg, seed=case["weight_seed"]).cuda()
    tr = LamTrainer(lam, train_encoder=True)
    assert any(k.startswith("image_encoder.") for k in tr.names)
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - float(loss)) <= 1e-3 * max(1.0, abs(float(loss)))
    gmax = max(float(v.abs().max()) for v in ref_g.values())
    worst, cos = {}, {}
    for k, gv in zip(tr.names, tr.opt.grad_views):
        ref = ref_g.get(k)
        if ref is None:
            assert float(gv.abs().max()) == 0.0, k
            continue
        assert torch.isfinite(gv).all(), k
        mine = gv.cpu()
        worst[k] = float((mine - ref).abs().max()) / max(float(ref.abs().max()), 1e-2 * gmax)
        if float(ref.norm()) > 1e-3 * gmax * ref.numel() ** 0.5:
            cos[k] = float(torch.nn.functional.cosine_similarity(mine.flatten(), ref.flatten(), dim=0))
    enc = {k: v for k, v in worst.items() if k.startswith("image_encoder.")}
    print("trainable-encoder step: worst encoder tensors", sorted(enc.items(), key=lambda kv: -kv[1])[:5],
          "min cosine", min(cos.values()), min(cos, key=cos.get))
    assert len(enc) >= 30
    bad = {k: v for k, v in worst.items() if v > 1e-1}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert min(cos.values()) >= 0.995
    # and an optimizer step moves the encoder
    qw = dict(lam.named_parameters())["image_encoder.encoder.layer.0.attention.attention.query.weight"]
    before = qw.detach().clone()
    tr.apply_update()
    assert not torch.equal(before, qw.detach())


def test_backbone_lr_is_its_own_parameter_group():
    """The reference's ``backbone_lr`` branch (models/lam.py:340-346): the image encoder steps with its own rate, everything else with
    ``lr``; a frozen backbone with a backbone rate raises as in the reference."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from tests.cases import CASES
    case = CASES["hf_tiny_1w1s_masks"]
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    with pytest.raises(ValueError, match="freeze the backbone"):
        LamTrainer(Lam(case["cfg"], seed=3).cuda(), backbone_lr=1e-5)
    moved = {}
    for blr in (None, 1e-6):
        lam = Lam(case["cfg"], seed=3).cuda()
        tr = LamTrainer(lam, lr=1e-3, weight_decay=0.0, train_encoder=True, backbone_lr=blr)
        params = dict(lam.named_parameters())
        before = {k: params[k].detach().clone() for k in ("image_encoder.encoder.layer.0.attention.attention.query.weight",
                                                           "mask_decoder.output_upscaling.0.weight")}
        tr.step(batch, gt)
        moved[blr] = {k: float((params[k].detach() - v).abs().max()) for k, v in before.items()}
    enc, dec = "image_encoder.encoder.layer.0.attention.attention.query.weight", "mask_decoder.output_upscaling.0.weight"
    # the first AdamW step moves an entry with a gradient by ~ its learning rate
    assert 0.5e-3 <= moved[None][enc] <= 1.01e-3 and 0.5e-3 <= moved[None][dec] <= 1.01e-3, moved
    assert 0.5e-6 <= moved[1e-6][enc] <= 1.01e-6 and 0.5e-3 <= moved[1e-6][dec] <= 1.01e-3, moved


def test_steps_with_trainable_encoder_match_the_reference_fixture():
    """tests/golden/train_step_encoder.safetensors = the REFERENCE's WrapperModule + LabelAnythingLoss + torch AdamW + HF warm-up with
    NO frozen parameters (tools/make_golden_train.py, hf_tiny at 240 px): losses, per-tensor gradient norms of the first step, the
    full gradient and the final value of 13 tensors (10 of them inside the image encoder)."""
    import json
    import os
    from safetensors.torch import load_file
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from tests.cases import TRAIN_ENC_CASE as case
    from tests.helpers import GOLDEN, rel_err
    gold = load_file(os.path.join(GOLDEN, "train_step_encoder.safetensors"))
    with open(os.path.join(GOLDEN, "train_step_encoder.json")) as fh:
        keys = json.load(fh)["keys"]
    batch = make_episode(**case["episode"])
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    start = {k: p.detach().clone() for k, p in lam.named_parameters()}
    tr = LamTrainer(lam, lr=case["lr"], weight_decay=case["weight_decay"], num_warmup_steps=case["warmup"], train_encoder=True)
    assert sorted(tr.names) == keys
    losses = []
    for step in range(case["steps"]):
        tr.zero_grad()
        res = tr.forward_backward(batch, gold["gt"])
        losses.append(float(res["loss"]))
        if step == 0:
            assert rel_err(res["logits"], gold["logits0"]) <= 1e-3
            g0 = {k: gv.clone() for k, gv in zip(tr.names, tr.opt.grad_views)}
        tr.apply_update()
    assert torch.allclose(torch.tensor(losses), gold["loss"], rtol=2e-3, atol=0), (losses, gold["loss"])
    gn = torch.stack([g0[k].norm() for k in keys]).cpu()
    floor_g = 1e-2 * float(gold["grad_norm"].max())
    rel_n = (gn - gold["grad_norm"]).abs() / gold["grad_norm"].clamp_min(floor_g)
    print("trainable-encoder fixture: worst gradient-norm error", float(rel_n.max()), keys[int(rel_n.argmax())])
    # (a rounding-level change of the encoder forward moved this from 2e-3 to 1.2e-2 on one decoder bias: the decoder of a random-weight
    # model amplifies the 16-bit encoder error, as in tests/test_train_gpu.py's frozen-encoder bound)
    assert float(rel_n.max()) <= 3e-2
    params = dict(lam.named_parameters())
    gmax = max(float(v.abs().max()) for k, v in gold.items() if k.startswith("grad."))
    worst = 0.0
    for k, v in gold.items():
        if k.startswith("grad."):
            err = float((g0[k[5:]].cpu() - v).abs().max()) / max(float(v.abs().max()), 1e-2 * gmax)
            worst = max(worst, err)
            assert err <= 3e-2, (k, err)                     # measured 2.1e-3 (16-bit operands forward and backward)
        if k.startswith("final."):
            name = k[6:]
            mine, ref0 = params[name].detach().cpu(), start[name].cpu()
            sig = gold["grad." + name].abs() > 5e-2 * gold["grad." + name].abs().max()             # entries with a clear gradient
            step_ref, step_mine = (v - ref0)[sig], (mine - ref0)[sig]
            assert float((step_mine - step_ref).abs().max()) <= 5e-2 * float(step_ref.abs().max()), name
    print("trainable-encoder fixture: worst entry-wise gradient error", worst)


@pytest.mark.parametrize("shape", [(46852, 768, 768), (23426, 3072, 768), (5000, 128, 256), (900, 768, 3072)])
def test_split_k_weight_gradient_gemm_matches_torch(shape):
    """la_gemm with LaGemmEpilogue.ksplit on la_transpose16 operands: dW += dY^T X accumulated with fp32 atomics over K chunks."""
    r, n, k = shape
    g = torch.Generator().manual_seed(r + n)
    dy = torch.randn(r, n, generator=g).cuda()
    x = torch.randn(r, k, generator=g).half().cuda()
    rp = (r + 63) // 64 * 64
    dyt = torch.empty(n, rp, dtype=torch.float16, device="cuda")
    xt = torch.empty(k, rp, dtype=torch.float16, device="cuda")
    db0 = torch.randn(n, generator=g).cuda()
    db = db0.clone()
    L.transpose16(dy, dyt, colsum=db)                 # the bias gradient db += colsum(dY) from the same pass
    L.transpose16(x, xt)
    assert torch.equal(dyt[:, :r], dy.half().t()) and torch.equal(xt[:, :r], x.t())
    want = db0.double() + dy.half().double().sum(0)
    assert float((db.double() - want).abs().max()) <= 2e-5 * float(dy.half().double().abs().sum(0).max()), "fused column sums"
    assert rp == r or (float(dyt[:, r:].abs().max()) == 0.0 and float(xt[:, r:].abs().max()) == 0.0)
    dw0 = torch.randn(n, k, generator=g).cuda()
    dw = dw0.clone()
    L.gemm(dyt, xt, out32=dw, ksplit=1)
    torch.cuda.synchronize()
    ref = dw0.double() + dy.half().double().t() @ x.double()
    assert float((dw.double() - ref).abs().max() / ref.abs().max()) < 1e-5      # fp32 accumulation of exactly representable products


@pytest.mark.parametrize("shape", [(46852, 768, 768), (23426, 3072, 768), (5000, 256, 256), (901, 768, 3072), (130, 256, 512, "bf16"), (46852, 2304, 768, "group")])
def test_weight_gradient_from_row_major_16bit_operands_matches_torch(shape):
    """la_gemm_tn16: dW += dY^T X and db += colsum(dY) straight from the row-major 16-bit operands (LDS transpose reads feed both MFMA
    operands; no la_transpose16 copies), split over the rows with fp32 atomics.  Operands are column slices of wider matrices (as q | k | v
    gradients are), R is ragged (not a multiple of 64: the clamped tail rows must not count).  "group": the three [E, E] weight blocks of
    HF's separate query / key / value Linears a fixed number of rows apart, from ONE product (la_gemm's LA_MAP_GROUP)."""
    r, n, k = shape[:3]
    dt = torch.bfloat16 if "bf16" in shape else torch.float16
    g = torch.Generator().manual_seed(r + n)
    dy_wide = torch.full((r, n + 64), NAN, dtype=dt, device="cuda")          # the parents' other columns hold NaN
    x_wide = torch.full((r, k + 8), NAN, dtype=dt, device="cuda")
    dy_wide[:, 64:] = torch.randn(r, n, generator=g).to(dt).cuda()
    x_wide[:, :k] = torch.randn(r, k, generator=g).to(dt).cuda()
    dy, x = dy_wide[:, 64:], x_wide[:, :k]
    db0 = torch.randn(n, generator=g).cuda()
    db_buf, db = guarded(n)                                                  # dW and db between NaN guards
    db.copy_(db0)
    ref = dy.double().t() @ x.double()
    if "group" in shape:
        e, apart = n // 3, n // 3 + 5                  # E weight rows, then 5 rows of something else (the bias and alignment) before the next block
        buf0 = torch.randn(3 * apart, k, generator=g).cuda()
        buf_buf, buf = guarded(3 * apart, k)
        buf.copy_(buf0)
        L.gemm_tn16(dy, x, buf[:e], db=db, gsize=e, gstride=apart)
        check_guards(buf_buf, buf)
        for j in range(3):
            got = buf[j * apart: j * apart + e].double() - buf0[j * apart: j * apart + e].double()
            assert float((got - ref[j * e:(j + 1) * e]).abs().max() / ref.abs().max()) < 1e-5, j
            assert torch.equal(buf[j * apart + e:(j + 1) * apart], buf0[j * apart + e:(j + 1) * apart])         # rows in between untouched
    else:
        dw0 = torch.randn(n, k, generator=g).cuda()
        dw_buf, dw = guarded(n, k)
        dw.copy_(dw0)
        L.gemm_tn16(dy, x, dw, db=db)
        check_guards(dw_buf, dw)
        assert float((dw.double() - dw0.double() - ref).abs().max() / ref.abs().max()) < 1e-5      # fp32 accumulation of exactly representable products
    check_guards(db_buf, db)
    want = db0.double() + dy.double().sum(0)
    assert float((db.double() - want).abs().max()) <= 2e-5 * float(dy.double().abs().sum(0).max()), "fused column sums"


@pytest.mark.parametrize("shape", [(46852, 3072, 768), (16384, 3072, 768), (65636, 1024, 256, "bf16")])
def test_gelu_in_the_gemm_epilogue_forward_with_saved_pre_activation_and_backward(shape):
    """LaGemmEpilogue.aux16 (training forms of the MLP's GELU on the persistent four-wave kernel): ACT_GELU writes the pre-activation beside
    the activation in ONE launch - both bit-identical to what the plain and the GELU epilogue write alone; ACT_GELU_BWD multiplies the data
    gradient dY W by gelu'(saved pre-activation) in the epilogue - against torch in fp64 (models/common.py:36-37, erf GELU)."""
    m, n, k = shape[:3]
    dt = torch.bfloat16 if "bf16" in shape else torch.float16
    assert L.gemm_fused_act_ok(m, n, k) and not L.gemm_fused_act_ok(300, n, k) and not L.gemm_fused_act_ok(m, n + 64, k)
    g = torch.Generator().manual_seed(m + n)
    x = torch.randn(m, k, generator=g).to(dt).cuda()
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(dt).cuda()
    b = torch.randn(n, generator=g).cuda()
    pre, post = torch.empty(m, n, dtype=dt, device="cuda"), torch.empty(m, n, dtype=dt, device="cuda")
    L.gemm(x, w, bias=b, out16=post, act=L.ACT_GELU, aux16=pre)
    pre1, post1 = torch.empty_like(pre), torch.empty_like(post)
    L.gemm(x, w, bias=b, out16=pre1)
    L.gemm(x, w, bias=b, out16=post1, act=L.ACT_GELU)
    torch.cuda.synchronize()
    assert torch.equal(pre, pre1) and torch.equal(post, post1)
    rows = torch.randperm(m, generator=g)[:2048].cuda()
    ref_pre = x[rows].double() @ w.double().t() + b.double()
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    assert float((pre[rows].double() - ref_pre).abs().max()) <= eps * float(ref_pre.abs().max())
    ref_post = torch.nn.functional.gelu(ref_pre)
    assert float((post[rows].double() - ref_post).abs().max()) <= eps * float(ref_post.abs().max()) + 1e-4
    # backward: d pre = (dY W2) * gelu'(pre), W2 [k2, n] as the transposed weight [n, k2] of the data-gradient product
    k2 = k
    dy = torch.randn(m, k2, generator=g).to(dt).cuda()
    w2t = (torch.randn(n, k2, generator=g) * k2 ** -0.5).to(dt).cuda()
    dpre = torch.full((m, n), float("nan"), dtype=dt, device="cuda")
    L.gemm(dy, w2t, out16=dpre, act=L.ACT_GELU_BWD, aux16=pre)
    torch.cuda.synchronize()
    xs = pre[rows].double()
    gp = 0.5 * (1.0 + torch.erf(xs * 0.5 ** 0.5)) + xs * torch.exp(-0.5 * xs * xs) * (2.0 * math.pi) ** -0.5
    ref = (dy[rows].double() @ w2t.double().t()) * gp
    assert bool(torch.isfinite(dpre).all())
    assert float((dpre[rows].double() - ref).abs().max()) <= (eps + 1e-4) * float(ref.abs().max())
    # ... and the two-pass form it replaces (product in fp32, la_gelu_bwd16) agrees to the 16-bit rounding of the result
    dh = torch.empty(m, n, device="cuda")
    L.gemm(dy, w2t, out32=dh)
    two = torch.empty_like(dpre)
    L.gelu_bwd16(pre, dh, None, two)
    torch.cuda.synchronize()
    assert float((two.double() - dpre.double()).abs().max()) <= 2.0 * eps * float(ref.abs().max())


def test_trainer_leaves_the_models_inference_numerics_alone():
    """``LamTrainer(train_encoder=True)`` must not strip the token-mean correction groups from ``lam.precise`` - validation
    between training steps runs the SAME inference configuration as before; the training forward's own numerics live in the trainer's
    private encoder engine, which re-packs after every optimizer step (the second step must see the updated weights)."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from tests.cases import CASES
    case = CASES["hf_tiny_1w1s_masks"]
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    lam = Lam(case["cfg"], seed=3, precise=("patch", "vmean", "projmean", "neck")).cuda()
    before = tuple(lam.precise)
    ref = lam(batch)["logits"].clone()
    tr = LamTrainer(lam, lr=0.0, weight_decay=0.0, train_encoder=True)          # lr 0: the weights do not move
    assert tuple(lam.precise) == before and "vmean" not in tr.train_precise and "vmean" not in tr.enc_graph.precise
    l1 = float(tr.step(batch, gt)["loss"])
    assert tuple(lam.precise) == before
    assert torch.equal(lam(batch)["logits"], ref)                               # inference between steps: unchanged configuration
    eng1 = tr.enc_graph.engine()
    l2 = float(tr.step(batch, gt)["loss"])
    assert tr.enc_graph.engine() is eng1 and l1 == l2                           # same engine object, re-packed; same weights -> same loss
    tr2 = LamTrainer(Lam(case["cfg"], seed=3).cuda(), lr=1e-2, weight_decay=0.0, train_encoder=True)
    a = float(tr2.step(batch, gt)["loss"])
    b = float(tr2.step(batch, gt)["loss"])
    assert a != b                                                               # the second forward ran on re-packed (moved) weights


def test_bf16_training_through_the_encoder_as_baseline_cfg3_words_it():
    """BASELINE configs[2] says "bf16 training": the same graphs with bf16 MFMA operands (forward and backward; the loss scale stays a
    power of two, bf16 would not need one).  8 mantissa bits instead of 11 cost what they cost in the forward (4e-3 class):
    every encoder parameter's gradient of a linear functional against the oracle's autograd stays within 5e-2 of the tensor's largest
    entry (fp16: 1e-2), and a full optimizer step runs finite and moves the encoder."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from labelanything_amd.train_encoder import HfEncoderGraph
    from labelanything_amd.weights import init_state_dict
    from oracle import lam_oracle as O
    from tests.cases import CASES, geometry_for
    cfg = _hf_cfg(224)
    g = torch.Generator().manual_seed(224)
    images = torch.randn(3, 3, 224, 224, generator=g)
    sd = init_state_dict(cfg, 31)
    wref = {k: (v.clone().requires_grad_(True) if k.startswith("image_encoder.") and v.is_floating_point() else v) for k, v in sd.items()}
    out_ref = O.hf_vit_encoder(wref, geometry_for(cfg), images)
    r = torch.randn(out_ref.shape, generator=g)
    (out_ref * r).sum().backward()
    lam = Lam(cfg, seed=31, compute_dtype=torch.bfloat16).cuda()
    names = [k for k, p in lam.named_parameters() if k.startswith("image_encoder.")]
    grads = {k: torch.zeros_like(dict(lam.named_parameters())[k]) for k in names}
    graph = HfEncoderGraph(lam, grads)
    out = graph.forward(images.cuda())
    bn, c, gg, _ = out_ref.shape
    ref_rows = out_ref.detach().permute(0, 2, 3, 1).reshape(bn * gg * gg, c)
    f_err = float((out.cpu() - ref_rows).abs().max()) / float(ref_rows.abs().max())
    graph.backward(r.permute(0, 2, 3, 1).reshape(bn * gg * gg, c).contiguous().cuda())
    torch.cuda.synchronize()
    gmax = max(float(wref[k].grad.abs().max()) for k in names)
    worst = max(float((grads[k].cpu() - wref[k].grad).abs().max()) / max(float(wref[k].grad.abs().max()), 1e-2 * gmax) for k in names)
    print(f"bf16 encoder graph: forward {f_err:.2e}, worst parameter gradient {worst:.2e}")
    assert f_err <= 1e-2 and worst <= 5e-2, (f_err, worst)
    case = CASES["hf_tiny_1w1s_masks"]
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    lam2 = Lam(case["cfg"], seed=3, compute_dtype=torch.bfloat16).cuda()
    tr = LamTrainer(lam2, lr=1e-3, weight_decay=0.0, train_encoder=True)
    qw = dict(lam2.named_parameters())["image_encoder.encoder.layer.0.attention.attention.query.weight"]
    before = qw.detach().clone()
    res = tr.step(batch, gt)
    assert bool(torch.isfinite(res["loss"])) and bool(torch.isfinite(tr.opt.flat).all()) and not torch.equal(before, qw.detach())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [901 * 3072, 8 * 1000 + 3])
def test_gelu_forward_and_backward_on_16bit_rows_match_torch(dt, n):
    """la_gelu_fwd16 / la_gelu_bwd16 (8 elements per thread when the size allows, element-wise otherwise) against torch's erf GELU in fp64
    on the same 16-bit pre-activations."""
    from labelanything_amd import _lib as L
    g = torch.Generator().manual_seed(n % 97)
    pre = (torch.randn(n, generator=g) * 2).to(dt).cuda()
    dh = torch.randn(n, generator=g).cuda()
    d32, d16 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=dt)
    L.gelu_bwd16(pre, dh, d32, d16)
    x = pre.double().cpu().requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.backward(dh.double().cpu())
    assert float((d32.double().cpu() - x.grad).abs().max()) <= 2e-6 * float(x.grad.abs().max())
    assert torch.equal(d16, d32.to(dt))
    if n % 8 == 0:
        post = torch.empty_like(pre)
        L.gelu_fwd16(pre, post)
        assert torch.equal(post, y.detach().to(dt).cuda()) or float((post.double().cpu() - y.detach()).abs().max()) <= 2.0 ** -8 * float(y.abs().max())


def test_checkpoint_restore_between_steps_reaches_the_trainers_encoder():
    """the trainer's private encoder engine and its W^T copies follow the MODEL's ``weights_version`` - a checkpoint restore
    (``load_state_dict``) or a manual edit + ``lam.invalidate()`` after the first training step must reach the next training forward AND
    backward exactly as a fresh trainer on the same weights sees them."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from tests.cases import CASES
    case = CASES["hf_tiny_1w1s_masks"]
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    lam = Lam(case["cfg"], seed=3).cuda()
    tr = LamTrainer(lam, lr=1e-2, weight_decay=0.0, train_encoder=True)
    tr.step(batch, gt)                                                   # engine packed, W^T copies cached, weights moved
    other = Lam(case["cfg"], seed=7).cuda()
    lam.load_state_dict(other.state_dict())                              # "restore a checkpoint"
    tr.zero_grad()
    la = float(tr.forward_backward(batch, gt)["loss"])
    ga = tr.opt.grad.clone()
    fresh = LamTrainer(other, lr=1e-2, weight_decay=0.0, train_encoder=True)
    fresh.zero_grad()
    lb = float(fresh.forward_backward(batch, gt)["loss"])
    gb = fresh.opt.grad
    assert la == lb, (la, lb)                                            # the forward ran on the restored weights (deterministic kernels)
    assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())  # ... and so did the backward (fp32 atomics: order only)
    # manual edit + invalidate(): the documented out-of-band path
    with torch.no_grad():
        for p in lam.parameters():
            p.mul_(1.01)
    lam.invalidate()
    tr.zero_grad()
    lc = float(tr.forward_backward(batch, gt)["loss"])
    assert lc != la
    import labelanything_amd.autograd_ops as A
    assert A.WT is not tr._wt and A.SINK is not tr._sink                 # the trainer's W^T copies / gradient sink do not outlive the call


def test_decoder_graph_behind_the_trainable_encoder_is_exact_at_its_own_embeddings():
    """Why the end-to-end fixture bounds of the trainable-encoder steps are loose, without the looseness: the decoder of these
    random-weight models has ReLU kinks on a handful of token-side units, so its gradients are DISCONTINUOUS in the embeddings - the CPU
    oracle alone, with the encoder output perturbed by 3e-4 of its largest entry, moves a decoder-side gradient norm by 1e-3 for one noise
    seed and by 1e-1 for the next (tools/train_kink_study.py, profiles/r05_train_kink_study.log).  Evaluated AT THE SAME embeddings there is
    nothing loose: with the HIP encoder's own output handed to the oracle's autograd as the embeddings,
      * every decoder-side gradient (LAM neck, prompt encoder, mask decoder) agrees to 4e-4 of the largest gradient entry, and
      * the gradient the decoder graph hands to the encoder backward (d loss / d embeddings) agrees to 1e-3;
    the encoder's own backward is held to 1e-2 (measured 1e-3) by the linear-functional tests above."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from labelanything_amd.weights import init_state_dict
    from oracle import lam_oracle as O, loss_oracle as LO
    from tests.cases import TRAIN_ENC_CASE as case, geometry_for
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    tr = LamTrainer(lam, train_encoder=True)
    seen = {}
    fwd, bwd = tr.enc_graph.forward, tr.enc_graph.backward

    def spy_forward(images):
        out = fwd(images)
        seen["e"] = out.detach().clone()
        return out

    def spy_backward(g):
        seen["g"] = g.detach().clone()
        return bwd(g)

    tr.enc_graph.forward, tr.enc_graph.backward = spy_forward, spy_backward
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    im = batch["images"]
    b, n = im.shape[:2]
    gg = im.shape[-1] // lam.cfg.encoder_spec.patch
    e = seen["e"].float().cpu().view(b * n, gg, gg, -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True)     # (Bn, E, g, g) pre-neck
    w = {k: (v.clone().requires_grad_("image_encoder" not in k and "gaussian" not in k) if v.is_floating_point() else v)
         for k, v in init_state_dict(case["cfg"], case["weight_seed"]).items()}
    b2 = {k: v for k, v in batch.items() if k != "images"}
    b2["embeddings"] = e.view(b, n, *e.shape[1:])
    out = O.lam_forward(w, geometry_for(case["cfg"]), b2)
    loss, _ = LO.focal_objective(out["logits"], gt)
    loss.backward()
    assert abs(float(res["loss"]) - float(loss.detach())) <= 2e-6 * max(1.0, abs(float(loss.detach())))
    ref_g = {k: v.grad for k, v in w.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    gmax = max(float(v.abs().max()) for v in ref_g.values())
    worst = 0.0
    for k, gv in zip(tr.names, tr.opt.grad_views):
        if k in ref_g and not k.startswith("image_encoder."):
            err = float((gv.cpu() - ref_g[k]).abs().max()) / max(float(ref_g[k].abs().max()), 1e-2 * gmax)
            worst = max(worst, err)
            assert err <= 4e-4, (k, err)
    de_ref = e.grad.permute(0, 2, 3, 1).reshape(b * n * gg * gg, -1)
    de = seen["g"].float().cpu()
    derr = float((de - de_ref).abs().max()) / float(de_ref.abs().max())
    print(f"decoder graph at the HIP encoder's own embeddings: worst decoder-side gradient error {worst:.2e}, d loss / d embeddings {derr:.2e}")
    assert derr <= 1e-3
