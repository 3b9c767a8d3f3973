"""Query substitution on the device: the error-point sampler (la_error_count + la_error_points) against the reference's recorded draws
(tests/golden/substitution.*, tools/make_golden_substitution.py) and against a host restatement, the Substitutor's grown prompts,
graph capture, and LamTrainer.embed_batch / substitution_steps.

Host restatement (``host_points``): each (b, c)'s own error pixels in raster order (torch.nonzero), the k-th draw picking its rank,
coordinates scaled as torch_apply_coords does on 0-d tensors (float32 throughout).  The reference itself sorts its rows by
``b * B + c`` (experiment/substitution.py:83); where that key is not injective (B = 2 with C = 3, 4 and 6 here) its output can put
points on other (b, c), so those cases are checked against the restatement with the reference's draws."""
import json
import os
import types

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd.substitution import Substitutor, generate_points_from_errors
from tests.helpers import dataset_batch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "substitution")
META = json.load(open(GOLD + ".json"))["cases"]
T = load_file(GOLD + ".safetensors")
SAMPLED = sorted(n for n, c in META.items() if c["n"] > 0 and c["sub"])
f32 = np.float32


def scale_of(h, w, long_side=1024, custom=True):
    """torch_apply_coords on 0-d int64 tensors: every step a float32 op, x / t evaluated as reciprocal(t) * x."""
    if custom:
        sc = f32(f32(1) / f32(max(h, w))) * f32(long_side)
        nh, nw = int(f32(f32(h) * sc) + f32(0.5)), int(f32(f32(w) * sc) + f32(0.5))
    else:
        nh = nw = long_side
    return f32(f32(1) / f32(w)) * f32(nw), f32(f32(1) / f32(h)) * f32(nh)


def errors_of(logits, gt, ignore_index=-100):
    g = gt.clone()
    g[g == ignore_index] = 0
    p = logits.argmax(1)
    return p, g


def host_points(logits, gt, ranks, dims=None, long_side=1024, custom=True):
    logits, gt, ranks = logits.cpu().float(), gt.cpu(), ranks.cpu()
    B, C = logits.shape[:2]
    n = ranks.shape[2]
    p, g = errors_of(logits, gt)
    pts = np.zeros((B, C, n, 2), np.float32)
    lab = np.zeros((B, C, n), np.float32)
    for b in range(B):
        fx, fy = (f32(1), f32(1)) if dims is None else scale_of(int(dims[b, 0, 0]), int(dims[b, 0, 1]), long_side, custom)
        for c in range(C):
            err = (p[b] != g[b]) & ((g[b] == c) | (p[b] == c))
            yx = torch.nonzero(err)
            if yx.shape[0] == 0:
                continue
            for k in range(n):
                r = min(max(int(ranks[b, c, k]), 0), yx.shape[0] - 1)
                y, x = int(yx[r, 0]), int(yx[r, 1])
                pts[b, c, k] = (f32(x) * fx, f32(y) * fy)
                lab[b, c, k] = 0.0 if c == 0 else (1.0 if int(g[b, y, x]) == c else -1.0)
    return torch.from_numpy(pts), torch.from_numpy(lab)


def step_inputs(name, i):
    pre = f"{name}.step{i}."
    return (T[pre + "logits"].float().cuda(), T[pre + "gt"].cuda(), T[pre + "ranks"].cuda(), T[pre + "dims"],
            T[pre + "new_points"], T[pre + "new_labels"])


# ---- 1. the sampler with the recorded draws -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAMPLED)
def test_sampler_reproduces_the_reference_draws(name):
    cfg = META[name]
    kw = dict(long_side_length=cfg.get("long_side", 1024), custom_preprocess=cfg.get("custom", True))
    for i in range(len(cfg["steps"])):
        logits, gt, ranks, dims, ref_pts, ref_lab = step_inputs(name, i)
        pts, lab = generate_points_from_errors(logits, gt, cfg["n"], ranks=ranks, dims=dims.cuda(), **kw)
        hp, hl = host_points(logits, gt, ranks, dims, cfg.get("long_side", 1024), cfg.get("custom", True))
        assert torch.equal(pts.cpu(), hp) and torch.equal(lab.cpu(), hl), (name, i)
        if cfg["injective"]:
            assert torch.equal(pts.cpu(), ref_pts) and torch.equal(lab.cpu(), ref_lab), (name, i)


def test_non_injective_cases_are_where_the_reference_misplaces_points():
    # the restatement is the intent; the reference differs from it on at least one step of each case with a colliding key
    for name in ("b2_m4_c4_n1_nonin", "b2_m3_c6_n1_nonin", "b2_m3_c3_n1"):
        assert not META[name]["injective"]
        differs = False
        for i in range(len(META[name]["steps"])):
            logits, gt, ranks, dims, ref_pts, ref_lab = step_inputs(name, i)
            hp, hl = host_points(logits, gt, ranks, dims)
            differs |= not (torch.equal(hp, ref_pts) and torch.equal(hl, ref_lab))
        assert differs, name


@pytest.mark.parametrize("shape", [(3, 5, 300, 257), (2, 6, 1024, 1024), (1, 2, 1, 4097), (16, 3, 64, 48)])
def test_sampler_multi_tile_against_host(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + H)
    gt = torch.randint(0, C, (B, H, W), generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = -100
    logits = torch.randn(B, C, H, W, generator=g)
    logits.scatter_add_(1, gt.clamp(min=0).unsqueeze(1), torch.full((B, 1, H, W), 1.5))
    p, gg = errors_of(logits, gt)
    counts = torch.tensor([[int(((p[b] != gg[b]) & ((gg[b] == c) | (p[b] == c))).sum()) for c in range(C)] for b in range(B)])
    n = 3
    ranks = (torch.rand(B, C, n, generator=g) * counts.unsqueeze(-1).clamp(min=1)).to(torch.int32)
    ranks[..., -1] = (counts - 1).clamp(min=0).to(torch.int32)      # the last error pixel of every class
    dims = torch.tensor([[H, W]] * B).view(B, 1, 2)
    pts, lab = generate_points_from_errors(logits.cuda(), gt.cuda(), n, ranks=ranks.cuda(), dims=dims.cuda())
    hp, hl = host_points(logits, gt, ranks, dims)
    assert torch.equal(pts.cpu(), hp) and torch.equal(lab.cpu(), hl)


# ---- 2. the Substitutor's grown prompts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SAMPLED if META[n]["injective"]])
def test_substitutor_grows_prompts_like_the_reference(name):
    cfg = META[name]
    keys = ["embeddings", "prompt_points", "flag_points", "prompt_bboxes", "flag_bboxes", "prompt_masks", "flag_masks",
            "flag_examples", "dims"]
    batch = {k: T[f"{name}.in.{k}"].cuda() for k in keys}
    batch.update({k: cfg["steps"][0][k] for k in ("classes", "intended_classes")})
    sub = Substitutor(num_points=cfg["n"], long_side_length=cfg.get("long_side", 1024), custom_preprocess=cfg.get("custom", True))
    sub.reset(batch=(batch, T[f"{name}.in.gts"].cuda()))
    steps = 0
    for i, (inp, gt) in enumerate(sub):
        pre = f"{name}.step{i}."
        for k in ("prompt_points", "flag_points"):
            assert inp[k].dtype == T[pre + k].dtype and torch.equal(inp[k].cpu(), T[pre + k]), (name, i, k)
        assert torch.equal(gt.cpu(), T[pre + "gt"])
        sub.generate_new_points(T[pre + "logits"].float().cuda(), gt, ranks=T[pre + "ranks"].cuda())
        steps += 1
    assert steps == cfg["M1"] + 1
    assert sub.batch["prompt_points"].shape[3] == T[f"{name}.in.prompt_points"].shape[3] + steps * cfg["n"]


# ---- 3. device-drawn ranks ---------------------------------------------------------------------------------------------------
def test_device_draws_land_on_errors_of_their_sign():
    B, C, H, W, n = 4, 5, 200, 333, 3
    g = torch.Generator().manual_seed(7)
    gt = torch.randint(0, C - 1, (B, H, W), generator=g)
    gt[:, :10] = -100
    logits = torch.randn(B, C, H, W, generator=g)
    logits[1, 2] = -50          # class 2 of image 1: never predicted; present in the ground truth
    gt[2][gt[2] == 3] = 1       # class 3 of image 2: absent from the ground truth ...
    logits[2, 3] = -50          # ... and never predicted: no errors
    p, gg = errors_of(logits, gt)
    outs = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(1234)
        outs.append(generate_points_from_errors(logits.cuda(), gt.cuda(), n, generator=gen))
    pts, lab = outs[0]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    pts, lab = pts.cpu(), lab.cpu()
    assert torch.all(lab[:, 0] == 0)
    assert torch.all(lab[2, 3] == 0) and torch.all(pts[2, 3] == 0)
    for b in range(B):
        for c in range(1, C):
            for k in range(n):
                if b == 2 and c == 3:
                    continue
                x, y = int(pts[b, c, k, 0]), int(pts[b, c, k, 1])
                assert float(pts[b, c, k, 0]) == x and float(pts[b, c, k, 1]) == y
                want = 1.0 if int(gg[b, y, x]) == c and int(p[b, y, x]) != c else (-1.0 if int(p[b, y, x]) == c and int(gg[b, y, x]) != c else 0.0)
                assert want != 0.0 and float(lab[b, c, k]) == want, (b, c, k)
    assert torch.all(lab[1, 2] == 1)                                   # only false negatives exist for it
    other = generate_points_from_errors(logits.cuda(), gt.cuda(), n, generator=torch.Generator(device="cuda").manual_seed(99))
    assert not torch.equal(other[0], outs[0][0])


# ---- 4. graph capture ---------------------------------------------------------------------------------------------------------
def test_sampler_replays_in_a_captured_graph():
    B, C, H, W, n = 2, 4, 257, 300, 2
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, C, H, W, generator=g).cuda()
    gt = torch.randint(0, C, (B, H, W), generator=g).cuda()
    dims = torch.tensor([[[500, 375]], [[333, 2048]]]).cuda()
    u = torch.rand(B, C, n, generator=g).cuda()
    preds = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
    ref = generate_points_from_errors(logits, gt, n, u=u, dims=dims)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                   # warm-up on the capture stream
        generate_points_from_errors(logits, gt, n, u=u, dims=dims, preds_out=preds)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = generate_points_from_errors(logits, gt, n, u=u, dims=dims, preds_out=preds)
    preds.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    assert torch.equal(preds, torch.argmax(logits, 1))
    u.copy_(torch.rand(B, C, n, generator=g).cuda())              # new draws through the same graph
    graph.replay()
    again = generate_points_from_errors(logits, gt, n, u=u, dims=dims)
    torch.cuda.synchronize()
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])


# ---- 5. the argmax output ------------------------------------------------------------------------------------------------------
def test_preds_out_is_torch_argmax():
    g = torch.Generator().manual_seed(3)
    logits = torch.randint(-2, 3, (3, 6, 130, 70), generator=g).float()      # many ties: first maximal index
    logits[0, :, 5, 5] = float("-inf")
    gt = torch.randint(0, 6, (3, 130, 70), generator=g)
    preds = torch.full((3, 130, 70), -1, dtype=torch.int64, device="cuda")
    generate_points_from_errors(logits.cuda(), gt.cuda(), 1, preds_out=preds)
    assert torch.equal(preds.cpu(), torch.argmax(logits, 1))
    preds.fill_(-1)
    generate_points_from_errors(logits.cuda(), gt.cuda(), 0, preds_out=preds)
    assert torch.equal(preds.cpu(), torch.argmax(logits, 1))


# ---- 6 - 8. the trainer ----------------------------------------------------------------------------------------------------------
def make_trainer(case, rows, **kw):
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    lam.selected_rows = rows
    return LamTrainer(lam, **kw)


def test_embed_batch_is_bit_identical_to_images():
    from tests.cases import CASES
    from labelanything_amd.episodes import make_episode
    case = CASES["sam_tiny_2w2s_all_prompts"]
    batch = make_episode(**case["episode"])
    gt = dataset_batch(case, seed=2)[1][:, 0]
    rows = torch.tensor([0, 3, 7])
    ta, tb = make_trainer(case, rows, lr=1e-3), make_trainer(case, rows, lr=1e-3)
    emb = tb.embed_batch(batch)
    assert "images" not in emb and emb["embeddings"].shape[:2] == batch["images"].shape[:2]
    ta.zero_grad()
    tb.zero_grad()
    ra, rb = ta.forward_backward(batch, gt, sync=True), tb.forward_backward(emb, gt, sync=True)
    torch.cuda.synchronize()
    assert torch.equal(ra["loss"], rb["loss"]) and torch.equal(ra["logits"], rb["logits"])
    adopt_gradient(tb, ta.opt.grad)
    ta.apply_update()
    tb.apply_update()
    for (k, pa), (_, pb) in zip(ta.lam.named_parameters(), tb.lam.named_parameters()):
        assert torch.equal(pa, pb), k
    with pytest.raises(ValueError):
        type(ta).embed_batch(types.SimpleNamespace(train_encoder=True), batch)


# Two backward passes over the same forward differ in the last bits: the weight-gradient reductions add with float atomics in a
# run-dependent order (the forward is deterministic: loss and logits are compared bit for bit).  That rounding scales with the summed
# terms, not with the result, so it does not shrink with a gradient that cancels.  Measured on the MI355X for the novit_d256_2w3s
# model over 18 pairs of identical backward passes: the largest element difference was 1.2e-7 ... 6.8e-7 in absolute terms, at
# 2e-5 of the gradient's largest element for steps whose gradient reaches 3.5e-2 and 1.9e-3 of it for a step whose gradient only
# reaches 6.6e-5.  The bound is GRAD_ABS (15x the worst absolute difference) plus GRAD_REL of the gradient's largest element (50x the
# worst relative one of the large gradients).  What these tests must catch is far larger: a wrong loss normaliser or one of the M+2
# accumulated steps missing moves the gradient by a sizeable fraction of its largest element.
GRAD_ABS, GRAD_REL = 1e-5, 1e-3


def adopt_gradient(tr, grad):
    """Check that ``tr``'s flat gradient agrees with ``grad`` to atomic-order rounding, then adopt ``grad`` bit for bit, so that the
    optimizer step that follows - deterministic and element-wise - must reproduce the other trainer's parameters exactly."""
    diff = float((tr.opt.grad - grad).abs().max())
    assert diff <= GRAD_ABS + GRAD_REL * float(grad.abs().max()), (diff, float(grad.abs().max()))
    tr.opt.grad.copy_(grad)


class HostSubstitution:
    """The test's own restatement of the substitution loop: rotations composed on the host, error points by ``host_points`` with
    ranks from the same device uniforms (rank = min(floor(u * count), count - 1))."""

    def __init__(self, batch, gts, n, gen_seed, long_side):
        self.long_side = long_side
        self.batch = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        self.gts = gts.clone()
        self.n = n
        self.gen = torch.Generator(device="cuda").manual_seed(gen_seed)
        self.m1 = batch["embeddings"].shape[1]

    def steps(self):
        sep = ("prompt_points", "prompt_masks", "prompt_bboxes", "flag_masks", "flag_bboxes", "flag_points", "flag_examples")
        for it in range(self.m1 + 1):
            if it > 0:
                order = ([self.m1 - 1] + list(range(1, self.m1 - 1)) + [0]) if it == self.m1 else \
                    [it] + list(range(it)) + list(range(it + 1, self.m1))
                for k in list(sep) + ["dims", "embeddings"]:
                    if k in self.batch:
                        self.batch[k] = self.batch[k][:, order]
                self.gts = self.gts[:, order]
            yield {k: (v[:, 1:] if k in sep else v) for k, v in self.batch.items()}, self.gts[:, 0]

    def add_points(self, logits, gt):
        B, C = logits.shape[:2]
        u = torch.rand(B, C, self.n, generator=self.gen, device="cuda").cpu()
        p, g = errors_of(logits.cpu(), gt.cpu())
        counts = torch.tensor([[int(((p[b] != g[b]) & ((g[b] == c) | (p[b] == c))).sum()) for c in range(C)] for b in range(B)])
        ranks = torch.minimum(torch.floor(u.double() * counts.unsqueeze(-1)), (counts.unsqueeze(-1) - 1).clamp(min=0)).to(torch.int32)
        pts, lab = host_points(logits, gt, ranks, self.batch["dims"].cpu(), self.long_side)
        pp, fp = self.batch["prompt_points"], self.batch["flag_points"]
        newp = torch.zeros(B, pp.shape[1], C, self.n, 2)
        newp[:, 0] = pts
        newl = torch.zeros(B, fp.shape[1], C, self.n)
        newl[:, 0] = lab
        self.batch["prompt_points"] = torch.cat([pp, newp.to(pp.device)], 3)
        self.batch["flag_points"] = torch.cat([fp, newl.to(fp.device)], 3)


@pytest.mark.parametrize("accumulate", [False, True])
def test_substitution_steps_match_a_host_driven_loop(accumulate):
    """substitution_steps against the test's own loop over the same batch: per step the same model input, loss, logits (bit for
    bit) and the same gradient (to atomic-order rounding, see GRAD_ABS / GRAD_REL); every update of the host loop adopts the gradient the
    product's update used, so the weights - which do move (lr > 0) - stay bit-identical from step to step and at the end."""
    from tests.cases import CASES
    case = CASES["novit_d256_2w3s"]
    batch, gts = dataset_batch(case, seed=4)
    rows = torch.tensor([0, 5, 9])
    n = 2
    ta = make_trainer(case, rows, lr=1e-3)
    initial = [p.detach().clone() for p in ta.lam.parameters()]
    sub = Substitutor(num_points=n, long_side_length=256, generator=torch.Generator(device="cuda").manual_seed(77))
    used = []                                                   # the gradient of every optimizer step of the product's loop
    orig = ta.opt.step
    ta.opt.step = lambda *a, **k: (used.append(ta.opt.grad.clone()), orig(*a, **k))[1]
    got = list(ta.substitution_steps(batch, gts, sub, accumulate=accumulate))
    m1 = batch["embeddings"].shape[1]
    assert len(got) == m1 + 1
    assert len(used) == (1 if accumulate else m1 + 1)

    tb = make_trainer(case, rows, lr=1e-3)
    host = HostSubstitution(batch, gts, n, 77, 256)
    norm = float(m1 + 1) if accumulate else 1.0
    updates = 0
    for i, (inp, gt) in enumerate(host.steps()):
        g = got[i]
        for k, v in inp.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(g["input"][k].cpu(), v.cpu()), (i, k)
        assert torch.equal(g["gt"].cpu(), gt.cpu())
        if not accumulate or i == 0:
            tb.zero_grad()
        res = tb.forward_backward(inp, gt, norm, sync=not accumulate or i == m1)
        if not accumulate or i == m1:
            adopt_gradient(tb, used[updates])
            tb.apply_update()
            updates += 1
        assert torch.equal(res["loss"], g["loss"]) and torch.equal(res["logits"], g["logits"]), i
        assert torch.equal(g["preds"], torch.argmax(g["logits"], 1))
        host.add_points(res["logits"], gt)
    assert updates == len(used)
    moved = False
    for (k, pa), (_, pb), p0 in zip(ta.lam.named_parameters(), tb.lam.named_parameters(), initial):
        assert torch.equal(pa, pb), k
        moved |= not torch.equal(pa, p0)
    assert moved                                                # the comparison above is not one of untouched weights


def test_mask_only_episode_trains_through_every_step():
    from tests.cases import CASES
    case = CASES["novit_d256_2w3s"]
    batch, gts = dataset_batch(case, seed=6, prompts=("mask",))
    assert not batch["flag_points"].any()
    tr = make_trainer(case, torch.tensor([1, 2, 3]), lr=1e-3)
    sub = Substitutor(num_points=1, long_side_length=256, generator=torch.Generator(device="cuda").manual_seed(3))
    seen = []
    for r in tr.substitution_steps(batch, gts, sub):
        assert torch.isfinite(r["loss"])
        seen.append((int(r["input"]["prompt_points"].shape[3]), bool(r["input"]["flag_points"].ne(0).any())))
    m1 = batch["embeddings"].shape[1]
    assert len(seen) == m1 + 1
    assert [s[0] for s in seen] == [seen[0][0] + i for i in range(m1 + 1)]      # the point dimension grows by num_points every step
    assert not seen[0][1] and all(s[1] for s in seen[1:])                # points appear once a former query is a support
