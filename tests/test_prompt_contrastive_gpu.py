"""GPU: la_prompt_contrastive at the widths and row counts training runs with - D = 512 (the embed_dim of the configs that use the
term), D > 256 and n > 256 (the kernel's second and later register slices and its strided flag count), and the limits n = 1024,
D = 1024 - against the fp64 restatement (tests/loss_components_ref.py), the gradient row by row: one row lies below F.normalize's eps
and has a gradient of order 1e10, so a bound relative to the largest gradient of the whole tensor would leave every other row
unchecked.  The tolerance is that of tests/loss_profiles.py: the error of the fp32 restatement of the kernel on the same inputs,
against fp64 under the same measure, times its margin."""
import math

import pytest
import torch

from labelanything_amd.loss import LabelAnythingLoss
from tests import loss_components_ref as R
from tests import loss_profiles as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 3, 21, 512), (1, 5, 61, 1000), (2, 16, 64, 1024)])
def test_large_rows_and_widths_match_the_restatement(shape):
    b, m, c, d = shape
    g = torch.Generator().manual_seed(m * c + d)
    emb = torch.randn(b, m, c, d, generator=g)
    flags = (torch.rand(b, m, c, generator=g) < 0.85).to(torch.uint8)
    emb[0, 1, 2] *= 1e-14                                   # a row below F.normalize's eps
    emb[-1, 0] += 2.0                                       # correlated rows: large positive and negative margins
    crit = LabelAnythingLoss({"prompt_contrastive": {"weight": 1.0}}).cuda()
    pc = crit.prompt_components["prompt_contrastive"]
    with torch.no_grad():
        pc.t_prime.fill_(math.log(30.0))
        pc.bias.fill_(-7.0)
    e = emb.cuda().requires_grad_(True)
    res = crit({"logits": torch.zeros(b, 2, 4, 4, device="cuda"), "class_examples_embeddings": e, "flag_examples": flags.cuda()},
               torch.zeros(b, 4, 4, dtype=torch.long, device="cuda"))
    res["value"].backward()
    ed = emb.cuda().double().requires_grad_(True)
    tp = torch.tensor([math.log(30.0)], dtype=torch.float64, device="cuda", requires_grad=True)
    bs = torch.tensor([-7.0], dtype=torch.float64, device="cuda", requires_grad=True)
    ref = R.prompt_contrastive(ed, flags.cuda(), tp, bs)
    ref.backward()
    assert abs(float(res["value"]) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref))), (float(res["value"]), float(ref))
    assert torch.equal(res["components"]["prompt_contrastive"], res["value"])
    case = {"emb": emb, "flags": flags, "t_prime": torch.tensor([math.log(30.0)]), "bias": torch.tensor([-7.0])}
    want = {"demb": ed.grad.cpu(), "loss": float(ref.detach()), "dt": float(tp.grad), "db": float(bs.grad)}
    const = P.contrastive_figures(want, P.contrastive32(case))            # the fp32 restatement against fp64: no kernel in it
    got = {"demb": e.grad, "loss": float(res["value"]), "dt": float(pc.t_prime.grad), "db": float(pc.bias.grad)}
    for k, v in P.contrastive_figures(want, got).items():                 # d emb per row; the loss, d t' and d bias relatively
        print(f"{shape} {k}: {v:.3g}, restatement {const[k]:.3g}")
        assert v <= P.MARGIN * max(const[k], P.U), (k, v, const[k])
    rows = flags.reshape(b, m * c) == 0                     # unflagged rows get no gradient
    assert float(e.grad.reshape(b, m * c, d)[rows.cuda()].abs().max()) == 0.0 if bool(rows.any()) else True


def test_rows_beyond_the_limit_raise():
    crit = LabelAnythingLoss({"prompt_contrastive": {"weight": 1.0}}).cuda()
    with pytest.raises(RuntimeError, match="must be <="):
        crit({"logits": torch.zeros(1, 2, 4, 4, device="cuda"), "class_examples_embeddings": torch.randn(1, 17, 64, 8, device="cuda"),
              "flag_examples": torch.ones(1, 17, 64, device="cuda")}, torch.zeros(1, 4, 4, dtype=torch.long, device="cuda"))
