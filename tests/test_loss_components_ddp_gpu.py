"""GPU, two processes on the ONE GPU of the box (gloo rendezvous), as tests/test_train_ddp_gpu.py: the data-parallel trainer with the
composite LabelAnythingLoss.  prompt_contrastive's t_prime / bias are in the decoder gradient bucket, so DDP all-reduces their
gradients and every rank ends the step with the same values."""
import os
import socket

import pytest
import torch

from labelanything_amd.episodes import make_episode
from tests.cases import TRAIN_CASE

pytestmark = pytest.mark.gpu
LOSS_KEYS = ("loss.prompt_components.prompt_contrastive.t_prime", "loss.prompt_components.prompt_contrastive.bias")


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank: int, world: int, port: int, out_dir: str):
    import torch.distributed as dist
    from labelanything_amd.loss import LabelAnythingLoss
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    lam = Lam(TRAIN_CASE["cfg"], seed=TRAIN_CASE["weight_seed"]).cuda()
    lam.selected_rows = torch.tensor([1, 4, 7])
    crit = LabelAnythingLoss({"focal": {"weight": 0.725}, "dice": {"weight": 0.025}, "prompt_contrastive": {"weight": 0.25}},
                             class_weighting=True)
    tr = LamTrainer(lam, lr=1e-3, weight_decay=1e-2, loss=crit)
    tr.opt.keep_reduced_grad = True
    ep = dict(TRAIN_CASE["episode"])
    ep.update(batch=1, seed=700 + rank)                          # each rank its own episode
    batch = make_episode(**ep)
    c = batch["flag_examples"].shape[2]
    g = torch.Generator().manual_seed(800 + rank)
    h, w = int(batch["dims"][0, 0, 0]), int(batch["dims"][0, 0, 1])
    gt = torch.randint(0, c, (1, h // 4, w // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    local = None
    orig = tr.reducer.launch

    def launch(i, *a, **k):                                       # this rank's own gradient of the loss parameters, before the SUM
        nonlocal local
        if i == tr._dec_bucket and local is None:
            local = torch.cat([tr.opt.grad_views[tr.names.index(n)].reshape(-1) for n in LOSS_KEYS]).cpu()
        return orig(i, *a, **k)

    tr.reducer.launch = launch
    res = tr.step(batch, gt)
    torch.cuda.synchronize()
    idx = [tr.names.index(n) for n in LOSS_KEYS]
    red = torch.cat([tr.opt.reduced_grad[sum(p.numel() for p in tr.opt.params[:i]):][:1] for i in idx]).cpu()
    torch.save({"params": torch.cat([p.detach().reshape(-1) for p in crit.parameters()]).cpu(), "reduced": red, "local": local,
                "steps": [tr.opt.tensor_steps[i] for i in idx], "loss": float(res["loss"])}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_end_the_step_with_identical_loss_parameters(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt") for r in range(world))
    assert r0["loss"] != r1["loss"]                               # the ranks did see different episodes
    assert torch.equal(r0["params"], r1["params"])
    assert torch.equal(r0["reduced"], r1["reduced"])              # the same (world-averaged) gradient on both ranks
    assert torch.allclose(r0["reduced"], (r0["local"] + r1["local"]) / 2, rtol=1e-6, atol=0)
    assert r0["steps"] == r1["steps"] == [1, 1]
    start = torch.tensor([2.302585092994046, -10.0])
    assert not torch.equal(r0["params"], start.float())
