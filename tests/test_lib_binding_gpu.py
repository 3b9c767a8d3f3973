"""GPU: the binding's one call path (``_lib._call``) on real tensors - the device check reaches the tensors behind the first one, a checked
call still computes, and the stream a call is enqueued on is the current one."""
import pytest
import torch
from tests.helpers import L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24               # unit roundoff of fp32
P, HW, D = 2, 4, 8


@pytest.fixture(scope="module")
def x():
    return torch.randn(P, HW, D, generator=torch.Generator().manual_seed(77)).cuda()


def test_colmean_refuses_a_host_output_and_launches_nothing(L, x):
    """The host tensor is the fifth argument: before the table-driven call path only the first tensor of a wrapper was looked at, and
    la_colmean's not at all.  The first pass of the kernel writes ``scratch``, so an untouched scratch shows that nothing ran."""
    scratch = torch.full((P, L.COLMEAN_SPLIT, D), float("nan"), device="cuda")
    with pytest.raises(RuntimeError, match="device tensors"):
        L.colmean(x, P, HW, D, torch.zeros(P, D), scratch)
    torch.cuda.synchronize()
    assert bool(torch.isnan(scratch).all())


def test_colmean_on_device_tensors_gives_the_column_means(L, x):
    """Against the fp64 mean.  Bound: HW - 1 roundings in the sum and at most two in the scaling, each relative to a partial sum of at most
    sum |x|, over HW: (HW + 1) / HW * u * sum_i |x_i| per column."""
    out, scratch = torch.empty(P, D, device="cuda"), torch.empty(P, L.COLMEAN_SPLIT, D, device="cuda")
    L.colmean(x, P, HW, D, out, scratch)
    x64 = x.double().cpu()
    err = (out.double().cpu() - x64.mean(1)).abs()
    bound = (HW + 1) / HW * U * x64.abs().sum(1)
    print(f"colmean: max error {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())


def test_cast_runs_on_the_current_non_default_stream(L):
    """The stream is the last letter of a signature, appended by the call path: the 16-bit copy is complete once THAT stream is."""
    src = torch.randn(64, generator=torch.Generator().manual_seed(78)).cuda()
    dst = torch.full((64,), float("nan"), device="cuda", dtype=torch.float16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        L.cast(src, dst)
    side.synchronize()
    assert torch.equal(dst, src.half())
