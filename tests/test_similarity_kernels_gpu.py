"""GPU: the three kernels of csrc/similarity.hip, each against the fp64 restatement of tests/similarity_ref.py, outputs in guarded buffers."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import similarity_ref as R
from tests.helpers import L, check_guards, guarded  # noqa: F401  (L: the fixture)

pytestmark = pytest.mark.gpu


# ---- la_sim_prepare -------------------------------------------------------------------------------------------------------------------
# fp16 rounding of a value in [-1, 1] is at most 2^-12 = 2.4e-4; the fp32 resample, norm and division add ~1e-6: 6e-4 absolute holds both
PREPARE_BOUND = 6e-4


@pytest.mark.parametrize("gin,cs,d", [(6, 16, 64), (6, 6, 64), (8, 24, 768), (6, 20, 384), (5, 9, 1024)])
def test_prepare_resamples_normalises_and_rounds(L, gin, cs, d):
    """la_sim_prepare against fp64 F.interpolate(bicubic) + F.normalize; three images, so that blocks cross image borders."""
    gen = torch.Generator().manual_seed(gin * 1000 + cs)
    x = torch.randn(3, gin * gin, d, generator=gen)
    if gin == cs:
        x[1, 7] = 0.0                         # F.normalize's clamp: 0 / max(0, 1e-12) = 0 exactly
    want = R.prepare(x.transpose(1, 2).reshape(3, d, gin, gin), None if gin == cs else cs)
    buf, out = guarded(3, cs * cs, d, dtype=torch.float16)
    L.sim_prepare(x.cuda(), gin, cs, out)
    check_guards(buf, out)
    got = out.cpu().double()
    err = float((got - want).abs().max())
    print(f"la_sim_prepare gin {gin} cs {cs} D {d}: max abs err {err:.3e} (bound {PREPARE_BOUND:.0e})")
    assert err <= PREPARE_BOUND
    assert float((got.norm(dim=2) - want.norm(dim=2)).abs().max()) <= 1e-3
    if gin == cs:
        assert bool((out[1, 7] == 0).all())


# ---- la_sim_class_bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,hm,wm,cs", [(3, 5, 37, 29, 20), (2, 3, 256, 256, 128), (2, 32, 16, 16, 16), (1, 1, 8, 8, 12), (2, 2, 12, 12, 24)])
def test_class_bits_are_exact(L, p, n, hm, wm, cs):
    """la_sim_class_bits against the restatement: non-binary mask values (0.3, -1), pixels in two classes, a support whose foreground
    covers everything (bit 0 nowhere), one that has none (bit 0 everywhere); the input's class 0 is noise that must not be read."""
    gen = torch.Generator().manual_seed(p * 100 + n)
    masks = torch.zeros(p, n, hm, wm)
    masks[:, 0] = torch.randn(p, hm, wm, generator=gen)
    if n > 1:
        draw = torch.rand(p, n - 1, hm, wm, generator=gen)
        masks[:, 1:] = torch.where(draw < 0.2, torch.full_like(draw, 0.3), torch.where(draw < 0.3, torch.full_like(draw, -1.0), torch.zeros_like(draw)))
        masks[0, 1] = 1.0                       # foreground everywhere
        masks[p - 1, 1:] = 0.0 if p > 1 else masks[p - 1, 1:]
    want = R.class_bits(masks, cs)
    buf, bits = guarded(p, cs * cs, dtype=torch.int32, fill=-7)
    L.sim_class_bits(masks.cuda(), cs, bits)
    check_guards(buf, bits, fill=-7)
    got = bits.cpu().long() & 0xFFFFFFFF
    assert torch.equal(got, want)
    if n > 1:
        assert not bool((got[0] & 1).any()) and (p == 1 or bool((got[p - 1] == 1).all()))
        two = (got >> 1)
        assert n < 3 or bool(((two & (two - 1)) != 0).any()), "no pixel in two classes: the case lost its point"


# ---- la_sim_max -----------------------------------------------------------------------------------------------------------------------
#        B   Q    K     D    N
CASES = [(1, 36, 36, 64, 2),            # below one tile
         (2, 81, 162, 64, 3),           # ragged Q and K, two supports
         (1, 256, 771, 384, 5),         # ragged K, overlapping classes, a key split with a short last share
         (1, 400, 1200, 1024, 2),       # widest D, key split
         (1, 130, 260, 768, 32)]        # all 32 bits: four passes of eight classes


@functools.lru_cache(maxsize=None)
def max_case(i):
    """(q16, k16, bits int32, fp64 reference [B, N, Q]) on the host.  Beside random membership every case holds the constructions its N
    has room for: a class whose only key is the very last row, one without a key, one that owns every key, runs of keys of one class
    (whole 32-key tiles of it, tiles without it, tiles it ends in), two identical keys (an exact tie), a query row identical to a key."""
    b, q, k, d, n = CASES[i]
    gen = torch.Generator().manual_seed(900 + i)
    q16 = F.normalize(torch.randn(b, q, d, generator=gen), dim=2).half()
    k16 = F.normalize(torch.randn(b, k, d, generator=gen), dim=2).half()
    k16[:, k // 3] = k16[:, k - 2]                                   # an exact tie between two keys
    q16[:, q // 2] = k16[:, k // 2]                                  # logit 1 (within the bound) for every class of that key
    member = torch.rand(b, k, n, generator=gen) < 0.3
    member[:, : k // 2, 0] = True                                    # runs: class 0 owns the first half, and random keys beyond
    member[:, k // 2, :] = True
    if n >= 3:
        member[:, :, n - 1] = False
        member[b - 1, k - 1, n - 1] = True                           # only the very last key row (no key at all in the batch items before)
        member[:, :, 1] = True                                       # owns every key
    if n >= 5:
        member[:, :, 3] = False                                      # no key
    if n == 2:
        member[:, :, 1] = False
        member[:, (2 * k) // 5:, 1] = True                           # a run that overlaps class 0's and ends at the last key
    words = (member.long() << torch.arange(n)).sum(dim=2)
    bits = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return q16, k16, bits, R.masked_max(q16, k16, words, n)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"case{i + 1}" for i in range(len(CASES))])
def test_masked_max_matches_fp64_on_the_same_operands(L, i):
    """la_sim_max (planned by la_sim_max_plan) against fp64 on the SAME fp16 operands: what is left is the fp32 accumulation, for unit rows
    at most gamma_D sum |q_i k_i| <= D 2^-24; asserted: D 2^-23 absolute (a factor 2 for the unspecified summation order).  The -inf
    pattern is exact, the workspace and the output stay inside their guards, and a second launch gives the same bits."""
    b, q, k, d, n = CASES[i]
    q16, k16, bits, want = max_case(i)
    ksplit, floats = L.sim_max_plan(b, q, k, d, n)
    assert (ksplit > 1) == (floats > 0) and floats in (0, ksplit * b * n * q)
    wbuf, work = guarded(max(floats, 1))
    buf, out = guarded(b, n, q)
    qd, kd, bd = q16.cuda(), k16.cuda(), bits.cuda()
    L.sim_max(qd, kd, bd, n, out, work=work)
    check_guards(buf, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wbuf[:64]).all()) and bool(torch.isnan(wbuf[64 + work.numel():]).all()), "workspace guards were overwritten"
    got = out.cpu().double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == float("-inf")).all()), "-inf pattern differs"
    assert bool((~fin).any()) == (n >= 3)
    bound = d * 2.0 ** -23
    err = float((got[fin] - want[fin]).abs().max())
    print(f"la_sim_max case {i + 1} {CASES[i]}: key split {ksplit}, max abs err {err:.3e} (bound D 2^-23 = {bound:.3e})")
    assert err <= bound
    assert float((got[:, 0, q // 2] - 1.0).abs().max()) <= bound + 2.0 ** -10      # the query that is a key: |k16|^2 = 1 up to fp16 rounding
    again = torch.full_like(out, float("nan"))
    L.sim_max(qd, kd, bd, n, again)
    assert torch.equal(again, out), "two launches differ"
