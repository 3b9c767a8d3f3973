"""CPU: the inputs of tests/test_attention_conditioning_gpu.py really have the score profiles they are named after, and a torch model of
the kernels' deferred-maximum online softmax shows why they are needed: four faults in the rescale step that leave the output on the
suite's older inputs (q, k ~ N(0, 1)) bit for bit unchanged move it by >= 10 x the tolerance on these.  No kernel runs here."""
import pytest
import torch

from tests import softmax_profiles as SP

FWD = SP.forward_cases()
BWD = SP.backward_cases()


def _uniq(cases):
    seen, out = set(), []
    for c in cases:
        fam, kind, t, g, hd, dt = c[:6]
        order = c[6] if len(c) > 8 else "linear"
        key = (kind, t, g, hd, dt, order)
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


PROFILES = _uniq(FWD + BWD)


@pytest.mark.parametrize("case", PROFILES, ids=lambda c: "-".join(str(x) for x in c))
def test_every_gpu_input_meets_its_profile_in_fp64(case):
    kind, t, g, hd, dt, order = case
    tmap = SP.tile_map(order, t, g)
    p = SP.build(kind, t, hd, dt, tmap, b=1 if t > 1000 else 2, heads=1 if t > 1000 else 2, g=g)
    for name in ("q", "k", "v"):
        assert torch.equal(SP.round_to(p[name], "f16" if (dt == "e4m3" and name == "v") else dt), p[name])
    fig = SP.check_built(p, tmap)
    print(f"profile {case}: {fig}")
    if kind == "bias" and g == 64:
        assert fig["rows_two_seams"] >= 256, "G = 64: the loud rows with qy + 41 < 64 meet two qualifying seams (the second step of the table)"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_pad_row_spike_of_the_image_order_windows(dt):
    print(SP.check_pad_spike(SP.build_image_windows(dt)))


def _model_case(kind, t, g, hd, dt, order):
    tmap = SP.tile_map(order, t, g)
    p = SP.build(kind, t, hd, dt, tmap, b=1, heads=1, g=g)
    s2 = SP.scores_log2(p)[0, 0]
    ref, lse = SP.attention(p["q"], p["k"], p["v"], p["scale"], g, p.get("tabh"), p.get("tabw"))
    sp, vp = SP.kernel_order(s2, p["v"][0, 0], order, g)
    return sp, vp, ref[0, 0], lse[0, 0]


def _err(o, ref):
    return float((o - ref).abs().max() / ref.abs().max())


MODEL_CASES = [(kind, t, g, hd, dt, order)
               for dt in ("f16", "bf16", "e4m3")
               for kind, t, g, hd, order in (("stairs", 200, 0, 64, "linear"), ("stairs", 256, 0, 64, "linear"), ("creep", 200, 0, 64, "linear"),
                                             ("creep", 256, 0, 64, "linear"), ("tail", 200, 0, 64, "linear"), ("stairs", 196, 14, 64, "win16"),
                                             ("tail", 196, 14, 64, "win16"), ("stairs", 200, 0, 128, "linear"))
               if not (dt == "e4m3" and (g or hd == 128))]


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_model_is_within_tolerance_and_every_fault_is_caught_at_ten_times_it(case):
    kind, t, g, hd, dt, order = case
    sp, vp, ref, lse = _model_case(*case)
    pdt = "f16" if dt == "e4m3" else dt
    tol = SP.TOL_FP8 if dt == "e4m3" else SP.TOL16[dt]
    o, l2, fired = SP.deferred_softmax_model(sp, vp, pdt)
    good = _err(o, ref)
    assert fired >= 1, "the deferred maximum never advanced after tile 0"
    assert good <= tol, good
    assert float((l2 - lse).abs().max()) <= SP.TOL_LSE
    errs = {}
    for fault in SP.FAULTS:
        of, _, _ = SP.deferred_softmax_model(sp, vp, pdt, fault)
        errs[fault] = _err(of, ref)
        assert errs[fault] >= 10 * tol, (fault, errs[fault])
    print(f"model {case}: correct {good:.2e} (bound {tol:.1e}), rescales after tile 0: {fired}, faulty", {k: f"{v:.2e}" for k, v in errs.items()})


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_every_fault_is_invisible_on_the_older_tests_input(dt):
    """q, k, v ~ N(0, 1) rounded to 16 bits, scale 1 / 8, T = 901 (tests/test_ops_gpu.py::test_attention_plain): after tile 0 no row
    outgrows its maximum by 2^8, the rescale never runs, and a kernel with any of the faults gives the same bits."""
    t, hd = 901, 64
    gen = torch.Generator().manual_seed(40)
    q, k, v = (SP.round_to(torch.randn(t, hd, generator=gen, dtype=torch.float64), dt) for _ in range(3))
    s2 = (q * 0.125) @ k.t() * SP.LOG2E
    sp, vp = SP.kernel_order(s2, v, "linear")
    o, _, fired = SP.deferred_softmax_model(sp, vp, dt)
    assert fired == 0
    ref = torch.softmax(s2 / SP.LOG2E, -1) @ v
    assert _err(o, ref) <= SP.TOL16[dt]
    for fault in SP.FAULTS:
        of, _, _ = SP.deferred_softmax_model(sp, vp, dt, fault)
        assert torch.equal(of, o), fault
    tmax, rise, _ = SP.seam_stats(s2, SP.tiles_linear(t))
    print(f"N(0, 1) input, {dt}: largest rise of a tile maximum over the earlier tiles {float(rise[:, 1:].max()):.2f} log2 units")
    assert float(rise[:, 1:].max()) < 8.0


def test_check_profile_refuses_a_benign_input():
    t = 256
    gen = torch.Generator().manual_seed(3)
    s2 = torch.randn(t, t, generator=gen, dtype=torch.float64) * SP.LOG2E
    for kind in ("stairs", "creep", "front"):
        with pytest.raises(AssertionError):
            SP.check_profile(s2, SP.tiles_linear(t), kind)
    with pytest.raises(AssertionError):
        SP.check_profile(s2[:200, :200], SP.tiles_linear(200), "tail")
