"""GPU: every launch that tests/test_gemm_plan_cpu.py::TABLE plans is RUN, between guards and on padded strides, against the float64
contract of la_gemm (tests/gemm_ref.py), plus the cells the table does not hold (each family at its smallest shape with two outputs,
a periodic residual and the four row maps, fp16 and bf16).

Rows run at the table's own M - a launch is milliseconds - except where M N K exceeds SHRINK_ABOVE (lin1_group_m_8): such a row runs at
the smallest M for which la_gemm_plan on this device (ncu = 0: its own CU count) returns the same kernel, epi, planes, direct, ragged,
gm, ksplit.  Each case runs with the default pads of gemm_ref.PADS and once more in the row's own layout, and
prints its family and max(err / allowance) under -s.  An error of la_gemm_plan on any of these cases is a failure.  The cells la_gemm
must refuse stand apart in REFUSED, as (literal message, name, call) like ERRORS of test_gemm_plan_cpu.py: la_gemm_plan and la_gemm
itself, called on real guarded operands, must both raise that message and leave every output arena untouched.  The two rows whose
operands span 4 GiB run only with 12 GiB free (the rule of test_epilogue_reaches_rows_beyond_four_gigabytes).
"""
import math

import pytest
import torch

from tests import gemm_ref as R
from tests.helpers import L
from tests.test_gemm_plan_cpu import A, BF16, BIAS, BIG, F16, F32, NSO, O16, O32, RES, RVEC, TABLE, VT, W, call

TORCH_DT = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}
NEEDS_12GIB = ("a_over_4gib", "w_over_4gib")
PLAN_KEY = ("kernel", "epi", "planes", "direct", "ragged", "gm", "ksplit")
SHRINK_ABOVE = 1e11          # M N K: beyond it the float64 reference, not the launch, would take seconds
INT_KEYS = ("act", "map", "p", "res_mod", "a_kmod", "ksplit", "vt_col0", "vt_T", "vt_Tpad", "vt_hd", "vt_heads", "vt_ws", "amap", "rvec_rpg")
LD_KEYS = ("ldr", "ld32", "ld16", "ldaux")


# ---- the cells TABLE does not hold ----------------------------------------------------------------------------------------------
def _geometry(kind, m, n):
    """Row map of one kind fitted to about m rows: (rows, epilogue keywords)."""
    big = m >= 8192
    if kind == "group":
        p0 = 4096 if big else max(2, m // 3)
        return m, dict(map=R.MAP_GROUP, p=(p0, p0 + 1, 1, 0, 0))
    if kind == "merge":
        ws, nw, h = (16, 4, 60) if big else ((4, 2, 7) if m >= 64 else (2, 2, 3))
        per = nw * nw * ws * ws
        return m // per * per, dict(map=R.MAP_WINDOW_MERGE, p=(ws, nw, nw, h, h))
    if kind == "part":
        ws, nw, h = (14, 5, 64) if big else ((4, 2, 7) if m >= 49 else (2, 2, 3))
        return m // (h * h) * h * h, dict(map=R.MAP_WINDOW_PART, p=(ws, nw, nw, h, h))
    g = 64 if big else 4
    return m, dict(map=R.MAP_CONVT2X2, p=(g, g, n // 4, 0, 0))


def _extra_cells():
    cells = []

    def add(name, c):
        cells.append((name, c))

    shapes16 = [("NT", 77, 40, 288, {}), ("DMA128", 33, 256, 256, {}), ("DMA128", 300, 200, 768, {}), ("SKINNY", 32, 256, 256, {}),
                ("DMA256x128", 65536, 256, 128, {}), ("T256", 131072, 128, 256, {}), ("T256P", 32768, 256, 512, dict(a_kmod=256)),
                ("T256W", 131072, 256, 256, {})]
    shapes32 = [("SKINNY", 20, 256, 2048), ("F32_SMALL", 129, 256, 256), ("F32_N128", 513, 256, 256), ("F32_N128", 1024, 36, 256),
                ("F32_N32", 1024, 32, 256)]
    for fam, m, n, k, kw in shapes16:
        for dt in (F16, BF16):
            tag = f"{fam}_{m}x{n}x{k}_{'f16' if dt == F16 else 'bf16'}"
            lda = kw.get("a_kmod")
            add(f"{tag}_bias16", call(m, n, k, dt=dt, lda=lda, bias=BIAS, out16=O16, **kw))
            rm = 256 if (m % 256 == 0 and m >= 512) else 16
            add(f"{tag}_res_mod_two_outputs", call(m, n, k, dt=dt, lda=lda, bias=BIAS, res=RES, res_mod=rm, out32=O32, out16=O16, **kw))
            add(f"{tag}_gelu_res_two_outputs", call(m, n, k, dt=dt, lda=lda, bias=BIAS, res=RES, out32=O32, out16=O16, act=R.ACT_GELU, **kw))
            for kind in ("group", "merge", "convt", "part"):
                mm, g = _geometry(kind, m, n)
                if kind == "group":
                    add(f"{tag}_map_{kind}", call(mm, n, k, dt=dt, lda=lda, res=RES, res_mod=g["p"][1], out32=O32, **g, **kw))
                else:
                    add(f"{tag}_map_{kind}", call(mm, n, k, dt=dt, lda=lda, bias=BIAS, out16=O16, **g, **kw))
            mm, g = _geometry("part", m, n)                # amap: the rows gathered from window order (the proj GEMM of a window block)
            add(f"{tag}_amap_part_res_in_place", call(mm, n, k, dt=dt, lda=lda, bias=BIAS, res=O32, out32=O32, amap=g["map"], p=g["p"], **kw))
            add(f"{tag}_res_in_place_two_outputs", call(m, n, k, dt=dt, lda=lda, bias=BIAS, res=O32, out32=O32, out16=O16, **kw))
            if fam == "NT":
                add(f"{tag}_ld16_44", call(m, n, k, dt=dt, bias=BIAS, out16=O16, ld16=44))
            if fam == "T256":
                add(f"{tag}_relu", call(m, n, k, dt=dt, bias=BIAS, out16=O16, act=R.ACT_RELU))
    for m in (4096, 4096 + 8):                             # the producer of a folded LayerNorm on the stream it reads: whole tiles and a ragged tail
        add(f"T256W_{m}x256x256_f16_producer_in_place_rvec192",
            call(m, 256, 256, bias=BIAS, res=O32, out32=O32, out16=O16, nstat_out=NSO, rvec=RVEC, rvec_rpg=192))
    for fam, m, n, k in shapes32:
        tag = f"{fam}_{m}x{n}x{k}_f32"
        add(f"{tag}_bias32", call(m, n, k, dt=F32, bias=BIAS, out32=O32))
        add(f"{tag}_res_mod", call(m, n, k, dt=F32, bias=BIAS, res=RES, res_mod=16, out32=O32))
        add(f"{tag}_gelu_res", call(m, n, k, dt=F32, bias=BIAS, res=RES, out32=O32, act=R.ACT_GELU))
        for kind in ("group", "merge", "convt", "part"):
            mm, g = _geometry(kind, m, n)
            add(f"{tag}_map_{kind}", call(mm, n, k, dt=F32, bias=BIAS, out32=O32, **g))
    for dt in (F16, BF16):
        tag = f"T256Q_128x256x5056_{'f16' if dt == F16 else 'bf16'}_ksplit"
        add(f"{tag}_onto_nonzero", call(128, 256, 5056, dt=dt, out32=O32, ksplit=1))
        add(f"{tag}_map_group", call(128, 256, 5056, dt=dt, out32=O32, ksplit=1, map=R.MAP_GROUP, p=(64, 96, 8, 0, 0)))
    # V^T in the 16-wide slot order of window attention (vt_ws): the qkv GEMM of 14- and 8-wide windows at few rows, and the window
    # partition of 64 x 64 maps into 14-wide windows on the 256 x 256 slab
    for dt in (F16, BF16):
        tag = "f16" if dt == F16 else "bf16"
        for g in (14, 8):
            add(f"vt_ws{g}_{5 * g * g}x384x128_{tag}", call(5 * g * g, 384, 128, dt=dt, bias=BIAS, out16=O16, vt=VT, vt_col0=256, vt_T=g * g,
                                                          vt_Tpad=(16 * g + 63) // 64 * 64, vt_hd=64, vt_heads=2, vt_ws=g))
        mm, geo = _geometry("part", BIG, 512)
        add(f"vt_ws14_part_slab_{mm}x512x256_{tag}", call(mm, 512, 256, dt=dt, bias=BIAS, out16=O16, vt=VT, vt_col0=256, vt_T=196, vt_Tpad=256,
                                                         vt_hd=64, vt_heads=4, vt_ws=14, **geo))
    return cells


def _refused_cells():
    """(literal message of la_gemm, name, call): what each family must refuse of the cells above."""
    bare = "ksplit accumulates the bare product into out32 (no bias / residual / activation / second output; row map none or LA_MAP_GROUP)"
    cells = []
    for dt in (F16, BF16):
        tag = f"T256Q_128x256x5056_{'f16' if dt == F16 else 'bf16'}_ksplit"
        q = dict(dt=dt, out32=O32, ksplit=1)
        cells.append((bare, f"{tag}_with_bias", call(128, 256, 5056, bias=BIAS, **q)))
        cells.append((bare, f"{tag}_res_mod", call(128, 256, 5056, res=RES, res_mod=16, **q)))
        cells.append((bare, f"{tag}_two_outputs", call(128, 256, 5056, out16=O16, **q)))
        for kind in ("merge", "convt", "part"):
            mm, geo = _geometry(kind, 128, 256)
            cells.append((bare, f"{tag}_map_{kind}", call(mm, 256, 5056, **geo, **q)))
    return cells


TABLE_NAMES = [t[0] for t in TABLE]
TABLE_ROWS = {t[0]: (t[1], t[2]) for t in TABLE}
EXTRA = _extra_cells()
EXTRA_ROWS = dict(EXTRA)
REFUSED = _refused_cells()
REFUSED_ROWS = {name: (text, c) for text, name, c in REFUSED}


# ---- a planned call turned into operands ----------------------------------------------------------------------------------------
def build(c, device, m=None, seed=0):
    """Compact operands of a ``call`` of test_gemm_plan_cpu: (a, w, epilogue, lds, a_elem_off).  The key set of c["epi"] says which buffers
    exist; inputs are the suite's: N(0, 1) rounded to the operand type, W / sqrt(K), seeded."""
    m = c["m"] if m is None else m
    n, k, e = c["n"], c["k"], c["epi"]
    td = TORCH_DT[c["dt"]]
    gen = torch.Generator(device=device).manual_seed(1000 + seed)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen, device=device) * scale

    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=device)

    akm = e.get("a_kmod", 0)
    ka = akm or k
    geo = {key: e[key] for key in ("map", "p") if key in e}
    arows = int(R.map_rows(e["amap"], e["p"], torch.arange(m)).max()) + 1 if e.get("amap") else m
    a = rnd(arows, ka).to(td)
    w = (rnd(n, k) / math.sqrt(k)).to(td)
    drows = R.dest_rows(m, geo)
    cols = e["p"][2] if e.get("map") == R.MAP_CONVT2X2 else n
    out = {key: e[key] for key in INT_KEYS if key in e}
    lds = {key: e[key] for key in LD_KEYS if key in e}
    if c["lda"] > ka:
        lds["lda"] = c["lda"]
    if c["ldw"] > k:
        lds["ldw"] = c["ldw"]
    inplace = "nstat_out" in e and "out32" not in e and "res" not in e
    if "bias" in e:
        out["bias"] = rnd(cols)
    if "res" in e:
        out["res"] = rnd(e.get("res_mod") or drows, cols)
    if "out32" in e:
        out["out32"] = rnd(drows, cols) if e.get("ksplit") else zeros(drows, cols)
    if "out16" in e:
        out["out16"] = zeros(drows, cols, dtype=td)
    if "aux16" in e:
        out["aux16"] = rnd(m, n).to(td) if e.get("act") == R.ACT_GELU_BWD else zeros(m, n, dtype=td)
    if inplace:
        x0 = rnd(m, n, scale=3.0)
        out["out16"] = x0.to(td)
        out["aux16"] = (x0 - out["out16"].float()).to(td)
    if "vt" in e:
        out["vt"] = zeros(-(-drows // e["vt_T"]) * e["vt_heads"] * e["vt_hd"], e["vt_Tpad"], dtype=td)
    if "nstat_out" in e:
        out["nstat_out"] = zeros(m, n // 64, 2)
    if "rvec" in e:
        out["rvec"] = rnd(-(-m // e["rvec_rpg"]), n, scale=0.3)
    if "nstat_in" in e:
        mr = zeros(-(-m // 256) * 256, 2)
        mr[:m, 0] = rnd(m, scale=0.2)
        mr[:m, 1] = 0.5 + rnd(m).abs()
        out["nstat_in"] = mr
    if "ncol" in e:
        out["ncol"] = rnd(n)
    if "res" in e and e["res"] == e.get("out32"):          # one address: the residual stream is updated in place
        out["out32"] = out["res"] = rnd(drows, cols)
    off = (c["a"] - A) // (4 if td == torch.float32 else 2)
    return a, w, out, lds, off


def _plan(L, c, m, pads=None):
    """The device's plan of the call as written (fake addresses, ncu = 0), with ``pads`` added to the leading dimensions it does not fix."""
    e = dict(c["epi"])
    n, k = c["n"], c["k"]
    ka = e.get("a_kmod") or k
    lda, ldw = c["lda"], c["ldw"]
    if pads:
        cols = e["p"][2] if e.get("map") == R.MAP_CONVT2X2 else n
        lda = lda if lda > ka else ka + pads["lda"]
        ldw = ldw if ldw > k else k + pads["ldw"]
        for buf, key, width in (("res", "ldr", cols), ("out32", "ld32", cols), ("out16", "ld16", cols), ("aux16", "ldaux", n)):
            if buf in e and key not in e:
                e[key] = width + pads[key]
    return L.gemm_plan(c["a"], lda, W, ldw, m, n, k, c["dt"], 0, **e)


def smallest_m(L, c):
    """The fewest rows at which this device plans the same launch (PLAN_KEY), among row counts that keep M % 256 and every period of
    the call (res_mod, vt_T, the row map's image)."""
    e = c["epi"]
    step = 256
    for per in (e.get("res_mod", 0), e.get("vt_T", 0), e["p"][0] if e.get("map") == R.MAP_GROUP else 0,
                e["p"][3] * e["p"][4] if e.get("map") == R.MAP_WINDOW_PART else 0):
        if per:
            step = step * per // math.gcd(step, per)
    want = [getattr(_plan(L, c, c["m"]), f) for f in PLAN_KEY]
    for m in range(c["m"] % step or step, c["m"], step):
        try:
            if [getattr(_plan(L, c, m), f) for f in PLAN_KEY] == want:
                return m
        except RuntimeError:                                   # a row count this call's own constraints exclude: not a candidate
            continue
    return c["m"]


def run_case(L, name, c, want=None):
    """Padded and as-written runs of one call; prints what ran.  An error of la_gemm_plan or la_gemm fails the case."""
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    prev = L.gemm_variant(c["variant"])
    try:
        full = _plan(L, c, c["m"])
        fam_table = L.GEMM_KERNELS[full.kernel]
        if want is not None:
            got = {f: getattr(full, f) for f in PLAN_KEY}
            table = {f: want[f] for f in PLAN_KEY}
            if ncu == 256:                                     # the table's CU count: the device plans the launch the table holds, variant and all
                assert got == table, (name, fam_table)
            elif got != table:
                print(f"[gemm-contract] {name}: {ncu} CUs plan {fam_table} {got}, the table (256 CUs) {L.GEMM_KERNELS[want['kernel']]} {table}")
        m = smallest_m(L, c) if c["m"] * c["n"] * c["k"] > SHRINK_ABOVE else c["m"]
        a, w, epi, lds, off = build(c, "cuda", m)
        fam_row = L.GEMM_KERNELS[_plan(L, c, m).kernel]
        fam_pad = L.GEMM_KERNELS[_plan(L, c, m, R.PADS).kernel]
        for pads, fam in ((R.PADS, fam_pad), (None, fam_row)):
            r = R.check_gemm_call(L, a, w, m, c["n"], c["k"], c["dt"], epi, pads=pads, family=fam, lds=lds, a_elem_off=off, label=name)
            note = "" if fam == fam_row else f" (the pads move it from {fam_row})"
            per = " ".join(f"{k}={v:.3f}" for k, v in r["ratios"].items()) + (f" (rounding share {r['share16']:.2f})" if "out16" in r["ratios"] else "")
            print(f"[gemm-contract] {name} M={m} pads={'default' if pads else 'none'}: {r['family']} epi={r['plan'].epi}{note} "
                  f"err/allowance {r['ratio']:.3f} [{per}]")
            assert r["ratio"] <= 1.0
    finally:
        L.gemm_variant(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_planned_launch_runs_inside_its_guards(L, name):
    c, want = TABLE_ROWS[name]
    if name in NEEDS_12GIB and torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("needs 4 GiB for one strided operand")
    run_case(L, name, c, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [x[0] for x in EXTRA])
def test_family_cells_the_table_does_not_hold(L, name):
    run_case(L, name, EXTRA_ROWS[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [x[1] for x in REFUSED])
def test_la_gemm_refuses_what_its_families_do_not_take(L, name):
    """la_gemm_plan AND la_gemm raise the literal message, padded and compact, on real operands between guards that stay untouched."""
    text, c = REFUSED_ROWS[name]
    prev = L.gemm_variant(c["variant"])
    try:
        a, w, epi, lds, off = build(c, "cuda")
        for pads in (R.PADS, None):
            R.check_gemm_call(L, a, w, c["m"], c["n"], c["k"], c["dt"], epi, pads=pads, lds=lds, a_elem_off=off, label=name, refused=text)
        print(f"[gemm-contract] {name}: la_gemm_plan and la_gemm refuse it ({text[:44]}...)")
    finally:
        L.gemm_variant(prev)
