#!/usr/bin/env python
"""In-kernel clock of the four-wave GEMM's main loop (measurement library): workgroup 0 stamps s_memtime AND s_memrealtime (100 MHz)
at 1 main loop starts | 2 main loop done (la_gemm_variant bit 10); cycles / time over every stamped main loop = the clock the chip holds
there.  After WARM_S seconds of back-to-back launches on random data.  LA_W4_MFMA=16 / 32 picks the MFMA shape (one process each);
SHAPES "name:kind:m:n:k,...", kind in plain / gelu / res."""
import ctypes as C, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._dbglib import use_debug_library
use_debug_library()
import torch  # noqa: E402
from labelanything_amd import _lib as L  # noqa: E402

lib = L.lib()
NST = 128
buf, rbuf = (C.c_ulonglong * (4 * NST))(), (C.c_ulonglong * (4 * NST))()
M = int(os.environ.get("M", 131072))
WARM_S = float(os.environ.get("WARM_S", 2.0))
SHAPES = [("qkv", "plain", M, 2304, 768), ("lin1", "gelu", M, 3072, 768), ("lin2", "res", M, 768, 3072), ("sq8192", "plain", 8192, 8192, 8192)]
if os.environ.get("SHAPES"):
    SHAPES = [(t.split(":")[0], t.split(":")[1], *(int(x) for x in t.split(":")[2:])) for t in os.environ["SHAPES"].split(",")]
dt = torch.float16
for name, kind, m, n, k in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(m, k, device="cuda", generator=g).to(dt)
    w = (torch.randn(n, k, device="cuda", generator=g) / math.sqrt(k)).to(dt)
    bias = torch.randn(n, device="cuda", generator=g)
    o16 = torch.empty(m, n, device="cuda", dtype=dt) if kind != "res" else None
    res = torch.zeros(m, n, device="cuda") if kind == "res" else None

    def run():
        if kind == "gelu":
            L.gemm(a, w, bias=bias, out16=o16, act=L.ACT_GELU)
        elif kind == "res":
            L.gemm(a, w, bias=bias, res=res, out32=res)
        else:
            L.gemm(a, w, bias=bias, out16=o16)

    L.gemm_variant(2)
    mfma = L.gemm_plan(a, k, w, k, m, n, k, L.LA_F16, **(dict(bias=bias, res=res, out32=res) if kind == "res" else dict(bias=bias, out16=o16, act=L.ACT_GELU if kind == "gelu" else L.ACT_NONE))).mfma
    t0 = time.time()
    nrun = 0
    while time.time() - t0 < WARM_S:
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        nrun += 20
    us = (time.time() - t0) / nrun * 1e6
    lib.la_dbg_w4_stamps_clear()
    L.gemm_variant(2 | 0x400)
    run()
    lib.la_dbg_w4_stamps(C.cast(buf, C.c_void_p))
    lib.la_dbg_w4_rstamps(C.cast(rbuf, C.c_void_p))
    L.gemm_variant(2)
    cyc = rt = nloop = 0
    for wave in range(4):
        ev = [(int(buf[wave * NST + i]) & 0xff, int(buf[wave * NST + i]) >> 8, int(rbuf[wave * NST + i])) for i in range(NST) if buf[wave * NST + i]]
        for (t0_, c0, r0), (t1_, c1, r1) in zip(ev, ev[1:]):
            if (t0_, t1_) == (1, 2):
                cyc, rt, nloop = cyc + (c1 - c0), rt + (r1 - r0), nloop + 1
    print(f"{name:8s} {m}x{n}x{k} {kind:5s} mfma {'16x16x32' if mfma else '32x32x16'}: {us:8.1f} us per launch (host, back to back); "
          f"{nloop} main loops of workgroup 0: {cyc / max(nloop, 1):9.0f} cycles, {rt / max(nloop, 1) / 100:7.2f} us each = {cyc / max(rt, 1) * 100:6.0f} MHz in the main loop")
