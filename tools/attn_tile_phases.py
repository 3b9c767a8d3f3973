#!/usr/bin/env python
"""Per-tile timeline of attn_fwd_kernel's key loop for the two instances the benchmark runs (global rel-pos rows, G = 64, T = 4096:
tiles 28 - 35 of 64; 14 x 14 windows in image order: tiles 0 - 3), from the s_memtime stamps of the -DLA_DEBUG library (TILE_STAMP in
csrc/attn_enc.hip): the workgroup in the middle of the launch, every wave.  LA_TOOLS_LIB=<a -DLA_DEBUG build> picks the build.

A stamp marks where the wave's ISSUE stands, not where results are complete: an in-order wave stalls at the first instruction that
needs a pending result, so the tail of an MFMA cluster is counted in the phase behind it."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._dbglib import use_debug_library, use_env_library  # noqa: E402

if os.environ.get("LA_TOOLS_LIB"):
    use_env_library()
else:
    use_debug_library()
import torch  # noqa: E402
from labelanything_amd import _lib as L  # noqa: E402

lib = L.lib()
POINTS = ("top", "pieces issued", "S issued", "softmax done", "PV issued", "after wait", "after barrier")
buf = (C.c_uint * 512)()
g = torch.Generator(device="cuda").manual_seed(3)
heads, e, sc = 12, 768, 0.125


def report(name, inst, tile0, us):
    lib.la_dbg_tile_stamps(C.cast(buf, C.c_void_p))
    print(f"{name}: {us:.1f} us per launch; cycles from the tile's top to each stamp (issue order: pieces issued may come after S issued)")
    for w in range(4):
        st = [[int(buf[(inst * 4 + w) * 64 + tl * 8 + p]) for p in range(7)] for tl in range(8)]
        for tl, s in enumerate(st):
            if s[0] == 0 and s[6] == 0:
                continue
            d = [(x - s[0]) & 0xffffffff for x in s]
            nxt = st[tl + 1][0] if tl + 1 < 8 and st[tl + 1][0] else None
            print(f"   wave {w} tile {tile0 + tl:2d}: " + " | ".join(f"{n} {v}" for n, v in zip(POINTS[1:], d[1:]))
                  + f" || softmax {d[3] - max(d[2], 0)} PV {d[4] - d[3]} wait {d[5] - d[4]} barrier {d[6] - d[5]}"
                  + (f" next top +{(nxt - s[6]) & 0xffffffff}" if nxt else ""))


def timed(run):
    for _ in range(3):
        run()
    s, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        run()
    e_.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e_) / 10 * 1e3


# global rel-pos, 16 images
b, t, gg = 16, 4096, 64
qkv = (torch.randn(b * t, 3 * e, device="cuda", generator=g) * 0.8).half()
tabh = (torch.randn(2 * gg - 1, 64, device="cuda", generator=g) * 0.3).half()
tabw = (torch.randn(2 * gg - 1, 64, device="cuda", generator=g) * 0.3).half()
out = torch.empty(b * t, e, dtype=torch.float16, device="cuda")
us = timed(lambda: L.attn_fwd_rows(qkv, out, b, heads, t, t, gg, e, sc, L.ATTN_RELPOS, tabh=tabh, tabw=tabw))
report("global rel-pos 16x12 T4096 (ATTN_TABLES_ROW64)", 0, 28, us)

# 14 x 14 windows in image order, 96 images of 64 x 64 tokens
nimg, ih, gg = 96, 64, 14
nw = -(-ih // gg)
b, t, tpad = nimg * nw * nw, gg * gg, (16 * gg + 63) // 64 * 64
qkv = (torch.randn(nimg * ih * ih, 3 * e, device="cuda", generator=g) * 0.8).half()
padrow = (torch.randn(3 * e, device="cuda", generator=g) * 0.5).half()
tabh = (torch.randn(2 * gg - 1, 64, device="cuda", generator=g) * 0.3).half()
tabw = (torch.randn(2 * gg - 1, 64, device="cuda", generator=g) * 0.3).half()
out = torch.empty(nimg * ih * ih, e, dtype=torch.float16, device="cuda")
us = timed(lambda: L.attn_fwd_rows(qkv, out, b, heads, t, tpad, gg, e, sc, L.ATTN_RELPOS_WIN16, tabh=tabh, tabw=tabw, img_hw=(ih, ih), padrow=padrow))
report("windows 14x14 image order, 96 images (ATTN_TABLES_WIN16)", 1, 0, us)
