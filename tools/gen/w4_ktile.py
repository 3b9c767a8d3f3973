#!/usr/bin/env python
"""Generates labelanything_amd/csrc/gemm_w4_ktile.inc: the k-tile body of gemm_t256w (64 MFMAs 32x32x16 - or, LA_W4_BLOCK16_*, 128 MFMAs 16x16x32 -, 32 fragment reads,
16 LDS-DMA pieces, 2 waits + barriers) as macro sequences, one per filler GROUPING (LA_W4_GROUP): the memory instructions of an 8-MFMA block are placed
G at a time behind MFMA 1, 1 + stride, ... instead of one behind every MFMA.  Same instructions, same operands, same order of the MFMAs
(results are bit-identical); what changes is how many MFMA -> MFMA gaps carry fillers.  python tools/gen/w4_ktile.py > .../gemm_w4_ktile.inc"""

def MF(ib, ii, j, par, ks): return f"LA_W4_MF({ib}, {ii}, {j}, {par}, {ks})"
def blocks():
    b = []
    # (mfma args, mem ops, tail) per block; mfma order: ii = 0: j 0..3, ii = 1: j 0..3
    def mf(ib, par, ks): return [MF(ib, ii, j, par, ks) for ii in (0, 1) for j in range(4)]
    def rw(ks): return [f"LA_W4_RW({ks}, {j})" for j in range(4)]
    def ra(par, ii, i, ks): return f"LA_W4_RA({par}, {ii}, {i}, {ks})"
    # H1: reads of the next ks in order of first use: A_i0, W_0..3, A_i1
    b.append((mf(0, 0, 0), [ra(1, 0, 0, 1)] + rw(1) + [ra(1, 1, 1, 1), "LA_W4_PA1(sa1, 0, bo1)", "LA_W4_PA1(sa1, 1, bo1)"], None))
    b.append((mf(0, 1, 1), [ra(0, 0, 0, 2)] + rw(2) + [ra(0, 1, 1, 2), "LA_W4_PA1(sa1, 2, bo1)"], None))
    b.append((mf(0, 0, 2), [ra(1, 0, 0, 3)] + rw(3) + [ra(1, 1, 1, 3), "LA_W4_PA1(sa1, 3, bo1)"], "LA_W4_WAIT(16)"))
    b.append((mf(0, 1, 3), [ra(0, 0, 2, 0), ra(0, 1, 3, 0), "LA_W4_PA0(saw, 0, bofs)", "LA_W4_PA0(saw, 1, bofs)"], None))
    b.append((mf(2, 0, 0), [ra(1, 0, 2, 1), ra(1, 1, 3, 1), "LA_W4_PA0(saw, 2, bofs)", "LA_W4_PA0(saw, 3, bofs)", "LA_W4_PW(sww, 0, bofs)"], None))
    b.append((mf(2, 1, 1), [ra(0, 0, 2, 2), ra(0, 1, 3, 2), "LA_W4_PW(sww, 1, bofs)", "LA_W4_PW(sww, 2, bofs)", "LA_W4_PW(sww, 3, bofs)"], None))
    b.append((mf(2, 0, 2), [ra(1, 0, 2, 3), ra(1, 1, 3, 3), "LA_W4_PW(sww, 4, bofs)", "LA_W4_PW(sww, 5, bofs)", "LA_W4_PW(sww, 6, bofs)"], "LA_W4_WAIT(15)"))
    b.append((mf(2, 1, 3), [ra(0, 0, 0, 0)] + rw(0) + [ra(0, 1, 1, 0), "LA_W4_PW(sww, 7, bofs)"], None))
    return b

# The same k-tile on v_mfma_f32_16x16x32 (LA_W4_BLOCK16_<b>): a wave's 128 x 128 block is 8 x 8 blocks of 16 x 16, a k-tile two k-steps of
# 32; block b = 16 MFMAs of two 16-row A fragments against the eight W fragments of one k-step.  H1 (blocks 0-3) walks row blocks 0-3
# (the A0 rows), H2 (blocks 4-7) row blocks 4-7 (A1), each in the order (ks 0: rows lo, hi), (ks 1: rows lo, hi) - k ascends per
# accumulator - so the reads of W and A0 end with block 2 and the DMA pieces, waits and barriers sit exactly where the 32x32x16 body has them.
def MF16(bi, bj, par, ii, ks): return f"LA_W4_MF16({bi}, {bj}, {par}, {ii}, {ks})"
def blocks16():
    b = []
    def mf(bi0, par, ks): return [MF16(bi0 + ii, bj, par, ii, ks) for ii in (0, 1) for bj in range(8)]
    def rw(ks, js): return [f"LA_W4_RW16({ks}, {j})" for j in js]
    def ra(par, ii, bi, ks): return f"LA_W4_RA16({par}, {ii}, {bi}, {ks})"
    # reads of the next block's fragments in the order of their first use
    b.append((mf(0, 0, 0), [ra(1, 0, 2, 0), ra(1, 1, 3, 0)] + rw(1, range(0, 4)) + ["LA_W4_PA1(sa1, 0, bo1)", "LA_W4_PA1(sa1, 1, bo1)"], None))
    b.append((mf(2, 1, 0), [ra(0, 0, 0, 1)] + rw(1, range(4, 8)) + [ra(0, 1, 1, 1), "LA_W4_PA1(sa1, 2, bo1)"], None))
    b.append((mf(0, 0, 1), [ra(1, 0, 2, 1), ra(1, 1, 3, 1), "LA_W4_PA1(sa1, 3, bo1)"], "LA_W4_WAIT(16)"))
    b.append((mf(2, 1, 1), [ra(0, 0, 4, 0), ra(0, 1, 5, 0), "LA_W4_PA0(saw, 0, bofs)", "LA_W4_PA0(saw, 1, bofs)"], None))
    b.append((mf(4, 0, 0), [ra(1, 0, 6, 0), ra(1, 1, 7, 0), "LA_W4_PA0(saw, 2, bofs)", "LA_W4_PA0(saw, 3, bofs)", "LA_W4_PW(sww, 0, bofs)"], None))
    b.append((mf(6, 1, 0), [ra(0, 0, 4, 1), ra(0, 1, 5, 1), "LA_W4_PW(sww, 1, bofs)", "LA_W4_PW(sww, 2, bofs)", "LA_W4_PW(sww, 3, bofs)"], None))
    b.append((mf(4, 0, 1), [ra(1, 0, 6, 1), ra(1, 1, 7, 1), "LA_W4_PW(sww, 4, bofs)", "LA_W4_PW(sww, 5, bofs)", "LA_W4_PW(sww, 6, bofs)"], "LA_W4_WAIT(15)"))
    b.append((mf(6, 1, 1), [ra(0, 0, 0, 0)] + rw(0, range(8)) + [ra(0, 1, 1, 0), "LA_W4_PW(sww, 7, bofs)"], None))
    return b

def emit_block(mfs, mems, wait, g):
    # groups of g memory instructions behind MFMA 1, then evenly spaced; everything issued by the last MFMA but one (the wait sits in
    # front of the last)
    nm = len(mfs)
    groups = [mems[i:i + g] for i in range(0, len(mems), g)]
    n = len(groups)
    if g == 1:
        pos = list(range(1, n + 1))
    else:
        span = nm - 2      # positions 1 .. nm - 1
        pos = [1 + (span * k) // max(n - 1, 1) if n > 1 else 1 for k in range(n)]
    out = []
    for m in range(1, nm + 1):
        if m == nm and wait:
            out.append(wait)
            out.append("LA_W4_SB")
        out.append(mfs[m - 1])
        for k, p in enumerate(pos):
            if p == m:
                out.extend(groups[k])
    if wait:
        out += ["LA_W4_BAR", "LA_W4_SB"]
    return " ".join(out)

print("// GENERATED by tools/gen/w4_ktile.py - do not edit.  LA_W4_BLOCK_<b>: block b of the k-tile (see gemm_w4.hip) for the filler grouping LA_W4_GROUP")
first = True
blocks_16 = []
for g in (1, 2, 3, 4, 8):
    print(("#if" if first else "#elif") + f" LA_W4_GROUP == {g}")
    first = False
    for i, (mfs, mems, wait) in enumerate(blocks()):
        print(f"#define LA_W4_BLOCK_{i} {emit_block(mfs, mems, wait, g)}")
    blocks_16.append([f"#define LA_W4_BLOCK16_{i} {emit_block(mfs, mems, wait, g)}" for i, (mfs, mems, wait) in enumerate(blocks16())])
print("#else\n#error \"LA_W4_GROUP must be 1, 2, 3, 4 or 8\"\n#endif")
print("// LA_W4_BLOCK16_<b>: the k-tile on v_mfma_f32_16x16x32 (16 MFMAs per block)")
for k, g in enumerate((1, 2, 3, 4, 8)):
    print(("#if" if k == 0 else "#elif") + f" LA_W4_GROUP == {g}")
    print("\n".join(blocks_16[k]))
print("#endif")
