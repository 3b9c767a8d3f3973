#!/usr/bin/env python
"""Instructions of one tile's epilogue per wave, for every gemm_t256w_kernel instance of a device assembly listing:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S labelanything_amd/csrc/gemm_w4.hip -o w4.s
    python tools/w4_epilogue_isa_count.py w4.s

Counted from the seam's ``s_nop 15`` to the first MFMA behind it (the accumulator clear of the next tile).  A compile, not a run.
Instance tags are the mangled template arguments: DF16_ = fp16, Li<EPI>E, Li0E = no ablation, Lb<DIRECT>E, Lb<RAGGED>E, Li<MS>E (1 = the
16x16x32 main loop).  The last column group also shows scratch instructions: every instance but the mapped EPI 3 one has none."""
import collections, re, sys

txt = open(sys.argv[1]).read()
for m in re.finditer(r'^(_ZN2la17gemm_t256w_kernelI(\S+?)EEv\S*):[^\n]*\n(.*?)\n\s*s_endpgm', txt, re.S | re.M):
    tag, body = m.group(2), m.group(3)
    i = body.find('s_nop 15')
    if 'DF16_' not in tag or i < 0:
        continue
    ops = collections.Counter()
    for line in body[i:].split('\n')[1:]:
        line = line.strip()
        if not line or line.startswith((';', '.', '//')) or line.endswith(':'):
            continue
        op = line.split()[0]
        if op.startswith('v_mfma'):
            break
        ops[op] += 1
    c = lambda *p: sum(v for k, v in ops.items() if k.startswith(p))
    print(f"{tag:24s} total {sum(ops.values()):5d}  v_mov {c('v_mov_b32'):4d} saveexec {c('s_and_saveexec'):3d} mad64 {c('v_mad_i64', 'v_mad_u64'):3d} "
          f"lshl_add_u64 {c('v_lshl_add_u64'):3d} v_add {c('v_add_u32', 'v_add_co', 'v_addc'):4d} salu {c('s_'):4d} s_nop {c('s_nop'):4d} "
          f"scratch {c('scratch_'):3d} gload {c('global_load'):3d} gstore {c('global_store'):3d}")
