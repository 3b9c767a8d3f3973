#!/bin/bash
# Run on the MI355X box (via gpurun) from the repo root: refreshes everything the judge reads under profiles/ for round $1.
#   gpurun --timeout 2400 -- 'bash tools/collect_profiles.sh r04'
# (the timeline tools need the measurement library: make -C labelanything_amd/csrc DEBUG=1 before the call - the .so travels with the snapshot)
# Outputs land in gpurun_out/profiles_<round>/ (merged back by gpurun); copy them into profiles/ and commit.
set -u
R=${1:-r04}
export TMPDIR=/tmp
OUT=gpurun_out/profiles_$R
mkdir -p $OUT
# 1. HBM-side traffic of the GEMM kernels FIRST (one counter per pass, no other trace domains): the bench line below attaches the
#    bytes per launch of a traffic file that matches its workload, numerics and batch
timeout 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc -o f -- python bench.py --full --no-cpu-baseline --no-eager-baseline --no-graphs --steps 2 --warmup 1 > /dev/null 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc -o w -- python bench.py --full --no-cpu-baseline --no-eager-baseline --no-graphs --steps 2 --warmup 1 > /dev/null 2>&1
python tools/pmc_traffic.py $(find $OUT/pmc -name 'f_counter_collection.csv' | head -1) $(find $OUT/pmc -name 'w_counter_collection.csv' | head -1) $OUT/${R}_traffic.json > /dev/null 2> $OUT/traffic.stderr
cp $OUT/${R}_traffic.json profiles/${R}_traffic.json 2>/dev/null      # (on the box: bench.py reads profiles/)
# 2. the official bench line (--full: with roofline + cpu_baseline)
timeout 900 python bench.py --full > $OUT/${R}_bench.json 2> $OUT/bench.stderr
# 3. rocprofv3 kernel stats of the same command (eager launches so that every kernel is a separate dispatch record too)
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python bench.py --full --no-cpu-baseline --no-eager-baseline > $OUT/prof_graph.log 2>&1
cp $(find $OUT/prof -name 'bench_kernel_stats.csv' | head -1) $OUT/${R}_bench_kernel_stats.csv 2>/dev/null
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_eager -o bench -- python bench.py --full --no-cpu-baseline --no-eager-baseline --no-graphs > $OUT/prof_eager.log 2>&1
cp $(find $OUT/prof_eager -name 'bench_kernel_stats.csv' | head -1) $OUT/${R}_bench_eager_kernel_stats.csv 2>/dev/null
if [ -n "${ONLY_HEAD:-}" ]; then rm -rf $OUT/prof $OUT/prof_eager $OUT/pmc; ls -la $OUT; exit 0; fi
# 3b. the same two passes on cfg4 (decoder-dominated: the fused two-way kernels' stream traffic)
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc4 -o f -- python bench.py --full --workload cfg4 --no-cpu-baseline --no-graphs --steps 2 --warmup 1 > /dev/null 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc4 -o w -- python bench.py --full --workload cfg4 --no-cpu-baseline --no-graphs --steps 2 --warmup 1 > /dev/null 2>&1
python tools/pmc_traffic.py $(find $OUT/pmc4 -name 'f_counter_collection.csv' | head -1) $(find $OUT/pmc4 -name 'w_counter_collection.csv' | head -1) $OUT/${R}_traffic_cfg4.json cfg4 > /dev/null 2>> $OUT/traffic.stderr
# 3c. the other workloads (each carries its own kernel table; traffic stays null where no PMC file matches) and the two
#     numerics variants of the headline: plain 16-bit operands (round-1 numerics, misses 1e-3) and bf16
for w in cfg1 cfg3 cfg4 cfg5 cfg3_train; do timeout 600 python bench.py --full --workload $w --no-cpu-baseline --no-eager-baseline > $OUT/${R}_bench_$w.json 2>> $OUT/bench.stderr; done
timeout 600 python bench.py --full --workload cfg3_train --train-encoder --no-cpu-baseline > $OUT/${R}_bench_cfg3_train_encoder.json 2>> $OUT/bench.stderr
timeout 600 python bench.py --full --workload cfg2_train --train-encoder --no-cpu-baseline > $OUT/${R}_bench_cfg2_train_encoder.json 2>> $OUT/bench.stderr
timeout 600 python bench.py --full --workload cfg5 --attn-fp8 --no-cpu-baseline > $OUT/${R}_bench_cfg5_fp8.json 2>> $OUT/bench.stderr
# On an 8-GPU node (the driver's SCALE run; nothing here can launch it): one rank per GPU over RCCL, bucketed gradient all-reduce
#   python bench.py --gpus 8 --workload cfg3_train --train-encoder        (bench.py starts its own ranks when WORLD_SIZE is unset)
#   python bench.py --gpus 8
timeout 600 python bench.py --full --no-cpu-baseline --no-eager-baseline --precise patch,v,proj,neck > $OUT/${R}_bench_cfg2_weight_planes.json 2>> $OUT/bench.stderr
# round 6: the LayerNorm kernels instead of the folded form (same box A/B of the headline and of cfg1), the folded GEMM forms against the plain epilogues
timeout 600 python bench.py --full --no-cpu-baseline --no-eager-baseline --no-norm-fold > $OUT/${R}_bench_cfg2_no_norm_fold.json 2>> $OUT/bench.stderr
timeout 600 python bench.py --full --workload cfg1 --no-cpu-baseline --no-eager-baseline --no-norm-fold > $OUT/${R}_bench_cfg1_no_norm_fold.json 2>> $OUT/bench.stderr
timeout 600 python bench.py --full --no-cpu-baseline --no-eager-baseline --no-conv-implicit > $OUT/${R}_bench_cfg2_no_conv_implicit.json 2>> $OUT/bench.stderr
timeout 300 python tools/normfold_ab.py > $OUT/${R}_normfold_ab.log 2>&1
timeout 600 python tools/attn_fp8_report.py > $OUT/${R}_attn_fp8.log 2>&1
timeout 600 python tools/gemm_ab.py > $OUT/${R}_gemm_ab.log 2>&1
if [ -f labelanything_amd/libla_hip_dbg.so ]; then
  timeout 300 python tools/gemm_seam.py > $OUT/${R}_gemm_seam_timeline.log 2>&1
  timeout 300 python tools/twoway_phases.py > $OUT/${R}_twoway_phases.log 2>&1
  # the four-wave GEMM: seam timeline (cycles at the real clock against wall time), ablations of the k-tile body, SQ counters on 8192^3
  timeout 300 python tools/w4_seam.py > $OUT/${R}_w4_seam_timeline.log 2>&1
  timeout 300 python tools/w4_ablate.py > $OUT/${R}_w4_ablation.log 2>&1
  timeout 600 bash tools/w4_pmc.sh cube "2" > /dev/null 2>&1; cp gpurun_out/w4_pmc_cube.txt $OUT/${R}_w4_pmc_cube.txt 2>/dev/null
fi
VARIANTS=1,2 BLAS=1 timeout 400 python tools/gemm_ab.py > $OUT/${R}_gemm_ab_w4.log 2>&1
timeout 300 python tools/qkv_split_probe.py > $OUT/${R}_qkv_split_probe.log 2>&1
timeout 200 python tools/bw_probe.py > $OUT/${R}_bw_probe.log 2>&1
timeout 200 python tools/win96_probe.py > $OUT/${R}_window_attention_96_images.log 2>&1
[ -f labelanything_amd/libla_hip_dbg.so ] && timeout 200 python tools/win_phases.py > $OUT/${R}_window_phases.log 2>&1
IT=3 timeout 900 bash tools/kernel_pmc.sh attn attn_fwd python tools/attn_ab.py > /dev/null 2>&1; cp gpurun_out/pmc_attn.txt $OUT/${R}_attn_pmc.txt 2>/dev/null
timeout 300 python tools/twoway_d512_ab.py > $OUT/${R}_twoway_d512_ab.log 2>&1
timeout 900 python -m pytest tests/test_parity_seeds_gpu.py tests/test_encoder_train_gpu.py tests/test_sam_train_gpu.py tests/test_train_gpu.py::test_cfg3_train_step_at_full_size -m gpu -q -s > $OUT/${R}_parity_seeds.log 2>&1
timeout 600 python bench.py --full --no-cpu-baseline --no-eager-baseline --precise none > $OUT/${R}_bench_cfg2_plain16.json 2>> $OUT/bench.stderr
timeout 600 python bench.py --full --no-cpu-baseline --no-eager-baseline --dtype bf16 > $OUT/${R}_bench_cfg2_bf16.json 2>> $OUT/bench.stderr
timeout 300 python tools/blas_calibration.py > $OUT/${R}_blas_calibration.log 2>&1
# per-shape GEMM / attention time inside the model, the attention forms alone, the MFMA / VALU co-issue probe, the gradient diagnostic
timeout 600 python bench.py --full --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg2.log > /dev/null
timeout 600 python bench.py --full --workload cfg1 --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg1.log > /dev/null
timeout 300 python tools/attn_ab.py > $OUT/${R}_attn_shapes.log 2>&1
# training-side kernels by shape: flash-attention backward next to its forward, the fp32 weight-gradient GEMM, the rel-pos backward
timeout 300 python tools/attn_bwd_bench.py > $OUT/${R}_attn_bwd_shapes.log 2>&1
timeout 300 python tools/gemm_tn_bench.py > $OUT/${R}_gemm_tn_shapes.log 2>&1
timeout 300 python tools/wgrad_ab.py > $OUT/${R}_wgrad_ab_final.log 2>&1      # la_gemm_tn16 against transposes + split-K la_gemm
timeout 300 python tools/relpos_bwd_bench.py > $OUT/${R}_relpos_bwd_bench.log 2>&1
timeout 600 python bench.py --full --workload cfg3_train --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg3_train.log > /dev/null
timeout 600 python bench.py --full --workload cfg3_train --train-encoder --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg3_train_encoder.log > /dev/null
timeout 600 python bench.py --full --workload cfg2_train --train-encoder --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg2_train_encoder.log > /dev/null
timeout 600 python bench.py --full --workload cfg4 --gemm-shapes --no-cpu-baseline --no-eager-baseline 2> $OUT/${R}_gemm_shapes_cfg4.log > /dev/null
[ -x tools/probes/coissue ] && timeout 120 ./tools/probes/coissue > $OUT/${R}_coissue_probe.log 2>&1
timeout 600 python tools/train_grad_diag.py > $OUT/${R}_train_grad_diag.log 2>&1
timeout 900 python tools/race_screen.py 40 > $OUT/${R}_race_screen.log 2>&1
# 4. parity report + per-op micro benchmarks
timeout 900 python tools/parity_report.py > $OUT/${R}_parity.log 2>&1
timeout 900 python tools/parity_report.py --groups > $OUT/${R}_parity_groups.log 2>&1
timeout 600 python tools/bench_ops.py > $OUT/${R}_bench_ops.log 2>&1
rm -rf $OUT/prof $OUT/prof_eager $OUT/pmc $OUT/pmc4
ls -la $OUT
