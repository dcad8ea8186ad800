#!/bin/bash
# Round-4 profile set (results under gpurun_out/prof_r04/; the summaries are copied into profiles/r04_* by hand):
#   bash tools/profile_r04.sh [stats] [pmc] [traffic] [em]        (default: all)
# Both arithmetics: the default leg (shipped plans, f16x3) and the exact-split leg (bench.py --math-modes 0 1: fp32 MFMA / bf16x6).
# Under rocprofv3 the program itself follows `--` (no shell / env wrapper).  Counters in their own passes, --kernel-trace only.
export TMPDIR=/tmp
OUT=gpurun_out/prof_r04; mkdir -p $OUT
WHAT="${*:-stats pmc traffic em}"
COMMON="--full --no-cpu-baseline --no-em --no-legs"
for leg in default exact; do
  MM=""; TAG=""
  if [ $leg = exact ]; then MM="--math-modes 0 1"; TAG="_exact"; fi
  if [[ $WHAT == *stats* ]]; then
    # eager one-sequence frames, every kernel a record, joined with the per-launch layer list -> conv_by_layer
    rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/eager$TAG -- python3 bench.py --steps 8 --warmup 2 $COMMON --no-graph --seqs 1 $MM --trace-layers $OUT/layers.json > $OUT/bench_eager$TAG.json 2> $OUT/eager$TAG.err
    cp $(ls $OUT/eager$TAG/*/*kernel_stats.csv | head -1) $OUT/bench_seq1_eager_kernel_stats$TAG.csv
    python3 tools/conv_by_layer.py $OUT/layers.json$TAG $(ls $OUT/eager$TAG/*/*kernel_trace.csv | head -1) $OUT/conv_by_layer$TAG.csv > $OUT/conv_by_layer$TAG.txt 2>&1
    cp $OUT/layers.json$TAG $OUT/conv_layers_traced$TAG.json
    # the bench's own configuration (four sequences, graph replay)
    rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/graph$TAG -- python3 bench.py --steps 20 --warmup 5 $COMMON --no-roofline $MM > $OUT/bench_profiled$TAG.json 2> $OUT/graph$TAG.err
    cp $(ls $OUT/graph$TAG/*/*kernel_stats.csv | head -1) $OUT/bench_default_kernel_stats$TAG.csv
    rm -rf $OUT/eager$TAG $OUT/graph$TAG
  fi
  if [[ $WHAT == *traffic* ]]; then
    for c in FETCH_SIZE WRITE_SIZE; do
      rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/traffic$TAG/$c -- python3 bench.py --steps 6 --warmup 2 $COMMON --no-graph --no-roofline --seqs 1 $MM > $OUT/traffic$TAG.$c.log 2>&1
    done
    python3 tools/pmc_by_kernel.py $OUT/traffic$TAG $OUT/conv_traffic_by_kernel$TAG.json > $OUT/conv_traffic_by_kernel$TAG.txt
    rm -rf $OUT/traffic$TAG
  fi
done
if [[ $WHAT == *pmc* ]]; then
  # the dominant kernel of each leg on its largest layer (2x120x216 k3 256->256), the plans the shipped file holds for it
  bash tools/pmc_kernels.sh $OUT/conv_pmc.txt conv_igemm python3 tools/conv_bench.py --reps 8 --only 0 --plan 0x670122 > /dev/null
  bash tools/pmc_kernels.sh $OUT/conv_pmc_exact.txt conv_igemm python3 tools/conv_bench.py --reps 8 --only 0 --plan 0x8810122 > /dev/null
fi
if [[ $WHAT == *em* ]]; then
  bash tools/pmc_kernels.sh $OUT/em_pmc.txt 'em_|match_|conv_igemm' python3 tools/em_loop.py --reps 10 > /dev/null
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/emloop -- python3 tools/em_loop.py --reps 50 > $OUT/emloop.log 2>&1
  cp $(ls $OUT/emloop/*/*kernel_stats.csv | head -1) $OUT/em_loop_kernel_stats.csv; rm -rf $OUT/emloop
fi
rm -rf gpurun_out/pmc_conv_pmc gpurun_out/pmc_conv_pmc_exact gpurun_out/pmc_em_pmc
ls -la $OUT | head -40
