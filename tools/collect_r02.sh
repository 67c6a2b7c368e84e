#!/bin/bash
# Round-2 evidence, run on the GPU box through gpurun from the repo root:
#   kernel-trace stats of every bench workload, PMC passes (HBM traffic, LDS / issue counters; each in its own run,
#   never combined with other trace domains), and the un-profiled bench lines.  Results: gpurun_out/r02/.
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out/r02
mkdir -p $OUT
for WL in default m3a m1 m2b m4; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_$WL -- python3 bench.py --workload $WL --steps 20 --warmup 3 --repeats 0 --full --no-cpu-baseline > $OUT/under_rocprof_$WL.log 2>&1
  cp $OUT/trace_$WL/*/*kernel_stats.csv $OUT/kernel_stats_$WL.csv 2>/dev/null
  rm -rf $OUT/trace_$WL
  echo "== $WL"; python3 tools/kstats.py $OUT 0 >/dev/null 2>&1; head -8 $OUT/kernel_stats_$WL.csv | cut -c1-160
done
pmc() { # workload tag counters
  rocprofv3 --pmc $3 --kernel-trace --output-format csv -d $OUT/pmc_$1_$2 -- python3 bench.py --workload $1 --steps 3 --warmup 1 --repeats 0 --no-cpu-baseline > $OUT/pmc_$1_$2.log 2>&1
}
for WL in m1 m2b; do
  pmc $WL fetch "FETCH_SIZE"
  pmc $WL write "WRITE_SIZE"
  pmc $WL sq "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY"
  python3 tools/pmc_summary.py $OUT "" > $OUT/pmc_summary_$WL.txt
  rm -rf $OUT/pmc_${WL}_fetch $OUT/pmc_${WL}_write $OUT/pmc_${WL}_sq
done
python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
for WL in m2b m4 m3b; do python3 bench.py --workload $WL --full > $OUT/bench_$WL.json 2> $OUT/bench_$WL.err; done
MXX_BENCH_FORCE_DIST=1 python3 bench.py --steps 10 --repeats 1 --full --no-cpu-baseline > $OUT/bench_world1_rccl.json 2> $OUT/bench_world1_rccl.err
tail -c 300 $OUT/bench_default.json
