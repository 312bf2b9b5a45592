#!/bin/bash
# Round-5 evidence in one GPU-box visit (run via gpurun from the repo root): the -m gpu suite, the smoke run, the per-launch profile of the timed step (kernel trace +
# FETCH_SIZE + WRITE_SIZE passes: scripts/dominant_launches.sh) — copied into profiles/ BEFORE the bench so that the bench line's roofline.traffic comes from the
# launches of this very tree —, the bench line, rocprofv3 kernel stats of the bench command, the kernel-only stress set, single long sweeps alone on the device.
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/r5z
mkdir -p $OUT
cd $R
timeout 1200 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.txt 2>&1; tail -4 $OUT/pytest_gpu.txt
timeout 300 python __graft_entry__.py smoke 2>&1 | tail -2 | tee $OUT/smoke.txt
bash scripts/dominant_launches.sh > $OUT/dominant.txt 2>&1; tail -22 $OUT/dominant.txt | cut -c1-200
cp gpurun_out/dom/dominant_launches.json profiles/dominant_launches_latest.json 2>/dev/null
cp gpurun_out/dom/dominant_launches.json $OUT/dominant_launches.json 2>/dev/null
cp gpurun_out/dom/trace/*kernel_stats.csv $OUT/step_kernel_stats.csv 2>/dev/null
rm -rf gpurun_out/dom/pmc_FETCH_SIZE gpurun_out/dom/pmc_WRITE_SIZE gpurun_out/dom/trace
timeout 900 python bench.py --full 2>$OUT/bench.err | tee $OUT/bench.json | cut -c1-600
export TMPDIR=/tmp
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r05 -- python3 $R/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras > $OUT/bench_prof.json 2>$OUT/prof.err
cd $R
cp $OUT/prof/*kernel_stats.csv $OUT/c3_msa_kernel_stats.csv 2>/dev/null; rm -rf $OUT/prof
timeout 300 python scripts/stress_set.py --json $OUT/stress_set.json > $OUT/stress.txt 2>&1; cat $OUT/stress.txt | cut -c1-200
timeout 300 python scripts/dev/lane_probe.py > $OUT/lane_probe.txt 2>&1; cat $OUT/lane_probe.txt | cut -c1-220
du -sh $OUT
