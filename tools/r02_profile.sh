#!/bin/bash
# Round-2 evidence in ONE gpurun call (program directly after `--`; --pmc passes separate from --kernel-trace):
#   1. overlapped (default two-stream schedule) kernel trace + stats     -> gpurun_out/r02_<tag>_train_T8_kernel_stats.csv / _trace_summary.txt
#   2. SERIAL kernel trace + stats (MTE_NO_SIDE_STREAM=1 in the environment) -> ..._serial_kernel_stats.csv  (bench.py's roofline.frac is the serial figure)
#   3. per-shape conv table (bench.py --dump-conv)                       -> ..._conv_table.txt
#   4. FETCH_SIZE / WRITE_SIZE PMC passes                                -> ..._pmc_traffic_T8.txt
#   5. the bench line itself                                             -> ..._bench.json
tag=${1:-v1}
out=$GRAFT_REPO_ROOT/gpurun_out
mkdir -p $out; rm -rf /tmp/trO /tmp/trS /tmp/pmcF /tmp/pmcW
cd /tmp && export TMPDIR=/tmp
B="$GRAFT_REPO_ROOT/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-kernel-timing"
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/trO -- python3 $B > $out/r02_${tag}_trace_run.txt 2>&1
export MTE_NO_SIDE_STREAM=1
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/trS -- python3 $B > $out/r02_${tag}_trace_serial_run.txt 2>&1
unset MTE_NO_SIDE_STREAM
rocprofv3 --pmc FETCH_SIZE --output-format csv -d /tmp/pmcF -- python3 $GRAFT_REPO_ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-kernel-timing > $out/r02_${tag}_pmcF_run.txt 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d /tmp/pmcW -- python3 $GRAFT_REPO_ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-kernel-timing > $out/r02_${tag}_pmcW_run.txt 2>&1
cd $GRAFT_REPO_ROOT
cp "$(find /tmp/trO -name '*kernel_stats.csv' | head -1)" $out/r02_${tag}_train_T8_kernel_stats.csv
cp "$(find /tmp/trS -name '*kernel_stats.csv' | head -1)" $out/r02_${tag}_train_T8_serial_kernel_stats.csv
python tools/trace_summary.py "$(find /tmp/trO -name '*kernel_trace.csv' | head -1)" 4 90 > $out/r02_${tag}_train_T8_trace_summary.txt
python tools/trace_summary.py "$(find /tmp/trS -name '*kernel_trace.csv' | head -1)" 4 60 > $out/r02_${tag}_train_T8_serial_trace_summary.txt
python3 tools/pmc_traffic.py /tmp/pmcF /tmp/pmcW 3 > $out/r02_${tag}_pmc_traffic_T8.txt
python bench.py --steps 20 --warmup 5 --full --dump-conv $out/r02_${tag}_conv_table.txt > $out/r02_${tag}_train_T8_bench.json 2> $out/r02_${tag}_bench.err
head -3 $out/r02_${tag}_train_T8_serial_trace_summary.txt; tail -c 600 $out/r02_${tag}_train_T8_bench.json
