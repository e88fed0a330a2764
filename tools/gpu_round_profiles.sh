#!/bin/bash
# round 2: full GPU suite + the measurements that go to profiles/
set -o pipefail
O=$(realpath -m "${1:?usage: tools/gpu_round_profiles.sh OUTPUT_DIR}"); cd "$(dirname "$0")/.."; mkdir -p "$O"; export TMPDIR=/tmp
python -m pytest tests -m gpu -x -q > $O/tests_gpu_final.log 2>&1; echo "pytest rc=$?"; tail -4 $O/tests_gpu_final.log
python bench.py --full > $O/bench_final.json 2> $O/bench_final.err; echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_bench -o b -- python3 bench.py --steps 3 --full --no_cpu_baseline > $O/bench_under_rocprof.json 2> $O/bench_under_rocprof.err; echo "rocprof bench rc=$?"
cp $(find $O/prof_bench -name "*kernel_stats.csv" | head -1) $O/r02_bench_kernel_stats.csv
python tools/trace_by_grid.py $O/prof_bench $O/r02_bench_by_grid.json; rm -rf $O/prof_bench
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_fwd -o f -- python3 tools/bench_forward.py > $O/forward_under_rocprof.json 2> $O/forward_under_rocprof.err; echo "rocprof fwd rc=$?"
cp $(find $O/prof_fwd -name "*kernel_stats.csv" | head -1) $O/r02_forward_kernel_stats.csv
python tools/trace_by_grid.py $O/prof_fwd $O/r02_forward_by_grid.json; rm -rf $O/prof_fwd
python tools/bench_forward.py 2>/dev/null | tail -1 > $O/forward_unprofiled.json
python tools/bench_modules.py 2>/dev/null | tail -1 > $O/r02_modules_bench.json
python tools/bench_v2.py 2>/dev/null | tail -1 > $O/r02_v2_bench.json
python tools/bench_rpr_prefill.py 2>/dev/null | tail -1 > $O/r02_rpr_prefill.json
NB=32 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_v2 -o v -- python3 tools/prof_v2_batch.py > $O/prof_v2.log 2>&1
python tools/trace_by_grid.py $O/prof_v2 $O/r02_v2_lockstep_B32_by_grid.json; cp $(find $O/prof_v2 -name "*kernel_stats.csv" | head -1) $O/r02_v2_lockstep_B32_kernel_stats.csv; rm -rf $O/prof_v2
python tools/bench_v2_phases.py 2>/dev/null | tail -1 > $O/r02_v2_phases.json
NB=32 rocprofv3 --kernel-trace --output-format csv -d $O/prof_v2t -o v -- python3 tools/prof_v2_batch.py > $O/prof_v2t.log 2>&1
python tools/trace_v2_steps.py $O/prof_v2t $O/r02_v2_step_timeline.json > $O/r02_v2_step_timeline.txt; rm -rf $O/prof_v2t
python tools/bench_families.py 2>/dev/null | tail -1 > $O/r02_families_bench.json
cat $O/forward_unprofiled.json $O/r02_rpr_prefill.json
head -c 2500 $O/bench_final.json
