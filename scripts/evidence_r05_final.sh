#!/bin/bash
# Round-5 closing evidence on the final build: full GPU suite (-x, as the driver runs it), smoke, bench line, rocprofv3 kernel
# stats of the bench command.  Summaries land in gpurun_out/; the ones to be judged are copied to profiles/.
set -u
cd $GRAFT_REPO_ROOT
OUT=$GRAFT_REPO_ROOT/gpurun_out
timeout 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -6 > $OUT/r05_gpu_tests_final.log; tail -2 $OUT/r05_gpu_tests_final.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2 | tee -a $OUT/r05_gpu_tests_final.log
timeout 600 python bench.py --full > $OUT/r05_bench_n1.json 2> $OUT/r05_bench_n1.err || tail -5 $OUT/r05_bench_n1.err
python - <<PY
import json
d = json.load(open("$OUT/r05_bench_n1.json"))
print({k: d[k] for k in ("value", "ms_per_step")}, {k: d["roofline"][k] for k in ("frac", "mfma_frac", "kernel", "kernel_ms", "traffic")})
print(d["cpu_baseline"]["value"], d["extra"]["strong_scaling_proxy_1gpu"])
print(d["extra"]["backprop_mode_adjoint_false"])
PY
bash scripts/collect_profiles.sh r05 "stats" 2>&1 | tail -2
