#!/bin/bash
# End-of-round evidence on one MI355X: the default bench line, steady-state kernel traces of every bench workload and
# the kNN call -> gpurun_out/final_*  (copy into profiles/ afterwards).   tools/final_profiles.sh
root=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$root"
out=${1:?"usage: $0 <directory of the final_* files: where tools/profile_bench.sh and tools/pmc_bench.sh write theirs>"}
python bench.py --full > "$out/final_bench_default.json" 2> "$out/final_bench_default.err"
WM_PROFILE_MARKER=sgd_step bash tools/profile_bench.sh final_trace_simclr_r18 10 14 --no-kernel-timer
WM_PROFILE_MARKER=adamw_kernel bash tools/profile_bench.sh final_trace_dino_vit_tiny 10 14 --workload dino_vit_tiny --no-kernel-timer
WM_PROFILE_MARKER=adamw_kernel bash tools/profile_bench.sh final_trace_dino_vit_small 10 14 --workload dino_vit_small --no-kernel-timer
WM_PROFILE_MARKER=adamw_kernel bash tools/profile_bench.sh final_trace_mae_vit_small_16 10 14 --workload mae_vit_small_16 --no-kernel-timer
for w in dino_vit_tiny dino_vit_small mae_vit_small_16 mae_vit_b_32; do
  python bench.py --full --workload $w --steps 30 --warmup 5 --no-cpu-baseline > "$out/final_bench_$w.json" 2>/dev/null
done
python bench.py --workload knn_allpairs --batch 64 --steps 200 --warmup 20 > gpurun_out/final_bench_knn_allpairs_b64.json 2>/dev/null
python bench.py --workload knn_allpairs --steps 50 --warmup 5 > gpurun_out/final_bench_knn_allpairs.json 2>/dev/null
python bench.py --workload knn_allpairs --sharded --batch 64 --steps 200 --warmup 20 > gpurun_out/final_bench_knn_allpairs_b64_sharded.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp && cd "$root"
rm -rf gpurun_out/final_trace_knn
rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/final_trace_knn -o p -- python3 tools/knn_one.py 64 bf16 > /dev/null 2>&1
python3 tools/summarize_profile.py gpurun_out/final_trace_knn gpurun_out/final_trace_knn_b64.md 5 "python tools/knn_one.py 64 bf16 (5 calls of wm_knn_topk: 64 bf16 queries x 811 457 x 128 bank, k = 8) under rocprofv3 --kernel-trace --stats; per 'step' = per call"
rm -rf gpurun_out/final_trace_knn
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/final_smoke.txt 2>&1
ls -la gpurun_out/final_*
