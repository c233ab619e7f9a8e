#!/bin/bash
# final measurement pass of the round (on an MI355X, from the repository root): ST_PROF_OUT=DIR bash tools/final_prof.sh [TAG=r6]
# bench lines (configs[1] with the product harness, configs[2], configs[3], 2-rank gloo rehearsal) + rocprof kernel stats of the same
# command + trace overlap + per-shape table with PMC traffic + SQ counters of the fused MLP kernel.  Everything lands under DIR;
# copy what is to be judged into profiles/.
export TMPDIR=/tmp
TAG=${1:-r6}
OUT=${ST_PROF_OUT:?set ST_PROF_OUT to the folder that receives the results}
mkdir -p "$OUT"
set -x
python bench.py --full --no-cpu-baseline 2>$OUT/${TAG}_bench.err | grep '^{' > $OUT/${TAG}_bench_nocpu.json
python bench.py --full --batch 8 --streams 2 --steps 30 --warmup 4 --no-cpu-baseline 2>/dev/null | grep '^{' > $OUT/${TAG}_bench_batch8.json
# clean kernel table of the batch-8 forward (one stream: rocprof durations are then stand-alone; two streams overlap inside the trace)
rm -rf $OUT/prof_b8
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_b8 -o p -- python3 bench.py --batch 8 --streams 1 --steps 20 --warmup 4 > $OUT/prof_b8.log 2>&1
S8=$(find $OUT/prof_b8 -name "*kernel_stats.csv" | head -1)
cp $S8 $OUT/${TAG}_bench_batch8_kernel_stats.csv
python tools/kernel_stats_summary.py $S8 > $OUT/${TAG}_bench_batch8_kernel_summary.txt
rm -rf $OUT/prof_b8
# pairs/s over (batch, streams)
for cfg in "1 3" "2 3" "4 2" "4 3" "8 1" "8 2"; do set -- $cfg; steps=$((160 / $1)); [ $steps -lt 20 ] && steps=20
  python bench.py --full --batch $1 --streams $2 --steps $steps --warmup 6 --no-cpu-baseline --no-corr-roofline --harness none 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print('batch $1 streams $2:', round(d['value'], 2), 'pairs/s', round(d['ms_per_step'], 3), 'ms/step; GEMM family frac', round(d['roofline']['frac'], 4))"
done > $OUT/${TAG}_batch_sweep.txt
cat $OUT/${TAG}_batch_sweep.txt
# the product harness with 2 pairs per forward (the sweep's best point) beside the default bench line's 4
python bench.py --full --no-cpu-baseline --no-corr-roofline --harness-batch 2 2>/dev/null | grep '^{' > $OUT/${TAG}_bench_harness_batch2.json
python -c "
import json
for f in ('${TAG}_bench_nocpu', '${TAG}_bench_harness_batch2'):
    d = json.load(open('$OUT/' + f + '.json')); print(f, 'value', round(d['value'], 2), 'harness', round(d['harness_pairs_per_s'], 2), 'batched', round(d['harness_batched_pairs_per_s'], 2))
" > $OUT/${TAG}_harness_batch.txt; cat $OUT/${TAG}_harness_batch.txt
python bench.py --full --workload 1024 --steps 60 --warmup 8 --no-cpu-baseline 2>/dev/null | grep '^{' > $OUT/${TAG}_bench_1024.json
rm -rf $OUT/prof_final
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final -o p -- python3 bench.py > $OUT/prof_final.log 2>&1
S=$(find $OUT/prof_final -name "*kernel_stats.csv" | head -1)
cp $S $OUT/${TAG}_bench_kernel_stats.csv
python tools/kernel_stats_summary.py $S $(python - <<PY
import csv
rows=list(csv.DictReader(open("$S")))
print(next(int(r["Calls"]) for r in rows if "flow_warp_kernel" in r["Name"]))
PY
) $OUT/${TAG}_kernel_summary.json > $OUT/${TAG}_kernel_summary.txt
python tools/trace_overlap.py $(find $OUT/prof_final -name "*kernel_trace.csv" | head -1) > $OUT/${TAG}_trace_overlap.txt
tail -3 $OUT/${TAG}_kernel_summary.txt
bash tools/run_pmc_shapes.sh $TAG
bash tools/dma_gemm_pmc.sh > /dev/null 2>&1
tail -n 3 gpurun_out/r5_dma_gemm_sq_counters.txt
bash tools/mfma_util.sh > $OUT/${TAG}_mfma_utilisation.txt 2>/dev/null
bash tools/mlp_split3_pmc.sh > /dev/null 2>&1
python tools/mlp_split3_probe.py --json $OUT/${TAG}_mlp_split3_probe.json > $OUT/${TAG}_mlp_split3_probe.txt 2>/dev/null
tools/probes/_bin/mbc > $OUT/${TAG}_mfma_bf16_chain.txt 2>/dev/null
tail -n 3 $OUT/${TAG}_mfma_utilisation.txt
python tools/bench_out_harness.py 48 2>/dev/null | grep '^{' > $OUT/${TAG}_out_harness.json; cat $OUT/${TAG}_out_harness.json
python bench.py --full 2>>$OUT/${TAG}_bench.err | grep '^{' > $OUT/${TAG}_bench.json
# 2-rank rehearsal of the launcher / sharding / all-gather on the 1-GPU box (both ranks on cuda:0, gloo): bounded, last
timeout -k 10 300 python bench.py --full --gpus 2 --backend gloo --share-gpu --steps 40 --warmup 6 --no-cpu-baseline --no-corr-roofline --harness-pairs 48 2>$OUT/${TAG}_bench_2rank.err | grep '^{' > $OUT/${TAG}_bench_2rank_gloo_share_gpu.json
python -c "
import json
for f in ('${TAG}_bench', '${TAG}_bench_batch8', '${TAG}_bench_1024', '${TAG}_bench_2rank_gloo_share_gpu'):
    try: d = json.load(open('$OUT/' + f + '.json'))
    except Exception as e: print(f, 'missing', e); continue
    print(f, round(d['value'], 2), d.get('harness_pairs_per_s'), d.get('value_1_in_flight'), round(d['roofline']['frac'], 4))
"
