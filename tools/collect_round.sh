#!/bin/bash
# Round evidence on the GPU box (writes under profile_out/<tag>*): kernel stats + step timeline of the default bench command, the PMC
# traffic passes (f16 and f32 legs), the instruction-mix / MFMA-busy passes, the default bench line with the shape table.  Every JSON
# summary carries _source.code_tree_sha (tools/tree_sha.py) of the code it was taken on; bench.py prints `stale` against the running tree
# and tools/check_profiles.py refuses summaries of another tree.
# usage: tools/collect_round.sh <tag>
tag=$1
export TMPDIR=/tmp
cd "$(dirname "$0")/.." && mkdir -p profile_out
rm -rf profile_out/$tag profile_out/${tag}_f profile_out/${tag}_w profile_out/${tag}_A profile_out/${tag}_B
rocprofv3 --kernel-trace --stats -d profile_out/$tag -o $tag --output-format csv -- python bench.py --full --steps 5 --warmup 2 --no-cpu --no-f32 --no-extra > profile_out/$tag.log 2>&1
python tools/stats_to_txt.py $(find profile_out/$tag -name "*kernel_stats.csv" | head -1) "rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 5 --warmup 2 --no-cpu --no-f32 --no-extra  (ukbb192, batch 32, f16, 1 x MI355X; 27 train steps incl. 20 preparation steps + the eager profiling step, then the counterfactual loop); code tree $(python tools/tree_sha.py)" > profile_out/${tag}_kernel_stats.txt
python tools/timeline.py $(find profile_out/$tag -name "*kernel_trace.csv" | head -1) profile_out/${tag}_step_timeline.txt > /dev/null 2>&1
rm -rf profile_out/$tag
for dt in f16 f32; do
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d profile_out/${tag}_f -o f --output-format csv -- python bench.py --full --dtype $dt --steps 2 --warmup 1 --prep-steps 1 --no-cpu --no-cf --no-f32 --no-extra > profile_out/${tag}_f.log 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE -d profile_out/${tag}_w -o w --output-format csv -- python bench.py --full --dtype $dt --steps 2 --warmup 1 --prep-steps 1 --no-cpu --no-cf --no-f32 --no-extra > profile_out/${tag}_w.log 2>&1
  python tools/pmc_traffic.py $(find profile_out/${tag}_f -name "*counter_collection.csv" | head -1) $(find profile_out/${tag}_w -name "*counter_collection.csv" | head -1) profile_out/${tag}_hbm_traffic_${dt}_b32.json > /dev/null
  rm -rf profile_out/${tag}_f profile_out/${tag}_w
done
bash tools/pmc_insts.sh ${tag} python bench.py --full --steps 1 --warmup 1 --prep-steps 1 --no-cpu --no-cf --no-f32 --no-extra
python tools/pmc_insts.py profile_out/${tag} > profile_out/${tag}_instruction_mix.txt 2>&1
python tools/pmc_classes.py profile_out/${tag} > profile_out/${tag}_mfma_busy_by_class.json 2>profile_out/${tag}_mfma_busy.err
rm -rf profile_out/${tag}_A profile_out/${tag}_B
ls -la profile_out | grep $tag
