#!/bin/bash
# The round's evidence in one GPU-box call: GPU tests, profile rounds (C2, C3, C5: kernel trace + separate PMC passes), the
# driver's bench command (C2 line with C3 / C5 embedded, reading the PMC files of this same build), the plain lines of every
# config, the full-size reference pin.   bash tools/final_evidence.sh <tag>
TAG=${1:-rXX}
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout 900 python -m pytest tests -m gpu -q 2>&1 | tail -6 > $OUT/${TAG}_gputests.txt
for C in C2 C3 C5; do bash tools/profile_round.sh $TAG $C > /dev/null 2>&1; done
cp gpurun_out/pmc_traffic*.json gpurun_out/trace_timed_region*.json profiles/ 2>/dev/null
timeout 1500 python bench.py --full --gpus 1 --steps 20 --warmup 5 2> $OUT/${TAG}_driver_cmd.err | tail -1 > $OUT/${TAG}_driver_cmd_bench_line.json
for f in bench_detail.json bench_detail_C3.json bench_detail_C5.json; do cp $f $OUT/${TAG}_driver_cmd_$f 2>/dev/null; done
timeout 900 python bench.py --full --no-other-configs 2> $OUT/${TAG}_c2.err | tail -1 > $OUT/${TAG}_c2_bench_line.json
cp bench_detail.json $OUT/${TAG}_c2_bench_detail.json
timeout 900 python bench.py --full --config C3 2> $OUT/${TAG}_c3.err | tail -1 > $OUT/${TAG}_c3_bench_line.json
cp bench_detail_C3.json $OUT/${TAG}_c3_bench_detail.json
timeout 900 python bench.py --full --config C5 2> $OUT/${TAG}_c5.err | tail -1 > $OUT/${TAG}_c5_bench_line.json
cp bench_detail_C5.json $OUT/${TAG}_c5_bench_detail.json
timeout 300 python bench.py --full --config C1 2> $OUT/${TAG}_c1.err | tail -1 > $OUT/${TAG}_c1_bench_line.json
timeout 600 python tests/tools/ref_pin_fullsize.py 3 $OUT/${TAG}_ref_pin_fullsize.json > $OUT/${TAG}_ref_pin_fullsize.txt 2>&1
cat $OUT/${TAG}_gputests.txt
for f in driver_cmd c2 c3 c5 c1; do cut -c1-260 $OUT/${TAG}_${f}_bench_line.json; echo; done
tail -3 $OUT/${TAG}_ref_pin_fullsize.txt
