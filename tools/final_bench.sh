#!/bin/bash
# Last step of a collection (tools/collect_round.sh <tag> PART=1..3 + tools/install_round.py <tag> come first): the three default bench lines again AFTER the PMC summaries of
# this tree were installed under profiles/ (bench.py fills roofline.traffic only from a file whose csrc_sha matches), then tools/install_round.py <tag> once more.
# usage (from the repo root): bash tools/final_bench.sh r06 <out_dir>   (the folder tools/install_round.py reads the *_bench_final.json lines from)
TAG=${1:-r06}
OUT=$(realpath -m "${2:?usage: bash tools/final_bench.sh <tag> <out_dir>}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
python3 bench.py --full > "$OUT/${TAG}_bench_final.json" 2> "$OUT/bf.err"
python3 bench.py --full --config 3 > "$OUT/${TAG}_base384_bench_final.json" 2>> "$OUT/bf.err"
python3 bench.py --full --config 2 > "$OUT/${TAG}_hybrid384_bench_final.json" 2>> "$OUT/bf.err"
python3 -c "
import json
for t in ('$TAG','${TAG}_base384','${TAG}_hybrid384'):
    d=json.loads(open('$OUT/%s_bench_final.json'%t).read().strip().splitlines()[-1]); print(t, d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['traffic'], d['roofline_hbm']['frac'], d['tolerance']['worst_measured'], d['pipelined']['value'])
"
