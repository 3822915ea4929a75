#!/bin/bash
# usage (GPU box, repo root): tools/gpu_prof.sh <tag> "<ENV=val ...>" [extra bench args] -- kernel-trace of a 2-step bench
# logs and traces go to $OUT_DIR (default tool_out/); the bench runs use --full (stage step, output checks)
set -o pipefail
tag=$1; e=${2:-X=0}; shift 2
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
out=${OUT_DIR:-tool_out}; mkdir -p $out
rm -rf $out/prof_${tag}
env $e timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag} -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra "$@" > $out/prof_${tag}.log 2>&1 || { tail -20 $out/prof_${tag}.log; exit 1; }
f=$(ls $out/prof_${tag}/*/*kernel_trace.csv)
{ echo "== $tag ($e)"; python3 tools/prof_summary.py $f 4 ${TOPN:-16}; python3 tools/prof_timeline.py $f; } > $out/prof_${tag}.txt
head -20 $out/prof_${tag}.txt
cp $f $out/prof_${tag}_trace.csv
rm -rf $out/prof_${tag}
