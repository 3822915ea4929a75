#!/bin/bash
# usage: tools/gpu_ab.sh "<ENV=val ...>" ["<ENV=val ...>" ...] -- A/B of bench step times under different env settings on ONE box
# logs and traces go to $OUT_DIR (default tool_out/); the bench runs use --full (stage step, output checks)
# (each arm is checked bit-exact against the reference golden by bench.py's verify, outside the timed region); AB_ARGS adds bench flags
cd "$GRAFT_REPO_ROOT" || exit 1
out=${OUT_DIR:-tool_out}; mkdir -p $out; : > $out/ab.log
for e in "$@"; do
  echo "== $e" | tee -a $out/ab.log
  env $e timeout -k 10 200 python bench.py --full --steps ${AB_STEPS:-10} --warmup 2 --no-cpu-baseline --no-extra $AB_ARGS 2>$out/ab_last.err | grep -o '"ms_per_step": [0-9.]*\|"median_step_ms": [0-9.]*\|"stage_ms_per_step": {[^}]*}\|"bit_exact_vs_reference_js": [a-z]*\|"bwt_rounds": [0-9]*' | tr '\n' ' ' | tee -a $out/ab.log || { tail -5 $out/ab_last.err; exit 1; }
  echo | tee -a $out/ab.log
done
