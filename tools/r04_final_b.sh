#!/bin/bash
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p $OUT
: > $OUT/r04_batch_attn_pipe_ab.log
for cfg in "256 0" "512 0" "1024 0" "512 1"; do
  timeout -k 10 200 python tools/batch_rate.py 16 256 $cfg >> $OUT/r04_batch_attn_pipe_ab.log 2>&1 || exit 1
done
grep -v amdgpu $OUT/r04_batch_attn_pipe_ab.log
python bench.py --full > $OUT/r04_bench.json 2> $OUT/r04_bench.err && tail -c 300 $OUT/r04_bench.json && bash tools/r04_profile.sh > $OUT/r04_profile_run.log 2>&1
tail -4 $OUT/r04_profile_run.log
