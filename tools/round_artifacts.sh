# the round's kept artifacts (GPU box, repo root): bench line, rocprofv3 kernel stats, the slow GPU tests, side measurements
# usage: tools/round_artifacts.sh <out dir>
OUT=${1:?usage: tools/round_artifacts.sh <out dir>}; mkdir -p "$OUT"
python bench.py --full > $OUT/r6_bench_line.json 2> $OUT/r6_bench_err.txt; tail -c 600 $OUT/r6_bench_err.txt
tools/profile_round.sh r06 > $OUT/r6_profile_round.txt 2>&1
LT_RUN_SLOW=1 python -m pytest tests -q -m "gpu and slow" > $OUT/r6_slow_tests.txt 2>&1; tail -3 $OUT/r6_slow_tests.txt
python tools/shard_time.py 21 delta,sparse > $OUT/r6_shard_time.txt 2>&1; tail -2 $OUT/r6_shard_time.txt
(python tools/shard_step_time.py delta 500; python tools/shard_step_time.py delta 2000) > $OUT/r6_shard_step.txt 2>&1; tail -8 $OUT/r6_shard_step.txt
python tools/stageb_lab2.py delta > $OUT/r6_stageb_lab2.txt 2>&1; tail -9 $OUT/r6_stageb_lab2.txt
python tools/hub_noise.py > $OUT/r6_hub_noise.txt 2>&1; tail -3 $OUT/r6_hub_noise.txt
python tools/balanced_full_time.py > $OUT/r6_balanced.txt 2>&1; tail -3 $OUT/r6_balanced.txt
