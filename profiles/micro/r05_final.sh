# closing runs of round 5: the GPU suite, the smoke entry, the bench line alone and under rocprofv3
OUT=${1:?usage: bash $0 OUTPUT_DIR}  # (was r05z)
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -x -q -m gpu > $OUT/gputests.log 2>&1; echo "rc=$?" >> $OUT/gputests.log
grep -av "^t: \|^total cost\|^start\|^goal" $OUT/gputests.log | grep -a "passed\|failed\|rc=\|Error\|assert" | tail -6
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -1 $OUT/smoke.log
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -f csv -d $OUT/kt -o kt -- python bench.py --full --no-extras --no-cpu-baseline > $OUT/bench_under_rocprof.json 2> $OUT/kt.err
for f in $(find $OUT/kt -name '*kernel_stats.csv'); do cp "$f" $OUT/c4_kernel_stats_final.csv; done
head -3 $OUT/c4_kernel_stats_final.csv | cut -c1-200
tail -c 200 $OUT/bench_under_rocprof.json
