# round 5: GPU test suite, per-configuration counters, the bench line
OUT=${1:?usage: bash $0 OUTPUT_DIR}  # (was r05c)
mkdir -p "$OUT"
timeout 1200 python -m pytest tests -x -q -m gpu > $OUT/gputests.log 2>&1; echo "rc=$?" >> $OUT/gputests.log
grep -v "^t: \|^total cost\|^start\|^goal" $OUT/gputests.log | tail -5
bash profiles/run_round5_counters.sh r05ctr > $OUT/counters.log 2>&1
tail -5 $OUT/counters.log
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
tail -c 1500 $OUT/bench.json
