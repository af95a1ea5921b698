OUT=${1:?usage: bash $0 OUTPUT_DIR}  # (was r05e)
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -x -q -m gpu > $OUT/gputests.log 2>&1; echo "rc=$?" >> $OUT/gputests.log
grep -av "^t: \|^total cost\|^start\|^goal" $OUT/gputests.log | grep -a "passed\|failed\|rc=\|Error\|assert" | tail -12
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
tail -c 600 $OUT/bench.json
