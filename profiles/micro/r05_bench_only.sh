OUT=${1:?usage: bash $0 OUTPUT_DIR}  # (was r05f)
mkdir -p "$OUT"
timeout 600 python -m pytest tests/test_gpu_post.py tests/test_lpastar.py tests/test_gpu_plan.py -x -q -m gpu > $OUT/tests.log 2>&1; echo "rc=$?" >> $OUT/tests.log
grep -av "^t: \|^total cost\|^start\|^goal" $OUT/tests.log | grep -a "passed\|failed\|rc=\|Error\|assert" | tail -6
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
tail -c 300 $OUT/bench.json
