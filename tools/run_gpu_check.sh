set -e
python -m pytest tests -m gpu -x -q 2>&1 | tail -3
python bench.py --full --no-cpu-baseline 2>&1 | tail -1
python bench.py --full --no-cpu-baseline --strict-border 0 2>&1 | tail -1
ROOT=$(pwd); OUT=${OUT:-$ROOT/prof_out}; mkdir -p $OUT  # (kernel statistics land in prof_out/ unless OUT says otherwise)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c -o r01c -- python3 $ROOT/bench.py --full --no-cpu-baseline --steps 100 --warmup 20 > $OUT/prof_c.log 2>&1
