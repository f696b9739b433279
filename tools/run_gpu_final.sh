set -e
python -m pytest tests -m gpu -x -q 2>&1 | tail -2
python bench.py --full 2>&1 | tail -1
python bench.py --full --no-cpu-baseline --strict-border 0 2>&1 | tail -1
ROOT=$(pwd); OUT=${OUT:-$ROOT/prof_out}; mkdir -p $OUT  # (kernel statistics land in prof_out/ unless OUT says otherwise)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_d -o r01d -- python3 $ROOT/bench.py --full --no-cpu-baseline > $OUT/prof_d.log 2>&1
tail -1 $OUT/prof_d.log | cut -c1-120
