# Round-end evidence: full GPU suite, smoke, default bench line, and the
# rocprofv3 kernel-trace summary of a short bench run (copied to profiles/ by hand: kernel_stats.csv, bench line, test tail).
# Usage (GPU box): TAG=r02a bash tools/gpu/round.sh
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and JSON lines go
mkdir -p $OUT
export TMPDIR=/tmp
T=${TAG:-r02}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/${T}_gpu_tests.log 2>&1 || { echo "tests failed"; tail -30 $OUT/${T}_gpu_tests.log; exit 1; }
tail -2 $OUT/${T}_gpu_tests.log
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.log 2>&1 || { echo smoke failed; cat $OUT/${T}_smoke.log; exit 1; }
tail -1 $OUT/${T}_smoke.log
timeout -k 10 400 python bench.py --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || { echo bench failed; tail $OUT/${T}_bench.err; exit 1; }
tail -1 $OUT/${T}_bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof -o run --output-format csv -- python bench.py --full --steps 50 --no-pmc --no-cpu --no-cli --fp32-steps 0 > $OUT/${T}_prof_bench.json 2>$OUT/${T}_prof.err || { echo prof failed; tail $OUT/${T}_prof.err; exit 1; }
find $OUT/${T}_prof -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $OUT/${T}_kernel_stats.csv
head -8 $OUT/${T}_kernel_stats.csv
