# The GPU suite, the --full default line and the limiter's two shapes.  Usage: bash tools/_cmd_full.sh OUTDIR
[ -n "$1" ] || { echo "usage: bash tools/_cmd_full.sh OUTDIR" >&2; exit 2; }
out=$(realpath -m "$1")
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$out"
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -6 > "$out/pytest.txt"
timeout 600 python bench.py --full 2>&1 | tail -1 > "$out/bench_default.json"
for shape in "" "--sources 2048 --frames 32768"; do
  tag="limit$(echo $shape | tr -d ' -')"
  timeout 300 python bench.py --config limit $shape 2>&1 | tail -1 > "$out/bench_$tag.json"
done
echo done
