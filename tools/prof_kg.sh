set -o pipefail
cd /root/repo
export TMPDIR=/tmp
O=${1:-build/prof_kg}; mkdir -p "$O"
for v in 0 9; do
  GV_KG=$v timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/prof_kg$v" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-extras --no-cpu-baseline --no-latency > "$O/prof_kg$v.json" 2> "$O/prof_kg$v.err" || exit 1
done
