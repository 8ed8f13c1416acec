cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
o=${1:?usage: round_profiles.sh <output directory>}; mkdir -p $o
python bench.py --full > $o/bench_line.json 2> $o/bench.err
cat $o/bench_line.json | cut -c1-600
bash tests/tools/prof_stats.sh r2p/stats --no-stream > $o/stats.log 2>&1; head -12 $o/stats.log
bash tests/tools/prof_traffic.sh r2p/traffic --steps 2 --warmup 1 --no-stream > $o/traffic.log 2>&1
python bench.py --bcf --steps 5 --warmup 1 --full --no-cpu-baseline > $o/bench_bcf.json 2>/dev/null; cut -c1-400 $o/bench_bcf.json
python tests/tools/c5_sanity.py 10000 2000 2>&1 | tail -2 > $o/c5.txt; cat $o/c5.txt
./tests/tools/microbench/store_bw 32 > $o/store_bw.txt 2>&1
