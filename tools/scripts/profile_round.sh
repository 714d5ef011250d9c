# usage (on the GPU box, from the repo root): bash tools/scripts/profile_round.sh <tag> [<output dir>]
# separate PMC passes (FETCH_SIZE / WRITE_SIZE), rocprofv3 kernel traces of bench.py --full, then the full bench line (which quotes the
# fresh PMC traffic); everything lands in <output dir>/<tag>_* (default profile_out/ in the repo root; + profiles/<tag>_* written by
# summarize_prof.py)
set -euo pipefail
TAG=${1:-r01_final}
R=${GRAFT_REPO_ROOT:?set GRAFT_REPO_ROOT (the repo root on the GPU box)}
O=$(realpath -m ${2:-$R/profile_out})
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE -d $O/${TAG}_pmc_fetch -o f --output-format csv -- python3 $R/tools/prof_kernels.py > $O/${TAG}_pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/${TAG}_pmc_write -o w --output-format csv -- python3 $R/tools/prof_kernels.py > $O/${TAG}_pmc_write.log 2>&1
echo "pmc done"
rocprofv3 --kernel-trace --stats -d $O/${TAG}_kt_spmv -o kt --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --no-extras > $O/${TAG}_spmv_only_bench.json 2> $O/${TAG}_kt_spmv.err
echo "spmv-only trace done"
# the root rebalance alone (2^24 slots: every k_move2<false,...> row of this trace is that window), warm and cold; the SpMV cold
rocprofv3 --kernel-trace --stats -d $O/${TAG}_kt_reb -o kt --output-format csv -- python3 $R/tools/prof_rebalance.py warm 30 > $O/${TAG}_kt_reb.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/${TAG}_kt_rebcold -o kt --output-format csv -- python3 $R/tools/prof_rebalance.py cold 12 > $O/${TAG}_kt_rebcold.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/${TAG}_kt_spmvcold -o kt --output-format csv -- python3 $R/tools/prof_spmv.py cold > $O/${TAG}_kt_spmvcold.log 2>&1
echo "rebalance-only / cold traces done"
rocprofv3 --kernel-trace --stats -d $O/${TAG}_kt -o kt --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline > $O/${TAG}_kt_bench.json 2> $O/${TAG}_kt.err
echo "full trace done"
cd $R
python3 tools/summarize_prof.py $TAG $O/${TAG}_kt $O/${TAG}_pmc_fetch $O/${TAG}_pmc_write > $O/${TAG}_summary.log 2>&1
cp profiles/${TAG}_kernel_stats.csv $O/${TAG}_kernel_stats.csv
cp profiles/${TAG}_pmc_summary.json $O/${TAG}_pmc_summary.json
python3 - "$O" "$TAG" <<'PY'
import glob, shutil, sys
out, tag = sys.argv[1:3]
f = glob.glob("%s/%s_kt_spmv/**/*kernel_stats.csv" % (out, tag), recursive=True)
if f: shutil.copy(f[0], "%s/%s_spmv_only_kernel_stats.csv" % (out, tag))
for sub, name in (("kt_reb", "rebalance_only"), ("kt_rebcold", "rebalance_cold"), ("kt_spmvcold", "spmv_cold")):
    f = glob.glob("%s/%s_%s/**/*kernel_stats.csv" % (out, tag, sub), recursive=True)
    if f: shutil.copy(f[0], "%s/%s_%s_kernel_stats.csv" % (out, tag, name))
PY
cd /tmp
python3 $R/bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
echo "bench done"
tail -c 2500 $O/${TAG}_bench.json
