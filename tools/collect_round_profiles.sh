# usage (on an MI355X): bash tools/collect_round_profiles.sh <tag>
# Produces under profile_out/<tag>_*: FIRST the FETCH_SIZE / WRITE_SIZE PMC passes (resident-batch segment
# only) and their summary profiles/<tag>_pmc_fetch_write.json — so that every bench line
# written afterwards cites THIS collection's traffic figure —, then the full bench JSON (--full), the
# every-kind line, rocprofv3 kernel stats (csv) of the full command, and the other legs.
TAG=$1
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/profile_out
mkdir -p $O
ONLY="--rotate-batches 0 --no-fg-capped --no-device-targets --no-direct-head-forward --no-fp32-mfma --pipeline-examples 0 --no-extra-workloads"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/${TAG}_fetch -o ${TAG} -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-profile $ONLY > $O/${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/${TAG}_write -o ${TAG} -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-profile $ONLY > $O/${TAG}_write.log 2>&1
python $R/tools/summarize_profiles.py ${TAG} --pmc-only
cd $R
python $R/bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
python $R/bench.py --full --profile-all --no-cpu-baseline $ONLY > $O/${TAG}_bench_allkinds.json 2>> $O/${TAG}_bench.err
python $R/bench.py --workload infer --steps 3 --warmup 1 > $O/${TAG}_bench_infer.json 2>> $O/${TAG}_bench.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${TAG}_stats -o ${TAG} -- python $R/bench.py --full --no-cpu-baseline > $O/${TAG}_stats.log 2>&1
cd $R
ls $O | grep ${TAG}
python $R/bench.py --full --force-dp --no-cpu-baseline $ONLY > $O/${TAG}_bench_dp1.json 2>> $O/${TAG}_bench.err
python $R/bench.py --full --layers 101 --no-cpu-baseline $ONLY > $O/${TAG}_bench_r101.json 2>> $O/${TAG}_bench.err
# the fp32-MFMA kernels (the default arithmetic up to round 3): bench line with every GEMM kind timed + kernel stats
python $R/bench.py --full --profile-all --no-cpu-baseline $ONLY --tune split_bf16=0 > $O/${TAG}_bench_fp32_allkinds.json 2>> $O/${TAG}_bench.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${TAG}_fp32_stats -o ${TAG}_fp32 -- python $R/bench.py --full --no-cpu-baseline $ONLY --tune split_bf16=0 > $O/${TAG}_fp32_stats.log 2>&1
cd $R
python $R/bench.py --full --layers 101 --no-cpu-baseline $ONLY --tune split_bf16=0 > $O/${TAG}_bench_fp32_r101.json 2>> $O/${TAG}_bench.err
