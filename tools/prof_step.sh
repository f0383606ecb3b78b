# usage: bash tools/prof_step.sh <tag>   (on an MI355X) -> profile_out/<tag>/: kernel stats of a full bench run
R=$(cd "$(dirname "$0")/.." && pwd) && mkdir -p $R/profile_out && cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $R/profile_out/$1 -o $1 -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-profile > $R/profile_out/$1.log 2>&1
ls $R/profile_out/$1
