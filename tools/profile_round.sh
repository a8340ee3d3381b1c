# One profiling round on the GPU box (repository root; results under out/, git-ignored): kernel-trace stats of the default bench, HBM traffic
# PMC passes of the roofline layer for the tilings the tuner chooses between, and the default bench line.
set -e
R=$PWD
O=$R/out
mkdir -p $O
export PP_TUNE_CACHE=$O/tune.cache
rm -f $PP_TUNE_CACHE
python bench.py --full --no-cpu-baseline --steps 4 --warmup 2 > $O/warm.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 $R/bench.py --full --no-cpu-baseline --no-extras > $O/prof.json 2> $O/prof.err
unset PP_TUNE_CACHE
i=0
for T in "wino tw8 w1x4 bx1 kc4" "wino tw8 w1x4 bx1 kc8" "wino tw8 w1x4 bx2 kc8" "wino tw4 w1x4 bx2 kc8"; do
  export PP_FORCE_VARIANT="$T"
  rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmcf_$i -- python3 $R/bench.py --no-cpu-baseline --no-extras --steps 3 --warmup 1 > $O/pmcf_$i.json 2> $O/pmcf_$i.err
  rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmcw_$i -- python3 $R/bench.py --no-cpu-baseline --no-extras --steps 3 --warmup 1 > $O/pmcw_$i.json 2> $O/pmcw_$i.err
  i=$((i+1))
done
unset PP_FORCE_VARIANT
cd $R
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
cat $O/prof.json $O/bench_default.json
