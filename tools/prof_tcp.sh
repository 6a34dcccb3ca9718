cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
OUT=${ARK_PROF_OUT:-prof_out}/tcp
mkdir -p $OUT
timeout -k 10 -s KILL 240 rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum -d $OUT/p1 -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-configs > $OUT/p1.log 2>&1
