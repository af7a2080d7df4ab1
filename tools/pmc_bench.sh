#!/bin/bash
# usage: tools/pmc_bench.sh <tag> "<counters>"   -- bench.py (2 timed steps) under rocprofv3 --pmc, own pass per counter set
cd /tmp && export TMPDIR=/tmp
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd); O=${PMC_OUT:-/tmp/srn_pmc}; mkdir -p $O      # (PMC_OUT: where the passes and the bench line go)
rocprofv3 --pmc $1 --kernel-trace -d $O/pmcb_$tag -o pmc --output-format csv -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/pmcb_$tag.log 2>&1
grep -o '"kernel_ms_avg": [0-9.]*' $O/pmcb_$tag.log
