#!/bin/bash
# usage (on the GPU box, from the repo root): tools/pmc.sh <tag> "<counters>" [bench args...]
# One rocprofv3 --pmc pass of a short bench run; CSVs land in $VETO_PROFILE_OUT/pmc_<tag>/ (default profile_out/).
tag=$1; ctrs=$2; shift 2
R=$PWD
OUT=$(realpath -m "${VETO_PROFILE_OUT:-profile_out}"); mkdir -p "$OUT"
export TMPDIR=/tmp
cd /tmp && rocprofv3 --pmc $ctrs --kernel-trace --output-format csv -d $OUT/pmc_$tag -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > $OUT/pmc_$tag.log 2>&1
echo "pmc $tag rc=$?"
