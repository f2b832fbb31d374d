#!/bin/bash
# Round-end style run on the GPU box: the default bench (JSON line ->
# ${OUT:-bench_out}/bench.json), the rocprofv3 kernel-trace summary of the same
# command, and the FETCH_SIZE / WRITE_SIZE passes for the traffic figures.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
export ZD_CORPUS_CACHE=/tmp/zdc
timeout -k 10 900 python bench.py --full > ${OUT:-bench_out}/bench.json 2> ${OUT:-bench_out}/bench.err; rc=$?
echo "bench rc=$rc"; tail -3 ${OUT:-bench_out}/bench.err; cat ${OUT:-bench_out}/bench.json
[ $rc -eq 0 ] || exit $rc
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof_full -o run --output-format csv -- python bench.py --full --no-cpu-baseline > ${OUT:-bench_out}/bench_prof.json 2> ${OUT:-bench_out}/bench_prof.err; rc=$?
echo "prof rc=$rc"
[ $rc -eq 0 ] || exit $rc
B="python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-verify"
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d ${OUT:-bench_out}/pmc_fetch -o run --output-format csv -- $B > ${OUT:-bench_out}/pmc_fetch.log 2>&1; rc=$?
echo "fetch rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d ${OUT:-bench_out}/pmc_write -o run --output-format csv -- $B > ${OUT:-bench_out}/pmc_write.log 2>&1; rc=$?
echo "write rc=$rc"; [ $rc -eq 0 ] || exit $rc
python scripts/pmc_traffic.py ${OUT:-bench_out}/pmc_fetch ${OUT:-bench_out}/pmc_write ${OUT:-bench_out}/traffic.json "${1:-}"
