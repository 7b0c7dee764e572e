#!/bin/bash
# Collects, on an MI355X, what tools/summarize_profiles.py condenses into profiles/: kernel-trace stats of the full
# bench command (`--full`: headline and secondary workloads), and FETCH_SIZE / WRITE_SIZE / SQ counters in SEPARATE counter passes
# (MI355X_MICROARCH.md: TCC slots; --pmc never together with other trace domains), plus the calibration copies.
# usage (from the repo root): bash tools/scripts/profile_bench.sh; then tools/summarize_profiles.py <tag> profile_out
set -e
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${PROFILE_OUT:-$R/profile_out}  # profiler output and logs (kept out of git)
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
ARGS="--no-cpu-baseline --no-fhew --steps 10 --warmup 2 --preheat-ms 0"
SEC="--full --no-cpu-baseline --no-verify-secondary --steps 2 --warmup 1 --preheat-ms 0"
SQ="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE"
# kernel-trace stats of the full bench command: headline + every secondary workload
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -- python3 $R/bench.py --full --no-cpu-baseline > $O/prof_stats.log 2>&1
echo stats done
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/prof_pmc_fetch -- python3 $R/bench.py $ARGS > $O/prof_pmc_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/prof_pmc_write -- python3 $R/bench.py $ARGS > $O/prof_pmc_write.log 2>&1
rocprofv3 --kernel-trace --pmc $SQ --output-format csv -d $O/prof_pmc_sq -- python3 $R/bench.py $ARGS > $O/prof_pmc_sq.log 2>&1
echo headline counters done
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/prof_sec_fetch -- python3 $R/bench.py $SEC > $O/prof_sec_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/prof_sec_write -- python3 $R/bench.py $SEC > $O/prof_sec_write.log 2>&1
rocprofv3 --kernel-trace --pmc $SQ --output-format csv -d $O/prof_sec_sq -- python3 $R/bench.py $SEC > $O/prof_sec_sq.log 2>&1
echo secondary counters done
if [ -x $R/tools/lab2 ]; then
  rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/prof_calib_fetch -- $R/tools/lab2 calib > $O/prof_calib_fetch.log 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/prof_calib_write -- $R/tools/lab2 calib > $O/prof_calib_write.log 2>&1
fi
echo profile_bench done
