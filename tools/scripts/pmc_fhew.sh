#!/bin/bash
# SQ counters of the fused FHEW kernels at cfg3 (bench.py's secondary block)
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${PROFILE_OUT:-$R/profile_out}  # profiler output and logs (kept out of git)
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_fhew1 -- python3 $R/bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > $O/pmc_fhew1.log 2>&1 &&
rocprofv3 --kernel-trace --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS --output-format csv -d $O/pmc_fhew2 -- python3 $R/bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > $O/pmc_fhew2.log 2>&1
echo pmc_fhew done
