#!/bin/bash
set -euo pipefail          # the first failing pass ends the run; every pass runs under its own time limit
# PMC passes over the batched FGW solve (tools/fgw_pmc.py): each pass in its own run, --pmc with --kernel-trace only.
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/${1:-fgw_pmc}; mkdir -p $O; cd /tmp; export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU --output-format csv -d $O/p1 -o a -- python3 $R/tools/fgw_pmc.py > $O/p1.log 2>&1
timeout -k 10 900 rocprofv3 --kernel-trace --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU SQ_INSTS_SMEM SQ_BUSY_CYCLES --output-format csv -d $O/p2 -o b -- python3 $R/tools/fgw_pmc.py > $O/p2.log 2>&1
timeout -k 10 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/p3 -o c -- python3 $R/tools/fgw_pmc.py > $O/p3.log 2>&1
timeout -k 10 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/p4 -o d -- python3 $R/tools/fgw_pmc.py > $O/p4.log 2>&1
python3 $R/tools/pmc_dump.py "fgw" $O/p1 $O/p2 $O/p3 $O/p4 | tee $O/summary.txt
python3 $R/tools/pmc_sq.py $O/p1 $O/fgw_pmc_sq.json "tools/fgw_pmc.py (3 batched FGW solves at cfg2 shape)" > /dev/null 2>&1
python3 $R/tools/pmc_summary.py $O/p3 $O/p4 $O/fgw_pmc_hbm.json "tools/fgw_pmc.py (3 batched FGW solves at cfg2 shape)" > /dev/null 2>&1
find $O -name "*.db" -delete
