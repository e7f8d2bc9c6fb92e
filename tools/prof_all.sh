#!/bin/bash
# Evidence run for profiles/ (on the GPU box: tools/prof_all.sh TAG): the default bench line, the train-mode lines, rocprofv3
# kernel-trace stats of the same bench commands, the two HBM traffic counter passes (FETCH_SIZE / WRITE_SIZE: separate --pmc passes
# with kernel-trace only, as the MI355X guide prescribes), the MFMA-busy / clock pass and the conv3x3_v6 stamps.
# Results land in $OUT/TAG/ (OUT: tools/steps.sh), which must not exist yet; tools/prof_collect.py TAG then writes profiles/TAG_* from them.
# Every program that opens the GPU goes through `step` (tools/steps.sh): a time limit of its own, and the script ends at the first
# failure.  Beside each step: its wall time on an MI355X box with 16 CPUs; the limit is at least five times that, for a cold start.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
source $R/tools/steps.sh
TAG=${1:?usage: tools/prof_all.sh TAG}
O=$OUT/$TAG
[ ! -e $O ] || { echo "$O exists already: choose another TAG" >&2; exit 2; }
mkdir -p $O
RAW=$(mktemp -d); trap 'rm -r "$RAW"' EXIT       # rocprofv3's raw output (its working directory too): only the CSVs kept below survive
keep() { find $RAW/$1 -name "*$2" -exec cp {} $O/$3 \; ; }
cd $R
step 120 $O/bench.err python bench.py --steps 20 --warmup 3 > $O/bench_steps20.json                                # 24 s
step 60 $O/bench.err python bench.py --mode train --steps 5 > $O/bench_train.json                                 # 5 s
step 60 $O/bench.err python bench.py --mode train --precision bf16x3 --steps 5 > $O/bench_train_x3.json           # 4 s
step 60 $O/bench.err python bench.py --precision bf16x3 --steps 10 --warmup 2 --no-extras --no-cpu-baseline > $O/bench_x3_steps10.json   # 5 s
step 60 $O/kbench.err python tools/kbench.py bf16x3 > $O/kbench_x3.txt                                            # 2 s
step 60 $O/kbench.err python tools/kbench.py bf16 32 32 512 > $O/kbench_c5.txt                                    # 6 s
if [ -f scratch/x/v6_stamp/lib.so ]; then                                                                          # not measured: two forwards more than kbench.py
  HRNET_HIP_LIB=scratch/x/v6_stamp/lib.so step 60 $O/v6_stamps.err python tools/stamps/read_v6.py > $O/v6_stamps.txt
fi
cd $RAW
step 60 $O/stats.err rocprofv3 --kernel-trace --stats --output-format csv -d $RAW/stats -o s -- python3 $R/bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-extras > $O/bench_steps5_under_rocprof.json   # 4 s
step 60 $O/stats_x3.err rocprofv3 --kernel-trace --stats --output-format csv -d $RAW/stats_x3 -o s -- python3 $R/bench.py --precision bf16x3 --steps 3 --warmup 1 --no-cpu-baseline --no-extras > /dev/null   # 5 s
step 60 $O/stats_tr.err rocprofv3 --kernel-trace --stats --output-format csv -d $RAW/stats_tr -o s -- python3 $R/bench.py --mode train --steps 3 --warmup 1 > /dev/null   # 5 s
step 60 $O/stats_trx3.err rocprofv3 --kernel-trace --stats --output-format csv -d $RAW/stats_trx3 -o s -- python3 $R/bench.py --mode train --precision bf16x3 --steps 3 --warmup 1 > /dev/null   # 4 s
step 60 $O/pmc_fetch.err rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $RAW/pmc_fetch -o f -- python3 $R/tools/kbench.py bf16 > $O/pmc_fetch.out   # 3 s
step 60 $O/pmc_write.err rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $RAW/pmc_write -o w -- python3 $R/tools/kbench.py bf16 > $O/pmc_write.out   # 3 s
step 60 $O/pmc_busy.err rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES --kernel-trace --output-format csv -d $RAW/pmc_busy -o t -- python3 $R/tools/kbench.py bf16 > $O/pmc_busy.out   # 2 s
cd $R
keep stats kernel_stats.csv bench_steps5_kernel_stats.csv
keep stats_x3 kernel_stats.csv x3_kernel_stats.csv
keep stats_tr kernel_stats.csv train_kernel_stats.csv
keep stats_trx3 kernel_stats.csv train_x3_kernel_stats.csv
keep pmc_fetch counter_collection.csv pmc_fetch_counter_collection.csv
keep pmc_write counter_collection.csv pmc_write_counter_collection.csv
keep pmc_busy counter_collection.csv pmc_busy_cc.csv
keep pmc_busy kernel_trace.csv pmc_busy_kt.csv
python tools/pmc_busy_summary.py $O/pmc_busy_kt.csv $O/pmc_busy_cc.csv | tee $O/pmc_busy_summary.txt
ls $O; du -sh $O
