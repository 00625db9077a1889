#!/bin/bash
# evidence of the round's final state: full GPU suite + smoke + default bench (with the per-launch table), rocprofv3 kernel stats and
# FETCH_SIZE / WRITE_SIZE passes of the bench command, kernel traces for the gap timelines (one frame / two frames in flight),
# kernel stats of the secondary configurations
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp
O=gpurun_out/r04F; mkdir -p $O
timeout 1500 python3 -m pytest tests -m gpu -x -q --durations=5 > $O/pytest_gpu.txt 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.txt
tail -10 $O/pytest_gpu.txt
timeout 120 python3 -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1; echo "smoke rc=$?" >> $O/smoke.txt; tail -2 $O/smoke.txt
timeout 600 python3 bench.py --full --dump-trace $O/conv_launches.txt > $O/bench_default.json 2> $O/bench_default.err; echo "bench rc=$?"; head -c 700 $O/bench_default.json; echo
timeout 300 python3 bench.py --full --frames-in-flight 1 --cpu-baseline 0 --secondary 0 > $O/bench_depth1.json 2> $O/bench_depth1.err; head -c 300 $O/bench_depth1.json; echo
CMD="python3 bench.py --full --steps 3 --warmup 1 --cpu-baseline 0 --secondary 0"
timeout 300 rocprofv3 --kernel-trace --stats -d $O/stats -o s --output-format csv -- $CMD > $O/stats.log 2>&1
timeout 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/fetch -o p --output-format csv -- $CMD > $O/fetch.log 2>&1
timeout 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/write -o p --output-format csv -- $CMD > $O/write.log 2>&1
timeout 400 rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 -d $O/busy -o p --output-format csv -- $CMD > $O/busy.log 2>&1
python3 profiles/mfma_busy.py $O/busy > $O/mfma_busy.md 2>&1; head -8 $O/mfma_busy.md
timeout 300 rocprofv3 --kernel-trace -d $O/gap1 -o p --output-format csv -- python3 bench.py --full --steps 12 --warmup 2 --cpu-baseline 0 --secondary 0 --frames-in-flight 1 > $O/gap1.log 2>&1
timeout 300 rocprofv3 --kernel-trace -d $O/gap2 -o p --output-format csv -- python3 bench.py --full --steps 20 --warmup 2 --cpu-baseline 0 --secondary 0 --frames-in-flight 2 > $O/gap2.log 2>&1
python3 profiles/step_gaps.py $(find $O/gap1 -name p_kernel_trace.csv | head -1) "one frame at a time (bench.py --full --steps 12 --warmup 2 --frames-in-flight 1)" > $O/step_gaps_1.md
python3 profiles/step_gaps.py $(find $O/gap2 -name p_kernel_trace.csv | head -1) "two frames in flight (bench.py --full --steps 20 --warmup 2, the default depth)" > $O/step_gaps_2.md
head -8 $O/step_gaps_1.md; head -8 $O/step_gaps_2.md
timeout 300 rocprofv3 --kernel-trace --stats -d $O/int -o s --output-format csv -- python3 tools/timeline_int.py > $O/int.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $O/color -o s --output-format csv -- python3 tools/timeline_color.py > $O/color.log 2>&1
timeout 400 rocprofv3 --kernel-trace --stats -d $O/train -o s --output-format csv -- python3 bench_train.py --steps 4 --warmup 1 > $O/train.log 2>&1
tail -3 $O/int.log; tail -3 $O/color.log
find $O -name 's_kernel_trace.csv' -delete; rm -f $O/write/p_kernel_trace.csv; find $O/gap1 $O/gap2 $O/busy -name p_kernel_trace.csv -delete
find $O -name '*.csv' | xargs ls -la | head -40
