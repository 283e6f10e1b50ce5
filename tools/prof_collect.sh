#!/bin/bash
# Assemble profiles/rNN_* from what tools/prof_round.sh + tools/pmc_round.sh (+ a `bench.py --full` run saved as
# $OUT/bench_default.log, tools/patch_bench.py -> $OUT/r2/patch_bench.json) left under $OUT (default tool_out/).
#   bash tools/prof_collect.sh r02        (run in the repo root; PROF_DIR=r4prof for the directory tools/prof_round.sh writes now)
set -e
R=${1:-r02}
O=${OUT:-tool_out}
one() {  # name, bench args, output file
  [ -f $O/${PROF_DIR:-prof}/$1_kernel_stats.csv ] || return 0
  { echo "# rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py $2 --full --no-cpu-baseline   (tools/prof_round.sh, one MI355X)"
    echo "# bench line of the same run:"
    echo "# $(grep "^{\"metric\"" $O/${PROF_DIR:-prof}/$1.json.log | tail -1 | cut -c1-330)"
    grep -v "at::native\|rocclr" $O/${PROF_DIR:-prof}/$1_kernel_stats.csv | cut -c1-260; } > profiles/$3
}
one vitb "" ${R}_bench_kernel_stats.txt
one medsam_b1 "--model medsam --batch 1" ${R}_medsam_b1_kernel_stats.txt
one medsam_b16 "--model medsam --batch 16 --steps 10" ${R}_medsam_b16_kernel_stats.txt
one vitl_dense "--model vit_large14_336 --batch 64 --out dense --steps 10" ${R}_vitl_dense_kernel_stats.txt
one vitg_fp8 "--model dinov2_giant14_224 --batch 32 --fp8 --steps 10" ${R}_vitg_fp8_kernel_stats.txt
one vitg_bf16 "--model dinov2_giant14_224 --batch 32 --steps 10" ${R}_vitg_bf16_kernel_stats.txt
cp $O/pmc_summary.txt profiles/${R}_pmc_traffic.txt
cp $O/pmc_summary.json profiles/${R}_pmc_traffic.json
[ -f $O/r2/patch_bench.json ] && cp $O/r2/patch_bench.json profiles/${R}_patch_embed_gbs.json
if [ -f $O/bench_default.log ]; then
  grep "^{\"metric\"" $O/bench_default.log | tail -1 > profiles/${R}_bench_default.json.log
  python3 tools/roofline_table.py profiles/${R}_bench_default.json.log > profiles/${R}_roofline_table.md
fi
ls -la profiles/${R}_*
