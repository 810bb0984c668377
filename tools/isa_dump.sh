#!/bin/bash
# Dump the gfx950 assembly of every MSV, Viterbi, Forward, domain and alignment kernel translation unit into $1
# (one .s per TU), for instruction-for-instruction comparisons of a source change (tools/isa_compare.py).
set -e
OUT=${1:?usage: tools/isa_dump.sh OUTDIR}
HERE=$(cd "$(dirname "$0")/../hmm_fasta_viterbi_amd/csrc" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
mkdir -p "$OUT"
FLAGS="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -fno-honor-nans -fno-slp-vectorize -ffp-contract=off -I$ROOT/include -I$HERE --cuda-device-only -S"
for k in 0 1 2 3 4 5 6 7; do
  /opt/rocm/bin/hipcc $FLAGS -DMSV_PART=$k -DMSV_PART_INC="\"msv_variants_$k.inc\"" "$HERE/msv_kernel_part.hip" -o "$OUT/part$k.s" &
done
for tu in msv_kernel msv_coop vit_kernel vit_team vit_trace fwd_kernel dom_kernel aln_kernel; do
  /opt/rocm/bin/hipcc $FLAGS "$HERE/$tu.hip" -o "$OUT/$tu.s" &
done
wait
