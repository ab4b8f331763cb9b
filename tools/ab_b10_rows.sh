OUT=${1:?usage: bash tools/ab_b10_rows.sh OUTDIR}
mkdir -p "$OUT"
run() { tag=$1; shift; env "$@" python bench.py --full --batch 10 --steps 100 > "$OUT/$tag.json" 2> "$OUT/$tag.err"; }
run base A=1
run r2min128 YNET_CONV_R2_MIN=128
run r2min256 YNET_CONV_R2_MIN=256
run r4min512 YNET_CONV_R4_MIN=512
