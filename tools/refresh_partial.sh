set -u
export OUT_ROOT=${OUT_ROOT:-prof_out}   # every output of this script goes under this folder of the repository root
R=r03
mkdir -p $OUT_ROOT/fin
python bench.py --full > $OUT_ROOT/fin/${R}_bench.json 2>$OUT_ROOT/fin/bench.err
python bench.py --full --mode train --train-dtype f32 --steps 50 --warmup 5 > $OUT_ROOT/fin/${R}_bench_train_f32.json 2>/dev/null
python bench.py --full --mode train --workload dgcnn --points 1024 --steps 10 --warmup 2 > $OUT_ROOT/fin/${R}_bench_train_dgcnn_n1024.json 2>/dev/null
python bench.py --full --mode train --workload dgcnn --batch 64 --steps 5 --warmup 1 > $OUT_ROOT/fin/${R}_bench_train_dgcnn_n4096_b64.json 2>/dev/null
python bench.py --full --mode train --workload dgcnn --batch 512 --steps 2 --warmup 1 --sustained-seconds 0 > $OUT_ROOT/fin/${R}_bench_train_dgcnn_n4096_b512.json 2>/dev/null
S="--sustained-seconds 0"
bash tools/profile.sh ${R}_train --mode train --train-dtype f32 --steps 20 --warmup 3 $S > $OUT_ROOT/fin/p_train.log 2>&1
bash tools/profile.sh ${R}_train_dgcnn --mode train --workload dgcnn --points 1024 --steps 6 --warmup 2 $S > $OUT_ROOT/fin/p_train_dgcnn.log 2>&1
mkdir -p $OUT_ROOT/profiles_${R}b
cp $OUT_ROOT/prof_${R}_train/summary/* $OUT_ROOT/prof_${R}_train_dgcnn/summary/* $OUT_ROOT/profiles_${R}b/ 2>/dev/null
cp $OUT_ROOT/fin/${R}_bench*.json $OUT_ROOT/profiles_${R}b/
for t in _train _train_dgcnn; do
  grep '^{' $OUT_ROOT/prof_${R}${t}/bench_trace.log > $OUT_ROOT/profiles_${R}b/${R}${t}_bench_under_rocprof.json 2>/dev/null
done
find $OUT_ROOT -name "*.db" -delete
ls $OUT_ROOT/profiles_${R}b
