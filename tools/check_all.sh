# Full GPU check: parity tests + bench lines for every network (run on the GPU box).  usage: bash tools/check_all.sh [outdir]
out=${1:-$(mktemp -d)}
mkdir -p $out
timeout -k 10 800 python -m pytest tests -m gpu -x -q > $out/pytest.log 2>&1; tail -3 $out/pytest.log | cut -c1-250
show() { python -c "
import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[1].split('/')[-1], d['value'], 'utt/s', d['ms_per_step'], 'ms', d['tflops_algorithmic'], 'TF', '%.1e'%d['parity_rel_l2_max'], d.get('cpu_baseline') and d['cpu_baseline']['value']);print('   ', [(k['name'][:12],k['ms'],k['tflops']) for k in d['kernels']])" $1 || tail -5 $out/err.txt; }
python bench.py --full --network resnet_18 --batch 64 --steps 10 --cpu-seconds 6 > $out/bench_resnet.json 2>$out/err.txt; show $out/bench_resnet.json
python bench.py --full --network resnet_18 --batch 64 --steps 10 --cpu-seconds 0 --precision f32 > $out/bench_resnet_f32.json 2>$out/err.txt; show $out/bench_resnet_f32.json
python bench.py --full --network extended_tdnn --cpu-seconds 0 > $out/bench_etdnn.json 2>$out/err.txt; show $out/bench_etdnn.json
python bench.py --full --cpu-seconds 0 > $out/bench_tdnn.json 2>$out/err.txt; show $out/bench_tdnn.json
echo "results in $out"
