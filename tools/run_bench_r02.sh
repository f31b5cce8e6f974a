TAG=${TAG:-r02c}   # the round's tag: results under ${OUT:-results}/${TAG}_bench, to be copied into profiles/$TAG
# the bench lines kept under profiles/${TAG} (run on the GPU box)
D=${OUT:-results}/${TAG}_bench
mkdir -p $D
python bench.py --full --steps 20 --warmup 5 > $D/bench_ped10.json 2> $D/bench_ped10.err
for w in ped5 ped15 trio quad; do python bench.py --full --workload $w --steps 10 --warmup 3 --no-cpu-baseline > $D/bench_$w.json 2>/dev/null; done
python bench.py --full --gpus 2 --share-gpu --steps 5 --warmup 2 --sites 2000000 --no-cpu-baseline > $D/bench_2ranks_shared_gpu_weak.json 2>/dev/null
python bench.py --full --gpus 2 --share-gpu --steps 5 --warmup 2 --scaling strong --no-cpu-baseline > $D/bench_2ranks_shared_gpu_strong.json 2>/dev/null
python tools/cli_throughput.py 3000000 --packed > $D/cli_packed_3M.txt 2>&1
python tools/cli_throughput.py 12000000 --packed > $D/cli_packed_12M.txt 2>&1
tail -5 $D/cli_packed_12M.txt
python tools/host_path_rate.py > $D/host_path_rate.txt 2>&1; tail -6 $D/host_path_rate.txt
ls -la $D
