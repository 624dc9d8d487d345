set -eo pipefail
# usage: tools/rehearse_gloo.sh [output directory]
out=${1:-rehearse_out}
mkdir -p "$out"
export INFERD_DIST_BACKEND=gloo
for n in 2 4; do
  timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus $n --steps 4 --warmup 1 --no-cpu-baseline --no-profile > "$out/rehearse_n$n.log" 2>&1
done
timeout -k 10 600 python bench.py --full > "$out/bench_n1_b.log" 2>&1
