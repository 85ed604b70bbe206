python bench.py --workload frame --steps 50 --warmup 10 --blocks 4 --full --no-cpu-baseline --no-other-workloads --no-end-to-end --no-live-traffic
