#!/bin/bash
# SURVEY 8(e) on a 1-GPU box: bench.py with 2 gloo ranks sharing the GPU (exchange staged through host memory) must print the SAME
# per-frame detection digests as the 1-rank run: real frames are routed through the frame ring, not i.i.d. per rank.
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}; OUT=$ROOT/gpurun_out/multirank; mkdir -p $OUT; cd $ROOT
timeout 300 python bench.py --full --steps 16 --warmup 4 --no-cpu-baseline --no-numerics --no-side-modes --no-from-points --no-latency --no-size-sweep > $OUT/n1.json 2> $OUT/n1.err
# round 5: the ranks are started by bench.py ITSELF (`python bench.py --gpus R`, no launcher) and every lane replays two HIP graphs per frame around its exchange
for R in ${RING_RANKS:-2 4}; do
COALIGN_BENCH_BACKEND=gloo COALIGN_BENCH_ONE_GPU=1 timeout 600 python bench.py --full --gpus $R --steps 8 --warmup 2 --no-cpu-baseline --no-numerics --no-side-modes --no-size-sweep > $OUT/n$R.json 2> $OUT/n$R.err
done
# north_star's wording: ONE frame, agents split over the ranks, all-gather, ego tail (bench.py --mode gather); 2 and 5 ranks (5 = one agent per rank)
# (6 ranks for 5 agents: one rank encodes an EMPTY agent block -- the sparse canvas of a frame without pillars)
for R in ${GATHER_RANKS:-2 5 6}; do
COALIGN_BENCH_BACKEND=gloo COALIGN_BENCH_ONE_GPU=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node $R --master-addr 127.0.0.1 --master-port $((29670 + R)) \
    bench.py --full --gpus $R --mode gather --steps 8 --warmup 2 --no-cpu-baseline --no-numerics --no-side-modes --no-size-sweep > $OUT/g$R.json 2> $OUT/g$R.err
done
# the fall-back chain with injected failures (raised on EVERY rank before the schedule's first collective: with host-blocking gloo collectives a failure on
# one rank only would leave its peer inside the collective until the process-group timeout): ring fails -> gather; ring and gather fail -> independent replicas
COALIGN_BENCH_INJECT_FAIL="ring:0,ring:1" COALIGN_BENCH_BACKEND=gloo COALIGN_BENCH_ONE_GPU=1 timeout 150 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29691 \
    bench.py --full --gpus 2 --steps 8 --warmup 2 --no-cpu-baseline --no-numerics --no-side-modes --no-size-sweep > $OUT/f1.json 2> $OUT/f1.err
[ -n "${SKIP_F2:-}" ] || COALIGN_BENCH_INJECT_FAIL="ring:0,ring:1,gather:0,gather:1" COALIGN_BENCH_BACKEND=gloo COALIGN_BENCH_ONE_GPU=1 timeout 150 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29692 \
    bench.py --full --gpus 2 --steps 8 --warmup 2 --no-cpu-baseline --no-numerics --no-side-modes --no-size-sweep > $OUT/f2.json 2> $OUT/f2.err
python - $OUT <<'PY'
import json,sys
out=sys.argv[1]
ref=json.loads([l for l in open(out+"/n1.json") if l.startswith("{")][-1])
print("N=1 ", ref["value"], "frames/s, digests reproducible:", ref["frame_digests_reproducible"])
ok=True
import os
for R in [int(v) for v in os.environ.get("RING_RANKS", "2 4").split()]:
    try:
        d=json.loads([l for l in open(f"{out}/n{R}.json") if l.startswith("{")][-1])
    except Exception as e:
        print(f"N={R}: no result ({e})"); ok=False; continue
    same=all(ref["frame_digests"].get(k)==v for k,v in d["frame_digests"].items())
    print(f"N={R} (self-launched, gloo, one GPU shared; functional only): {d['value']} frames/s, n_gpus {d['n_gpus']}, hip_graph {d['config']['hip_graph']}, parallelism = {d['config']['parallelism']}, "
          f"bytes sent per rank and step = {d.get('exchange_bytes_sent_per_rank_per_step')}, {len(d['frame_digests'])} pool frames, digests equal to N=1: {same}, reproducible: {d['frame_digests_reproducible']}")
    r=d.get("rccl") or {}
    print(f"      rccl key: world {r.get('world')}, backend {r.get('backend')}, ranks seen {[(x['rank'], x['local_rank']) for x in r.get('ranks_seen', [])]}, mode run {r.get('mode_run')}, "
          f"fallbacks {r.get('fallbacks')}, exchange {r.get('exchange_ms_per_frame')} ms, {r.get('bytes_sent_per_rank_per_exchange')} B sent per rank, {r.get('bytes_per_agent_fp32')} B per agent")
    ok = ok and same
for R in [int(v) for v in os.environ.get("GATHER_RANKS", "2 5 6").split()]:
    try:
        d=json.loads([l for l in open(f"{out}/g{R}.json") if l.startswith("{")][-1])
    except Exception as e:
        print(f"gather N={R}: no result ({e})"); ok=False; continue
    same=all(ref["frame_digests"].get(k)==v for k,v in d["frame_digests"].items())
    print(f"gather N={R} (gloo, one GPU shared; functional only): {d['value']} frames/s ({d['scaling']}), hip_graph {d['config']['hip_graph']}, fallbacks {(d.get('rccl') or {}).get('fallbacks')}, parallelism = {d['config']['parallelism']}, "
          f"{len(d['frame_digests'])} pool frames, digests equal to N=1: {same}")
    ok = ok and same
for name, want in ((("f1", "gather"),) if os.environ.get("SKIP_F2") else (("f1", "gather"), ("f2", "replicas"))):
    try:
        d=json.loads([l for l in open(f"{out}/{name}.json") if l.startswith("{")][-1])
    except Exception as e:
        print(f"fall-back run {name}: no result ({e})"); ok=False; continue
    r=d.get("rccl") or {}
    same=all(ref["frame_digests"].get(k)==v for k,v in d["frame_digests"].items())
    print(f"injected failure -> requested {r.get('requested_mode')}, ran {r.get('mode_run')} (expected {want}), fall-backs {r.get('fallbacks')}, {d['value']} frames/s, digests equal to N=1: {same}")
    ok = ok and r.get("mode_run") == want and same
print("N=1 digests:", ref["frame_digests"])
print("MULTIRANK_CHECK", "PASS" if ok else "FAIL")
PY
