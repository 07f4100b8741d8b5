"""Time Where2comm's messages at the OPV2V shapes (5 agents x {64 @ 100 x 352, 128 @ 50 x 176, 256 @ 25 x 88}): ``ops.w2comm_msg_index`` and
``ops.w2comm_msg_pack`` of the four non-ego agents, and ``ops.w2comm_fuse_packed`` (ego dense, the others packed) next to ``ops.w2comm_fuse_nhwc`` on the same maps,
masks and theta; and the messages' bytes against the dense maps'.  Mask sets: what ``ops.w2comm_masks`` gives for synthetic logits at the mini config's threshold
and 5 x 5 smoothing (agents 2 and 4 all ones: the even-agent rule), and uniform random masks of density 0.01, 0.1 and 0.5 on every agent at level 0, pooled 2 x 2
for the levels above as the module pools them.

Protocol (that of tools/time_where2comm.py): all versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device
events around ``--reps`` eager calls and around one replay of a graph that captured the same ``--reps`` calls.  Per version: the median over the rounds and their
spread, per call.  The eager figure includes the host's work between launches (allocations, ctypes); the replay figure is the kernels back to back with the
graph's own launch gaps.  Before timing, the packed fusion is compared with the dense one (``torch.equal``).

    python tools/time_where2comm_msg.py [--agents 5] [--reps 50] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coalign_amd import ops  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.fusion import Where2commFusion  # noqa: E402
from time_v2v_fusion import poses  # noqa: E402

LEVELS = ((64, 100, 352), (128, 50, 176), (256, 25, 88))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_where2comm_msg.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    n = a.agents
    g = torch.Generator().manual_seed(1)
    xs = [torch.relu(torch.randn(n, C, H, W, generator=g)).to(dev).contiguous(memory_format=torch.channels_last) for C, H, W in LEVELS]      # post-ReLU maps
    psm = (2 * torch.randn(n, 2, LEVELS[0][1], LEVELS[0][2], generator=g) - 2).to(dev)
    theta = poses(n, LEVELS[0][1], LEVELS[0][2])[None].to(dev)[0, 0, :n].contiguous()
    w2c = builtin_config("mini_pointpillar_where2comm")["model"]["args"]["where2comm"]
    m = Where2commFusion(dict(w2c, layer_nums=[1, 1, 1], num_filters=[64, 128, 256])).eval().to(dev)
    comm = m.naive_communication
    mask_sets = {"w2comm_masks at the mini config's threshold": ops.w2comm_masks(psm, [n], comm.gaussian_filter.weight.detach(), comm.gaussian_filter.bias.detach(), comm.thre, levels=3)[0]}
    for density in (0.01, 0.1, 0.5):
        m0 = (torch.rand(n, 1, LEVELS[0][1], LEVELS[0][2], generator=g) < density).float().to(dev)
        m1 = F.max_pool2d(m0, kernel_size=2)
        mask_sets[f"density {density}"] = [k[:, 0].to(torch.uint8).contiguous() for k in (m0, m1, F.max_pool2d(m1, kernel_size=2))]
    dense_bytes = sum(C * H * W * 4 for C, H, W in LEVELS)
    result = {"agents": n, "levels": LEVELS, "reps": a.reps, "rounds": a.rounds, "dense_bytes_per_agent": dense_bytes, "thre": comm.thre, "sets": {}}
    for name, masks in mask_sets.items():
        ego_x, ego_m = [x[:1] for x in xs], [k[:1] for k in masks]
        send_x, send_m = [x[1:] for x in xs], [k[1:] for k in masks]
        bits, rank, _ = ops.w2comm_msg_index(send_m)
        sent = m.pack_messages(send_x, send_m)
        versions = {"w2comm_msg_index": lambda: ops.w2comm_msg_index(send_m),
                    "w2comm_msg_pack": lambda: ops.w2comm_msg_pack(send_x, bits, rank),
                    "w2comm_fuse_packed": lambda: m.fuse_messages(ego_x, ego_m, sent, theta, ops.FUSE_ATT),
                    "w2comm_fuse_nhwc": lambda: ops.w2comm_fuse_nhwc(xs, masks, theta, ops.FUSE_ATT)}
        entry = {"mask_fractions_on": [float(k.float().mean()) for k in masks], "message_bytes": [msg.nbytes for msg in sent],
                 "packed equals dense (torch.equal)": all(torch.equal(p, q) for p, q in zip(versions["w2comm_fuse_packed"](), versions["w2comm_fuse_nhwc"]()))}
        entry["message_bytes_of_dense"] = [b / dense_bytes for b in entry["message_bytes"]]
        for fn in versions.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        graphs = {}
        for v, fn in versions.items():          # the same --reps calls captured once: a replay has the kernels back to back, without the host's work between them
            graphs[v] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[v]):
                for _ in range(a.reps):
                    fn()
            graphs[v].replay()
        torch.cuda.synchronize()
        eager, replay = {k: [] for k in versions}, {k: [] for k in versions}
        for _ in range(a.rounds):
            for v, fn in versions.items():
                t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                t0.record()
                for _ in range(a.reps):
                    fn()
                t1.record()
                graphs[v].replay()
                t2.record()
                t2.synchronize()
                eager[v].append(t0.elapsed_time(t1) / a.reps)
                replay[v].append(t1.elapsed_time(t2) / a.reps)
        for v in versions:
            e, r = sorted(eager[v]), sorted(replay[v])
            entry[v] = {"graph_replay_median_us": 1e3 * r[len(r) // 2], "graph_replay_min_us": 1e3 * r[0], "graph_replay_max_us": 1e3 * r[-1],
                        "eager_call_median_us": 1e3 * e[len(e) // 2], "eager_call_min_us": 1e3 * e[0], "eager_call_max_us": 1e3 * e[-1]}
        del graphs
        result["sets"][name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
