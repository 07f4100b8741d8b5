"""Time V2X-ViT's fusion at the OPV2V shape (5 agents x 256 x 48 x 176, depth 3, split attention): the kernel route (``V2XViTFusion.forward``: the agent attention
of every layer on ``ops.v2x_agent_attention``, the other blocks torch ops) against the module's own op-by-op PyTorch route (``forward_torch``: all L padded agents,
every layer for every agent) and against ``forward_reduced`` (the identities in PyTorch ops) on the same device and inputs.  Kernel route vs ``forward_torch`` is
the comparison of record; ``forward_reduced`` separates what the identities buy from what the kernel buys.  A fourth route is the kernel route with
``window_kernels`` set: the pyramid window attention with its split attention on ``ops.v2x_window_attention`` (off by default in the module); a fifth adds
``ffn_kernels``: the feed-forward block on ``ops.v2x_feed_forward`` (off by default too), every block of an encoder layer then hand-written.

Protocol: the five versions in ONE process; warm-up of each; then ``--rounds`` rounds, interleaving the versions, a round being device events around ``--reps``
calls.  Per version: the median over the rounds and their spread (min .. max).  Before timing, the outputs are compared element-wise at the timed size.
The split per block re-executes each block of each route's schedule on its own, on tensors of the shape that route hands it (event pairs around ``--reps`` calls,
the same rounds): agent attention, window attention (the pyramid with its split attention), feed-forward, summed over the layers.  The warp, the STTF resample and the
glue between the blocks are in the whole-fusion time only.  For the kernel: the share of the fp16 matrix peak (2.5 PFLOP/s dense) of the products its two
projections execute (three fp16 products per fp32 product); the same for the window kernel's four projections and the feed-forward kernel's two.  The feed-forward
is also timed on its own with the torch ops and the kernel INTERLEAVED round by round on the same tokens (``feed_forward_per_layer``): the kernel counts as faster
when its median is below the torch ops' fastest round.  ``--route-only`` runs nothing but the kernel route (``--window-kernels`` / ``--ffn-kernels``: with those
kernels): the program to put behind a kernel trace.

    python tools/time_v2xvit_fusion.py [--agents 5] [--hw 48 176] [--config opv2v_pointpillar_v2xvit] [--reps 3] [--rounds 7] [--route-only [--window-kernels] [--ffn-kernels]] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.fusion import V2XViTFusion  # noqa: E402
from coalign_amd.synthetic import v2xvit_parameters_  # noqa: E402
from coalign_amd.v2xvit import agent_attention_reduced  # noqa: E402

FP16_MATRIX_PEAK = 2.5e15
ROUTES = ("kernel route", "forward_torch (op by op)", "forward_reduced (identities, PyTorch ops)", "kernel route + window kernels", "kernel route + window + feed-forward kernels")


def poses(n, H, W, L, seed=0):
    """Row 0 of the affine matrix: every sender turned by up to 30 degrees and shifted by up to a quarter of the map."""
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(1, L, L, 2, 3, dtype=torch.float64)
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    for j in range(1, n):
        yaw = math.radians(float(torch.rand(1, generator=g)) * 60.0 - 30.0)
        c, s = math.cos(yaw), math.sin(yaw)
        tx, ty = (torch.rand(2, generator=g) - 0.5).tolist()
        A[0, 0, j] = torch.tensor([[c, -s * H / W, tx], [s * W / H, c, ty]], dtype=torch.float64)
    return A


def timed(fn, reps, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) / reps)
    return sorted(ts)


def stats(ts):
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=[48, 176])
    ap.add_argument("--config", default="opv2v_pointpillar_v2xvit")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--route-only", action="store_true", help="run the kernel route alone, --reps times after one warm call, and print nothing else: the program a kernel trace wraps")
    ap.add_argument("--window-kernels", action="store_true", help="with --route-only: the kernel route with the window kernels")
    ap.add_argument("--ffn-kernels", action="store_true", help="with --route-only: the kernel route with the feed-forward kernel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_v2xvit_fusion.py measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    hypes = builtin_config(a.config)
    L = int(hypes["train_params"]["max_cav"])
    n, (H, W) = a.agents, a.hw
    m = V2XViTFusion(hypes["model"]["args"]["v2xvit"])
    v2xvit_parameters_(m, seed=1)
    m = m.eval().to(dev)
    enc = m.fusion_net.encoder
    C = enc.prior_feed.out_features
    x = torch.relu(torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(2))).to(dev).contiguous(memory_format=torch.channels_last)      # post-ReLU maps, like the shrink header's
    A = poses(n, H, W, max(L, n)).to(dev)
    if not m.kernel_route(C, n, (H, W)):
        raise SystemExit("the kernel route does not take this shape")

    def run(fn):
        with torch.no_grad():
            return fn(x, [n], A)
    def run_windows():
        m.window_kernels = True
        try:
            return run(m.forward)
        finally:
            m.window_kernels = False
    def run_windows_ffn():
        m.window_kernels = m.ffn_kernels = True
        try:
            return run(m.forward)
        finally:
            m.window_kernels = m.ffn_kernels = False
    m.window_kernels = m.ffn_kernels = True
    reason = m.window_kernel_reason(C, (H, W))
    ffn_reason = m.ffn_kernel_reason(C)
    m.window_kernels = m.ffn_kernels = False
    if reason is not None:
        raise SystemExit("the window kernels do not take this shape: " + reason)
    if ffn_reason is not None:
        raise SystemExit("the feed-forward kernel does not take this shape: " + ffn_reason)
    if a.route_only:
        m.window_kernels, m.ffn_kernels = a.window_kernels, a.ffn_kernels
        for _ in range(1 + a.reps):
            run(m.forward)
        torch.cuda.synchronize()
        return
    versions = dict(zip(ROUTES, (lambda: run(m.forward), lambda: run(m.forward_torch), lambda: run(m.forward_reduced), run_windows, run_windows_ffn)))
    outs = {k: fn() for k, fn in versions.items()}
    torch.cuda.synchronize()
    want = outs[ROUTES[1]]
    scale = float(want.abs().max())
    result = {"shape": [n, C, H, W], "padded_to": max(L, n), "depth": len(enc.layers), "reps": a.reps, "rounds": a.rounds,
              "sttf_is_identity_at_this_shape": enc.sttf.positions(H, W)[1]}
    for k in (ROUTES[0], ROUTES[2], ROUTES[3], ROUTES[4]):
        err = (outs[k] - want).abs()
        result[k + ": max_err_of_scale vs forward_torch"] = float(err.max()) / scale
        result[k + ": elements_outside_1e-4+1e-5"] = int((err > 1e-4 * want.abs() + 1e-5 * scale).sum())
    del outs
    for fn in versions.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(a.rounds):
        for name, fn in versions.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.reps)
    for name, ts in times.items():
        result[name] = stats(sorted(ts))
    k_ms = result[ROUTES[0]]["median_ms"]
    result["speedup_median_vs_forward_torch"] = result[ROUTES[1]]["median_ms"] / k_ms
    result["speedup_median_vs_forward_reduced"] = result[ROUTES[2]]["median_ms"] / k_ms
    result["window_kernels: speedup_median_vs_kernel_route"] = k_ms / result[ROUTES[3]]["median_ms"]
    result["ffn_kernels: speedup_median_vs_window_kernels"] = result[ROUTES[3]]["median_ms"] / result[ROUTES[4]]["median_ms"]
    result["ffn_kernels: median_below_window_kernels_fastest_round"] = bool(result[ROUTES[4]]["median_ms"] < result[ROUTES[3]]["min_ms"])

    # ---- per block, each route's schedule re-executed block by block ----
    schedule = m._schedule(n)
    images = m.packed()
    wimages = m.packed_windows()
    fimages = {id(ff): img for ff, img in zip(m._feed_forwards(), m.packed_ffn())}
    Lp = max(L, n)
    tok = torch.randn(Lp, H, W, C, generator=torch.Generator().manual_seed(3)).to(dev)
    mask = torch.tensor([[1] * n + [0] * (Lp - n)], device=dev)[:, None, None, None, :]
    blocks = {r: {"agent attention": 0.0, "window attention": 0.0, "feed-forward": 0.0} for r in ROUTES}
    spread = {r: {} for r in ROUTES}
    kernel_ms, window_ms, ffn_layers = [], [], []
    with torch.no_grad():
        for (norm, att, R, pw, ff), img, wimg in zip(schedule, images, wimages):
            cav = next(blk[0] for layer in enc.layers for blk in layer[0].layers if blk[0].fn is att)
            per = {
                ROUTES[0]: (lambda: ops.v2x_agent_attention(tok[:n], None, img, receivers=R), R),
                ROUTES[1]: (lambda: cav(tok[None], mask=mask) + tok[None], Lp),
                ROUTES[2]: (lambda: agent_attention_reduced(tok[:n], R, norm, att, True), R),
                ROUTES[3]: (lambda: ops.v2x_agent_attention(tok[:n], None, img, receivers=R), R),
                ROUTES[4]: (lambda: ops.v2x_agent_attention(tok[:n], None, img, receivers=R), R),
            }
            for r, (fn, agents) in per.items():
                ts = timed(fn, a.reps, a.rounds)
                blocks[r]["agent attention"] += ts[len(ts) // 2]
                spread[r].setdefault("agent attention", []).append([ts[0], ts[-1]])
                if r == ROUTES[0]:
                    kernel_ms.append((R, ts[len(ts) // 2]))
                t = tok[None, :agents]
                tw = tok[:agents].contiguous()
                if r in (ROUTES[3], ROUTES[4]):
                    ts = timed(lambda: ops.v2x_window_attention(tw, wimg, pw.fn.fuse_mehod), a.reps, a.rounds)
                    if r == ROUTES[3]:
                        window_ms.append((agents, ts[len(ts) // 2]))
                else:
                    ts = timed(lambda: pw(t) + t, a.reps, a.rounds)
                blocks[r]["window attention"] += ts[len(ts) // 2]
                spread[r].setdefault("window attention", []).append([ts[0], ts[-1]])
                if ff is not None:
                    ts = timed((lambda: ops.v2x_feed_forward(tw, fimages[id(ff)])) if r == ROUTES[4] else (lambda: ff(t) + t), a.reps, a.rounds)
                    blocks[r]["feed-forward"] += ts[len(ts) // 2]
                    spread[r].setdefault("feed-forward", []).append([ts[0], ts[-1]])
            if ff is not None:
                # the feed-forward on its own, torch ops and kernel interleaved round by round on the tokens the kernel route hands it
                tw = tok[:R].contiguous()
                pair = {"torch ops": lambda: ff(tw) + tw, "kernel": lambda: ops.v2x_feed_forward(tw, fimages[id(ff)])}
                for fn in pair.values():
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                ts = {k: [] for k in pair}
                for _ in range(a.rounds):
                    for k, fn in pair.items():
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        for _ in range(a.reps):
                            fn()
                        t1.record()
                        t1.synchronize()
                        ts[k].append(t0.elapsed_time(t1) / a.reps)
                M = ff.fn.net[0].out_features
                executed = 3.0 * 2.0 * H * W * R * 2 * C * M                 # both linears, three fp16 products per fp32 product
                st = {k: stats(sorted(v)) for k, v in ts.items()}
                ffn_layers.append({"maps": R, "mlp_dim": M, "torch ops": st["torch ops"], "kernel": st["kernel"], "matrix_flop_executed": executed,
                                   "fraction_of_fp16_matrix_peak": executed / (st["kernel"]["median_ms"] * 1e-3) / FP16_MATRIX_PEAK,
                                   "kernel_median_below_torch_fastest_round": bool(st["kernel"]["median_ms"] < st["torch ops"]["min_ms"])})
    result["blocks_median_ms_summed_over_layers"] = blocks
    result["blocks_min_max_ms_per_layer"] = spread
    px = H * W
    kern = []
    for R, ms in kernel_ms:
        executed = 3.0 * 2.0 * px * C * C * (2 * n + R + R)          # k', v' of every sender, q of the receivers, the output projection of the receivers
        kern.append({"receivers": R, "ms": ms, "matrix_flop_executed": executed, "fraction_of_fp16_matrix_peak": executed / (ms * 1e-3) / FP16_MATRIX_PEAK})
    result["v2x_agent_attention_per_layer"] = kern
    win = []
    for agents, ms in window_ms:
        executed = 3.0 * 2.0 * px * agents * 12 * C * C              # the stacked 9C x C projection and the three output projections
        win.append({"maps": agents, "ms": ms, "matrix_flop_executed": executed, "fraction_of_fp16_matrix_peak": executed / (ms * 1e-3) / FP16_MATRIX_PEAK,
                    "window_products_fp32_flop": 2.0 * 2.0 * px * agents * C * (16 + 64 + 256), "workspace_bytes": int(ops.hip.lib().coalign_v2x_window_workspace_bytes(agents, C, H, W))})
    result["v2x_window_attention_per_layer"] = win
    result["feed_forward_per_layer"] = ffn_layers
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
