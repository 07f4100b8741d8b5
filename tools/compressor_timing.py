"""NaiveCompressor(64, r).forward at canvas resolution: the SplitMap route against the library route and against the all-64-channel SplitMap route.

    python tools/compressor_timing.py [--n 5] [--h 200] [--w 704] [--iters 50] [--rounds 5] [--out profiles/compressor/timing.json]

Routes, interleaved round by round in one process (boxes differ by several percent, a process does not):
  new      the module's forward as it stands: encoder on coalign_conv3x3_sp_narrow (channels-last canvas split in the loader), decoder on coalign_conv3x3_sp
  new2     the same call again (the run-to-run spread of one build)
  library  the forward of before: three F.conv2d (MIOpen, native fp32) + coalign_bias_act, NCHW
  wide64   everything zero-padded to 64 channels on the existing kernels: coalign_conv3x3_emu_ex (terms 16, SplitMap out) + two coalign_conv3x3_sp
  narrow   the narrow layer alone, channels-last input; narrow_sp: the same layer on a SplitMap input
With --sparse-out the SEGMENT pillar encoder + narrow layer is timed on the 5 x 8000-pillar OPV2V frame, again interleaved in one process:
  dense_segment    the route of before: the dense-route pillar op (persistent channels-last canvas, two launches) + the narrow layer on its channels-last loader
  sparse_segment   pillar_encode_sparse (one launch) + sp_pack_rows + the narrow layer gathering through the stamps (coalign_conv3x3_sp_narrow_sparse)
  sparse_segment2  the same call again
and the share of 16 x 32 output tiles whose whole 18 x 34 patch is empty is recorded (a K loop that skipped them is not built).
Times are medians over `rounds` windows of `iters` forwards between two device events.  Bytes of the narrow layer = the input map read once + the SplitMap
written (N H W (Cin + Cp) 4).  Needs the GPU; prints one JSON document and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import backbone as bb  # noqa: E402
from coalign_amd import ops  # noqa: E402
from coalign_amd.synthetic import fill_parameters_  # noqa: E402

DEV = "cuda:0"


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters          # microseconds per call


def sparse_segment(a):
    """Pillar encoder + narrow layer, dense canvas against sparse canvas, on the bench frame (opv2v_coalign, 5 agents x 8000 pillars)."""
    from coalign_amd.config import builtin_config
    from coalign_amd.detector import build_model
    from coalign_amd.synthetic import make_frame
    h = builtin_config("opv2v_coalign")
    margs = h["model"]["args"]
    model = build_model(h)
    fill_parameters_(model, seed=0)
    pfn = model.to(DEV).eval().pillar_vfe.pfn_layers[0]
    bn = (pfn.norm.weight, pfn.norm.bias, pfn.norm.running_mean, pfn.norm.running_var)
    gx, gy, _ = [int(v) for v in margs["point_pillar_scatter"]["grid_size"]]
    n_agents, pillars = 5, 8000
    pl = make_frame(h, n_agents, pillars_per_agent=pillars, seed=303)["processed_lidar"]
    vf, npts, coords = pl["voxel_features"].to(DEV), pl["voxel_num_points"].to(DEV).to(torch.int32), pl["voxel_coords"].to(DEV).to(torch.int32)
    folded_p = ops.pillar_fold_params(pfn.linear.weight, None, bn, 1e-3, True)
    dense_cache, sparse_cache = {}, {}
    vs, r0 = margs["voxel_size"], margs["lidar_range"][:3]

    def pillar_dense():
        return ops.pillar_vfe_scatter(vf, npts, coords, pfn.linear.weight, None, bn, 1e-3, True, False, vs, r0, n_agents, gy, gx, channels_last=True, canvas_cache=dense_cache)[1]

    def pillar_sparse():
        return ops.pillar_encode_sparse(vf, npts, coords, pfn.linear.weight, None, bn, 1e-3, True, vs, r0, n_agents, gy, gx, canvas_cache=sparse_cache, folded=folded_p)

    with torch.no_grad():
        occ = (pillar_sparse().dense().abs().amax(dim=1) > 0).float()[:, None]              # [N, 1, H, W]
        th, tw = 16, 32
        hp, wp = (gy + th - 1) // th * th, (gx + tw - 1) // tw * tw
        halo = F.max_pool2d(F.pad(occ, (0, wp - gx, 0, hp - gy)), 3, 1, 1)                    # a pixel's 3 x 3 neighbourhood holds a pillar
        tiles = F.max_pool2d(halo, (th, tw))
        result = {"frame": {"agents": n_agents, "pillars_per_agent": pillars, "grid": [gy, gx], "occupied_cells_share": round(float(occ.mean()), 4),
                            "tiles": int(tiles.numel()), "tiles_with_an_all_empty_patch_share": round(1.0 - float(tiles.mean()), 4)},
                  "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "ratios": {}}
        for r in a.ratios:
            m = bb.NaiveCompressor(64, r)
            fill_parameters_(m, seed=60 + r)
            m = m.to(DEV).eval()
            kind, cp, enc, be = m._split_images()[:4]
            if kind != "narrow":
                continue

            def dense_segment():
                return ops.conv3x3_sp_narrow(pillar_dense(), enc, be, cp, True)

            def sparse_segment():
                return ops.conv3x3_sp_narrow(pillar_sparse(), enc, be, cp, True)

            def narrow_dense(canvas=pillar_dense()):
                return ops.conv3x3_sp_narrow(canvas, enc, be, cp, True)

            routes = {"dense_segment": dense_segment, "sparse_segment": sparse_segment, "sparse_segment2": sparse_segment, "pillar_dense": pillar_dense,
                      "pillar_sparse": pillar_sparse, "narrow_dense_alone": narrow_dense}
            outs = {k: fn() for k, fn in routes.items()}
            for fn in routes.values():
                window(fn, 3)
            diff = float((outs["sparse_segment"].dense() - outs["dense_segment"].dense()).abs().max()) / float(outs["dense_segment"].dense().abs().max())
            times = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    times[k].append(window(fn, a.iters))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = abs(med["sparse_segment2"] / med["sparse_segment"] - 1.0)
            result["ratios"][str(r)] = {"padded_mid": cp, "median_us": {k: round(v, 2) for k, v in med.items()},
                                        "min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
                                        "sparse_over_dense": round(med["sparse_segment"] / med["dense_segment"], 4), "same_call_twice_spread": round(spread, 4),
                                        "faster_by_more_than_the_spread": bool(med["sparse_segment"] < med["dense_segment"] * (1.0 - spread)
                                                                               and med["sparse_segment2"] < med["dense_segment"] * (1.0 - spread)),
                                        "max_abs_diff_of_the_mid_maps_over_scale": diff}
            del m, outs
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--h", type=int, default=200)
    ap.add_argument("--w", type=int, default=704)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ratios", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--out", default="")
    ap.add_argument("--sparse-out", default="", help="time the pillar encoder + narrow layer segment, dense canvas against sparse canvas, and write it here")
    ap.add_argument("--sparse-only", action="store_true", help="skip the forward timings")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compressor_timing needs the GPU: a timing from anywhere else says nothing")
    if a.sparse_out:
        text = json.dumps(sparse_segment(a), indent=1)
        print(text)
        os.makedirs(os.path.dirname(os.path.abspath(a.sparse_out)), exist_ok=True)
        open(a.sparse_out, "w").write(text + "\n")
        if a.sparse_only:
            return
    g = torch.Generator(device=DEV).manual_seed(1)
    x_cl = torch.randn((a.n, 64, a.h, a.w), generator=g, device=DEV).relu_().contiguous(memory_format=torch.channels_last)
    x_nchw = x_cl.contiguous()
    result = {"shape": [a.n, 64, a.h, a.w], "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "ratios": {}}
    for r in a.ratios:
        m = bb.NaiveCompressor(64, r)
        fill_parameters_(m, seed=60 + r)
        m = m.to(DEV).eval()
        kind, cp = m.split_widths()
        folded = [bb.fold_bn(q[0].weight, q[0].bias, q[1]) for q in (m.encoder, m.decoder[0:3], m.decoder[3:6])]
        mid = folded[0][0].shape[0]
        we64, be64, w164 = torch.zeros((64, 64, 3, 3), device=DEV), torch.zeros(64, device=DEV), torch.zeros((64, 64, 3, 3), device=DEV)
        with torch.no_grad():
            we64[:mid], be64[:mid], w164[:, :mid] = folded[0][0], folded[0][1], folded[1][0]
            imgs64 = [ops.pack_conv3x3_emu_weight(w, 16, True) for w in (we64, w164, folded[2][0])]
            b64 = [be64, folded[1][1].detach(), folded[2][1].detach()]
            _, _, enc, be, _, _, _, _ = m._split_images()

        def new():
            return m(x_cl)

        def library():
            y = x_nchw
            for w, b in folded:
                y = ops.bias_act_(F.conv2d(y, w, None, 1, 1), b, None, True)
            return y

        def wide64():
            y = ops.conv3x3_emu_bias_act(x_nchw, imgs64[0], b64[0], 64, None, True, 16, out_split=True)
            y = ops.conv3x3_sp(y, imgs64[1], b64[1], 64, None, True, out_split=True)
            return ops.conv3x3_sp(y, imgs64[2], b64[2], 64, None, True, out_split=False)

        xs = ops.SplitMap.pack(x_cl)

        def narrow():
            return ops.conv3x3_sp_narrow(x_cl, enc, be, cp, True)

        def narrow_sp():
            return ops.conv3x3_sp_narrow(xs, enc, be, cp, True)

        routes = {"new": new, "library": library, "wide64": wide64, "new2": new, "narrow": narrow, "narrow_sp": narrow_sp}
        if kind != "narrow":
            routes.pop("narrow"), routes.pop("narrow_sp")
        with torch.no_grad():
            outs = {k: fn() for k, fn in routes.items()}                      # warm-up of every shape (code objects, MIOpen's choice, weight images)
            for k, fn in routes.items():
                window(fn, 3)
            ref = outs["library"]
            scale = float(ref.abs().max())
            agree = {k: float((outs[k] - ref).abs().max()) / scale for k in ("new", "wide64")}
            times = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    times[k].append(window(fn, a.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        entry = {"mid": mid, "padded_mid": cp, "median_us": {k: round(v, 2) for k, v in med.items()},
                 "min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
                 "max_abs_diff_to_library_over_scale": agree,
                 "speedup_vs_library": round(med["library"] / med["new"], 3), "speedup_vs_wide64": round(med["wide64"] / med["new"], 3),
                 "same_build_twice": round(med["new2"] / med["new"], 4)}
        if kind == "narrow":
            nbytes = a.n * a.h * a.w * (64 + cp) * 4
            entry["narrow_layer"] = {"bytes_read_plus_written": nbytes, "GBps_channels_last_in": round(nbytes / med["narrow"] / 1e3, 1),
                                     "GBps_split_map_in": round(nbytes / med["narrow_sp"] / 1e3, 1),
                                     "executed_fp16_products_G": round(3 * 9 * 64 * 32 * a.n * a.h * a.w / 1e9, 2)}
        result["ratios"][str(r)] = entry
        del m, outs
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
