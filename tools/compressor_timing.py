"""NaiveCompressor(64, r).forward at canvas resolution: the SplitMap route against the library route and against the all-64-channel SplitMap route.

    python tools/compressor_timing.py [--n 5] [--h 200] [--w 704] [--iters 50] [--rounds 5] [--out profiles/compressor/timing.json]

Routes, interleaved round by round in one process (boxes differ by several percent, a process does not):
  new      the module's forward as it stands: encoder on coalign_conv3x3_sp_narrow (channels-last canvas split in the loader), decoder on coalign_conv3x3_sp
  new2     the same call again (the run-to-run spread of one build)
  library  the forward of before: three F.conv2d (MIOpen, native fp32) + coalign_bias_act, NCHW
  wide64   everything zero-padded to 64 channels on the existing kernels: coalign_conv3x3_emu_ex (terms 16, SplitMap out) + two coalign_conv3x3_sp
  narrow   the narrow layer alone, channels-last input; narrow_sp: the same layer on a SplitMap input
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--h", type=int, default=200)
    ap.add_argument("--w", type=int, default=704)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ratios", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compressor_timing needs the GPU: a timing from anywhere else says nothing")
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
