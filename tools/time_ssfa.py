"""Time the SSFA neck of the SECOND detectors at the OPV2V shape [5, 128, 100, 352]: neck + shrink header + heads with ``COALIGN_SSFA`` off (the torch route: what the
model did before the kernel route existed, and the yardstick) against on, and the two new kernels against their library counterparts -- the transposed convolutions
against ``F.conv_transpose2d`` and against ``ops.conv3x3_sp`` on the zero-stuffed map, the blend against its torch expression.  Everything is warmed up at its
shape; device events; alternating rounds (as tools/time_sparse3d.py); median and min .. max.  Also the kernel route's launches and the two routes' distance.
``--numerics`` writes the error tables of both routes against the float64 forward (tests/ssfa_reference.py) instead.

    python tools/time_ssfa.py [--out profiles/ssfa/timing.json] [--agents 5]
    python tools/time_ssfa.py --numerics [--out profiles/ssfa/numerics.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from coalign_amd import backbone, ops, second  # noqa: E402
from coalign_amd.config import builtin_config  # noqa: E402
from coalign_amd.detector import build_model  # noqa: E402
from coalign_amd.synthetic import fill_parameters_  # noqa: E402

DEV = torch.device("cuda:0")


def bev_map(agents, H, W, seed=0, fill=0.35):
    """A to-dense map as the trunk leaves it: channels-last float32, non-negative (the trunk ends in a ReLU), most cells empty."""
    g = torch.Generator().manual_seed(seed)
    occ = (torch.rand((agents, H, W, 1), generator=g) < fill).float()
    return (torch.relu(torch.randn((agents, H, W, 128), generator=g)) * occ).to(DEV).permute(0, 3, 1, 2)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": [float(x) for x in v]}


def alternate(fns: dict, rounds: int, reps: int) -> dict:
    """{name: stats} of callables timed in alternating rounds; every callable is warmed up first and its first call of a round is not timed."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            f()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / reps)
    return {k: stats(v) for k, v in times.items()}


def model_of(name, seed=1):
    model = build_model(builtin_config("second/" + name))
    fill_parameters_(model.ssfa, seed=seed)
    return model.eval().to(DEV)


def run(model, bev, switch):
    model.ssfa.neck_kernels = switch
    model.bev_features = lambda data_dict: bev
    with torch.no_grad():
        return model({})


def worst(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def timing(a):
    out = {"shape": [a.agents, 128, a.H, a.W], "method": f"device events, {a.rounds} alternating rounds x {a.reps} calls, everything warmed up at its shape",
           "switch": "COALIGN_SSFA: off = the torch route (the parent commit's behaviour), on = the kernel route"}
    bev = bev_map(a.agents, a.H, a.W)
    for name in ("opv2v_second_uncertainty", "opv2v_second"):
        model = model_of(name)
        off, on = run(model, bev, False), run(model, bev, True)
        ops.PROFILE = {}
        run(model, bev, True)
        torch.cuda.synchronize()
        calls = {k: len(v) for k, v in ops.PROFILE.items()}
        ops.PROFILE = None
        t = alternate({"switch_off": lambda: run(model, bev, False), "switch_on": lambda: run(model, bev, True)}, a.rounds, a.reps)
        out[name] = {"neck_shrink_heads": t, "speedup_median": t["switch_off"]["median_ms"] / t["switch_on"]["median_ms"], "kernel_route_calls": calls,
                     "kernel_route_launches": sum(calls.values()) + 1,      # + SplitMap.pack of the to-dense map
                     "on_vs_off_worst_of_scale": {k: worst(on[k], off[k]) for k in on if on[k].dim() == 4}}
        del model
    # ---- per kernel: the two transposed convolutions of the neck (256 -> 128 at half resolution), with and without the residual
    g = torch.Generator(device=DEV).manual_seed(3)
    N, h, w = a.agents, a.H // 2, a.W // 2
    x = torch.relu(torch.randn((N, h, w, 256), generator=g, device=DEV)).permute(0, 3, 1, 2)
    wt = torch.randn((256, 128, 3, 3), generator=g, device=DEV) * (1.0 / (256 * 2.25)) ** 0.5
    b = torch.randn(128, generator=g, device=DEV) * 0.1
    r = torch.relu(torch.randn((N, 2 * h, 2 * w, 128), generator=g, device=DEV)).permute(0, 3, 1, 2)
    xs = ops.SplitMap.pack(x)
    image = ops.pack_conv3x3_emu_weight(wt.permute(1, 0, 2, 3).contiguous(), 16, True)
    flipped = ops.pack_conv3x3_emu_weight(wt.permute(1, 0, 2, 3).flip(2, 3).contiguous(), 16, True)
    z = torch.zeros((N, 2 * h, 2 * w, 256), device=DEV).permute(0, 3, 1, 2)
    z[:, :, ::2, ::2] = xs.dense()
    zs = ops.SplitMap.pack(z)
    xc = x.contiguous()                                            # the torch route's layout
    rc = r.contiguous()
    with torch.no_grad():
        kern = {"deconv3x3_s2_sp": lambda: ops.deconv3x3_s2_sp(xs, image, b, 128), "deconv3x3_s2_sp + residual": lambda: ops.deconv3x3_s2_sp(xs, image, b, 128, residual=r),
                "conv3x3_sp on the zero-stuffed map (map given)": lambda: ops.conv3x3_sp(zs, flipped, b, 128, None, True, out_split=True),
                "F.conv_transpose2d + bias + relu": lambda: torch.relu(F.conv_transpose2d(xc, wt, b, stride=2, padding=1, output_padding=1)),
                "F.conv_transpose2d + bias + relu + residual": lambda: torch.relu(F.conv_transpose2d(xc, wt, b, stride=2, padding=1, output_padding=1)) + rc}
        out["deconv_256_to_128"] = {"shape_in": [N, 256, h, w], **alternate(kern, a.rounds, a.reps)}
        out["deconv_256_to_128"]["kernel_vs_library_worst_of_scale"] = worst(kern["deconv3x3_s2_sp"]().dense(), kern["F.conv_transpose2d + bias + relu"]())
        out["deconv_256_to_128"]["equals_zero_stuffed_conv3x3_sp"] = bool(torch.equal(ops.deconv3x3_s2_sp(xs, image, b, 128).data, ops.conv3x3_sp(zs, flipped, b, 128, None, True, out_split=True, geometry=100000).data))
        # ---- the blend
        A = torch.relu(torch.randn((N, a.H, a.W, 128), generator=g, device=DEV)).permute(0, 3, 1, 2)
        B = torch.relu(torch.randn((N, a.H, a.W, 128), generator=g, device=DEV)).permute(0, 3, 1, 2)
        wa, wb = torch.randn(128, generator=g, device=DEV) * 0.1, torch.randn(128, generator=g, device=DEV) * 0.1
        Ac, Bc = A.contiguous(), B.contiguous()

        def torch_blend():
            la, lb = F.conv2d(Ac, wa.view(1, 128, 1, 1)) + 0.1, F.conv2d(Bc, wb.view(1, 128, 1, 1)) - 0.1
            sm = torch.softmax(torch.cat([la, lb], dim=1), dim=1)
            return (Ac * sm[:, 0:1] + Bc * sm[:, 1:]).contiguous()
        blend = {"ssfa_blend -> float32": lambda: ops.ssfa_blend(A, B, wa, wb, 0.1, -0.1), "ssfa_blend -> SplitMap": lambda: ops.ssfa_blend(A, B, wa, wb, 0.1, -0.1, True, False),
                 "torch: 2 x conv2d + softmax + weighted sum": torch_blend}
        out["blend"] = {"shape": [N, 128, a.H, a.W], **alternate(blend, a.rounds, a.reps)}
        out["blend"]["bytes_moved_float32_out"] = 3 * N * 128 * a.H * a.W * 4
        out["blend"]["kernel_vs_torch_worst_of_scale"] = worst(blend["ssfa_blend -> float32"](), torch_blend())
    return out


def numerics(a):
    from ssfa_reference import deconv_f64, ssfa_f64
    m = second.SSFA({"feature_num": 128})
    fill_parameters_(m, seed=1)
    m = m.eval().to(DEV)
    out = {"reference": "the module's own float64 forward, every convolution tap by tap (tests/ssfa_reference.py); errors as max |diff| / max |reference|",
           "arithmetic": backbone.EMU_MODE_NAMES[backbone.CONV_EMU_TERMS]}
    for shape in ((2, 128, 16, 32), (1, 128, 100, 352)):
        x = bev_map(shape[0], shape[2], shape[3], seed=shape[2])
        ref = ssfa_f64(m, x)
        with torch.no_grad():
            m.neck_kernels = False
            off = m(x)
            m.neck_kernels = True
            on = m(x)
        d_on, d_off = (on.double() - ref).abs(), (off.double() - ref).abs()
        scale = float(ref.abs().max())
        out["SSFA " + "x".join(str(v) for v in shape)] = {
            "kernel_route_worst_of_scale": float(d_on.max()) / scale, "torch_route_worst_of_scale": float(d_off.max()) / scale,
            "kernel_route_rms_of_scale": float(d_on.pow(2).mean().sqrt()) / scale, "torch_route_rms_of_scale": float(d_off.pow(2).mean().sqrt()) / scale}
    g = torch.Generator(device=DEV).manual_seed(5)
    for (N, Ci, Co, h, w) in ((2, 256, 128, 8, 16), (1, 256, 128, 50, 176), (1, 512, 256, 4, 4)):
        xs = ops.SplitMap.pack(torch.randn((N, Ci, h, w), generator=g, device=DEV))
        wt = torch.randn((Ci, Co, 3, 3), generator=g, device=DEV) * (1.0 / (Ci * 2.25)) ** 0.5
        b = torch.randn(Co, generator=g, device=DEV) * 0.1
        ref = deconv_f64(xs.dense(), wt, b)
        got = ops.deconv3x3_s2_sp(xs, ops.pack_conv3x3_emu_weight(wt.permute(1, 0, 2, 3).contiguous(), 16, True), b, Co, relu=False).dense()
        lib = F.conv_transpose2d(xs.dense(), wt, b, stride=2, padding=1, output_padding=1)
        scale = ref.abs().amax(dim=(0, 2, 3))
        out[f"deconv {N}x{Ci}x{Co}x{h}x{w}"] = {"kernel_worst_channel_of_its_scale": float(((got.double() - ref).abs().amax(dim=(0, 2, 3)) / scale).max()),
                                                  "float32_library_worst_channel_of_its_scale": float(((lib.double() - ref).abs().amax(dim=(0, 2, 3)) / scale).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--numerics", action="store_true")
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--W", type=int, default=352)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    path = a.out or os.path.join(ROOT, "profiles", "ssfa", "numerics.json" if a.numerics else "timing.json")
    result = numerics(a) if a.numerics else timing(a)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(result, open(path, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
