"""The yardstick and the case table of the pillar-encoder limit tests, pinned on the CPU (no GPU needed).

``pfn_f64`` (tests/pillar_reference.py) against the references that are themselves pinned to the reference implementation: ``oracle.pillar_vfe`` on the default flags,
tests/golden/pillar_variants.npz (recorded from the reference's own ``PillarVFE``) on the four flag sets the oracle lacks; hand-computed answers for the two properties
a float64 evaluation gets wrong most easily (the centre formed in float32, the padded rows inside the max).  Then, for EVERY case of tests/pillar_cases.py, the
reference's own float32 arithmetic stays inside the bound the GPU tests hold the kernels to: no case asks of a kernel what float32 cannot do."""
import numpy as np
import pytest
import torch

from oracle import coalign_oracle as oracle
from tests import pillar_cases as pc
from tests.conftest import assert_elementwise
from tests.pillar_reference import PREFIX, cell_centres, pfn_f32, pfn_f64

T = torch.from_numpy


def _golden_variant(g, name):
    sd = {str(k): T(g[f"{name}.sd.{k}"]) for k in g[f"{name}.state_keys"]}
    use_abs, with_dist, use_norm = [bool(v) for v in g[f"{name}.flags"]]
    args = (T(g[f"{name}.voxel_features"]), T(g[f"{name}.voxel_num_points"]), T(g[f"{name}.voxel_coords"]), sd, list(g[f"{name}.voxel_size"]), list(g[f"{name}.lidar_range"]),
            use_abs, with_dist)
    return args, (use_abs, with_dist, use_norm), T(g[f"{name}.out"])


@pytest.mark.parametrize("name", ["a_M41", "a_M81", "d_P32_C64_abs", "d_P5_C33_abs", "d_P65_C128_abs", "e_opv2v_abs_M41", "e_dair_abs_M41"])
def test_pfn_f64_agrees_with_the_oracle_on_the_default_flags(name):
    case = pc.get_case(name)
    assert case.default_flags
    ref = oracle.pillar_vfe(case.vf, case.npts, case.coords, case.sd, case.voxel_size, case.lidar_range)
    assert_elementwise(ref, pc.want64(case), what=name)


@pytest.mark.parametrize("name", ["dist", "bias", "noabs", "dist_bias"])
def test_pfn_f64_and_its_float32_rerun_agree_with_the_reference_goldens(golden, name):
    """The four flag sets ``oracle.pillar_vfe`` lacks: the reference's float32 output against the float64 evaluation and against the float32 rerun that stands in for
    the oracle in the bound.  The recorded inputs are the case table's own (same generator, same seed): the table is reproducible across numpy versions."""
    g = golden("pillar_variants.npz")
    args, (use_abs, with_dist, use_norm), out = _golden_variant(g, name)
    assert int(args[1].min()) == 1 and {1, 16, 17, 32} <= set(args[1].tolist()) and out.shape == (48, 64)
    assert (PREFIX + "norm.weight" in args[3]) == use_norm and (PREFIX + "linear.bias" in args[3]) == (not use_norm)
    want = pfn_f64(*args)
    assert_elementwise(out, want, what=name + ": reference vs float64")
    rerun = pfn_f32(*args)
    assert_elementwise(rerun, out, what=name + ": float32 rerun vs reference")
    err, err_ref = pc.bound_errors(rerun, want, out)
    print(f"\n{name}: float32 rerun {err:.2e}, reference {err_ref:.2e} of the scale against float64")
    assert err <= 2e-6 and err_ref <= 2e-6
    again = pc.make_case("golden_" + name, "golden", M=48, use_abs=use_abs, with_dist=with_dist, use_norm=use_norm, counts=np.arange(48) % 32 + 1)
    assert torch.equal(again.vf, args[0]) and torch.equal(again.npts, args[1]) and torch.equal(again.coords, args[2])
    assert all(torch.equal(again.sd[k], v) for k, v in args[3].items())


def test_pfn_f64_known_answers_centre_in_float32_and_padded_rows_in_the_max():
    """Two hand-made pillars, C = 1, no BatchNorm.  (1) Only the x weight of f_center is set and the single point lies 2^-12 m beside the FLOAT32 centre of a far cell:
    the answer is exactly 2^-12; a centre formed in float64 would shift it by the centre's rounding error, which this cell makes nonzero.  (2) The valid row answers
    0.4, the padded rows answer relu(bias) = 0.5: the padded rows win the max."""
    vs, rg = [0.4, 0.4, 4.0], [-140.8, -40.0, -3.0, 140.8, 40.0, 1.0]
    coords = torch.tensor([[0, 0, 7, 701]], dtype=torch.int32)
    c32 = cell_centres(coords, vs, rg)
    c64 = 701 * 0.4 + (0.2 - 140.8)
    assert c32.dtype == torch.float32 and float(c32[0, 0].double()) != c64                      # the rounding is visible in this cell
    assert torch.equal(c32[0, 0], torch.tensor(701.0) * torch.tensor(0.4) + torch.tensor(0.4 / 2 - 140.8))
    vf = torch.zeros(1, 4, 4)
    vf[0, 0, :3] = c32[0] + torch.tensor([2.0 ** -12, 0.0, 0.0])
    assert float(vf[0, 0, 0].double() - c32[0, 0].double()) == 2.0 ** -12                       # representable: the input itself is exact
    w = torch.zeros(1, 10)
    w[0, 7] = 1.0
    sd = {PREFIX + "linear.weight": w, PREFIX + "linear.bias": torch.zeros(1)}
    out = pfn_f64(vf, torch.tensor([4], dtype=torch.int32), coords, sd, vs, rg)
    assert out.dtype == torch.float64 and float(out[0, 0]) == 2.0 ** -12
    # (2)
    vf = torch.zeros(1, 4, 4)
    vf[0, 0, :3] = c32[0] + torch.tensor([0.125, 0.0, 0.0])
    w = torch.zeros(1, 10)
    w[0, 7] = -1.0
    sd = {PREFIX + "linear.weight": w, PREFIX + "linear.bias": torch.tensor([0.5])}
    assert float(pfn_f64(vf, torch.tensor([1], dtype=torch.int32), coords, sd, vs, rg)[0, 0]) == 0.5
    assert float(pfn_f64(vf[:, :1], torch.tensor([1], dtype=torch.int32), coords, sd, vs, rg)[0, 0]) == 0.375      # P = 1: no padded row


def test_run_length_cases_follow_the_launchers_rules():
    """Group b's pillar counts give the run lengths they are named for under the restated grid rules (tests/pillar_cases.py), on the MI355X's CU count; targets never
    coincide.  (The GPU test repeats this with the CU count the device reports.)"""
    pc.check_run_lengths(pc.MI355X_CUS)


@pytest.mark.parametrize("name", pc.names())
def test_float32_reference_meets_the_bound_on_every_case(name):
    """No case asks of a kernel what the reference's own float32 arithmetic cannot do: its error against float64 is inside the first limit of the bound (2e-6 of the
    scale; the second limit is relative to this very error).  Every case stays inside the encoders' stated operating range and has no empty pillar."""
    case = pc.get_case(name)
    assert case.M == 0 or int(case.npts.min()) >= 1 and int(case.npts.max()) <= case.P
    cells = case.coords[:, 0].long() * case.ny * case.nx + case.coords[:, 2].long() * case.nx + case.coords[:, 3].long()
    assert len(torch.unique(cells)) == case.M                                                    # one pillar per cell: oracle.scatter has no duplicate index
    ctr = cell_centres(case.coords, case.voxel_size, case.lidar_range)
    valid = (torch.arange(case.P)[None, :] < case.npts[:, None])
    off = ((case.vf[:, :, :3] - ctr[:, None, :]).abs() * valid[..., None]).amax(dim=(0, 1)) if case.M else torch.zeros(3)
    half = torch.tensor([0.2, 0.2, case.voxel_size[2] / 2])
    assert bool((off <= half * 1.0001).all()), (name, off)                                       # points inside their cell ...
    assert float(case.vf[:, :, 3].abs().max()) <= 255.0 if case.M else True                       # ... intensity <= 255: (p - c) 2^6 <= 160 and i 2^6 <= 16 320 < 65 504
    err_ref = pc.bound_errors(pc.ref32(case), pc.want64(case), pc.ref32(case))[1]
    print(f"\n{name}: float32 reference {err_ref:.2e} of the scale against float64")
    assert err_ref <= 2e-6, (name, err_ref)
