"""The case table of the pillar-encoder limit tests (tests/test_pillar_limits_cpu.py, tests/test_pillar_limits_gpu.py): every case is built from its name's seed,
so the CPU test (which proves that float32 arithmetic can meet the bound on a case) and the GPU tests (which hold the kernels to it) see identical inputs.

Groups:
  a  small pillar counts M (one wavefront's run of 1..10 pairs, the second workgroup, the sparse kernel's ``active`` partition)
  b  run lengths on the LDS-round boundaries of both matrix-core encoders, the 32-pair ceiling and the step above it -- derived from the launchers' rules below
  c  one capacity-sized frame for the device-side counts far below the capacity
  d  shapes and flags: P, C, use_absolute_xyz, with_distance, BatchNorm or Linear bias, 4 m and 5 m cells
  e  input range: coinciding points, points on the cell faces, intensities up to 255, the canvas corners of the full range, degenerate weight channels
No case holds a pillar with ``voxel_num_points == 0`` (the reference divides by zero there; the kernels document a deviation), and every value stays inside the
operating range the encoders state (csrc/pillar_sparse.hip, csrc/pillar_scatter.hip: points inside their cell, intensity <= 255).
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from tests.pillar_reference import PREFIX

MI355X_CUS = 256                      # multi_processor_count of the MI355X: what the CPU test builds groups b, c and e with
COUNT_POOL = (1, 2, 15, 16, 17, 31, 32)

# ---------------------------------------------------------------------------------------------------------------- the launchers' grid rules, restated
# csrc/pillar_sparse.hip, encode_sparse():   pairs = (M + 1) / 2;  unit = cus * kWaves(4) * kPairsPerWave(6);  k = clamp((pairs + unit / 2) / unit, 1, 3);
#   blocks = k * cus;  if pairs < 4 blocks: blocks = ceil(pairs / 4);  need = ceil(pairs / (4 * kRunPairs(32)));  if blocks < need: blocks = ceil(need / cus) * cus
# pillar_sparse_kernel:  nwave = 4 blocks;  active = max(1, min(nwave, ceil(pairs / 6)));  wavefront g < active owns pairs [g pairs / active, (g + 1) pairs / active)
SPARSE_ROUND, SPARSE_RUN_MAX = 4, 32
# csrc/pillar_scatter.hip, launch_rows() (matrix-core route):  pairs = (M + 1) / 2;  blocks = min(ceil(pairs / (4 * 2 * kRound(5))), 512);
#   need = ceil(pairs / (4 * kRunPairs(32)));  blocks = max(blocks, need, 1)
# pillar_rows_mx_kernel:  nwave = 4 blocks;  per_wave = ceil(pairs / nwave);  wavefront g owns pairs [g per_wave, min((g + 1) per_wave, pairs))
DENSE_ROUND, DENSE_RUN_MAX, DENSE_RESIDENT_WAVES = 5, 32, 2048


def sparse_launch(M, cus):
    """-> (workgroups, shortest run, longest run) of pillar_sparse_kernel for a capacity AND count of M pillars."""
    pairs = (M + 1) // 2
    unit = cus * 4 * 6
    k = min(max((pairs + unit // 2) // unit, 1), 3)
    blocks = k * cus
    if pairs < blocks * 4:
        blocks = (pairs + 3) // 4
    need = (pairs + 127) // 128
    if blocks < need:
        blocks = (need + cus - 1) // cus * cus
    blocks = max(blocks, 1)
    active = max(1, min(blocks * 4, (pairs + 5) // 6))
    runs = [(g + 1) * pairs // active - g * pairs // active for g in range(active)]
    return blocks, min(runs), max(runs)


def dense_launch(M):
    """-> (workgroups, pairs per wavefront) of pillar_rows_mx_kernel for M pillars."""
    pairs = (M + 1) // 2
    blocks = max(min((pairs + 39) // 40, 512), (pairs + 127) // 128, 1)
    return blocks, (pairs + blocks * 4 - 1) // (blocks * 4)


SPARSE_RUNS = (8, 9, 12, 13, 16, 17, 31, 32)         # 4 | 5 is crossed by group a's M = 8 / 9 ... 10 on one wavefront; 8 | 9, 12 | 13, 16 | 17: full / one-pair last round
DENSE_RUNS = (10, 11, 15, 16, 20, 21, 31, 32)        # 5 | 6 is crossed by group a (M = 40 / 41: four wavefronts x 5 pairs, then 6); 10 | 11, 15 | 16, 20 | 21


def sparse_run_counts(cus):
    """{M: intended run length}: M = 2 r (12 cus) puts exactly r pairs on each of the 3 cus x 4 wavefronts (k = 3 for r >= 5, need = 3 r cus / 32 <= 3 cus up to
    r = 32, active = min(12 cus, 2 r cus) = 12 cus); one pair more than r = 32 makes `need` exceed 3 cus workgroups: a fourth workgroup per CU, shorter runs."""
    out = {2 * r * 12 * cus: r for r in SPARSE_RUNS}
    out[2 * 32 * 12 * cus + 2] = None
    return out


def dense_run_counts():
    """{M: intended run length}: M = 2 r 2048 puts exactly r pairs on each of the 512 x 4 resident wavefronts (ceil(2048 r / 40) >= 512 for r >= 10,
    need = 16 r <= 512 up to r = 32); one pair more than r = 32 makes `need` 513 workgroups."""
    out = {2 * r * DENSE_RESIDENT_WAVES: r for r in DENSE_RUNS}
    out[2 * 32 * DENSE_RESIDENT_WAVES + 2] = None
    return out


def check_run_lengths(cus):
    """Every count of group b gives the run length it is named for under the rules above (so two targets cannot coincide), the step above 32 pairs adds
    workgroups; group a's small counts cross the first round boundary of either kernel and the second workgroup.  Fails loudly when a CU count breaks a target."""
    sparse, dense = sparse_run_counts(cus), dense_run_counts()
    assert len(sparse) == len(SPARSE_RUNS) + 1 and len(dense) == len(DENSE_RUNS) + 1
    for M, r in sparse.items():
        for m in (M, M - 1):
            blocks, lo, hi = sparse_launch(m, cus)
            if r:
                assert (blocks, lo, hi) == (3 * cus, r, r), (m, r, blocks, lo, hi)
            else:
                assert blocks > 3 * cus and hi <= SPARSE_RUN_MAX, (m, blocks, hi)
    for M, r in dense.items():
        for m in (M, M - 1):
            blocks, run = dense_launch(m)
            if r:
                assert (blocks, run) == (512, r), (m, r, blocks, run)
            else:
                assert blocks > 512 and run <= DENSE_RUN_MAX, (m, blocks, run)
    # group a on one wavefront / one workgroup: the small counts cross 4 | 5 pairs (sparse rounds) and 5 | 6 pairs per wavefront (dense rounds) and the second workgroup
    assert [sparse_launch(m, cus)[2] for m in (8, 9, 10, 11, 12)] == [4, 5, 5, 6, 6] and sparse_launch(13, cus)[1:] == (3, 4)
    assert [dense_launch(m) for m in (40, 41, 80, 81)] == [(1, 5), (1, 6), (1, 10), (2, 6)]


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass
class PillarCase:
    name: str
    group: str
    vf: torch.Tensor                   # [M, P, 4] float32
    npts: torch.Tensor                 # [M] int32
    coords: torch.Tensor               # [M, 4] int32 (agent, z, y, x), one pillar per cell
    sd: dict                           # PREFIX + linear.weight and either norm.* (BatchNorm) or linear.bias
    use_abs: bool
    with_dist: bool
    voxel_size: list
    lidar_range: list
    n_agents: int
    ny: int
    nx: int
    info: dict = field(default_factory=dict)

    @property
    def use_norm(self):
        return PREFIX + "norm.weight" in self.sd

    @property
    def default_flags(self):
        return self.use_abs and not self.with_dist and self.use_norm

    @property
    def M(self):
        return int(self.vf.shape[0])

    @property
    def P(self):
        return int(self.vf.shape[1])

    @property
    def C(self):
        return int(self.sd[PREFIX + "linear.weight"].shape[0])

    @property
    def margs(self):
        return {"voxel_size": self.voxel_size, "lidar_range": self.lidar_range, "point_pillar_scatter": {"grid_size": [self.nx, self.ny, 1]}}

    @property
    def pl(self):
        return {"voxel_features": self.vf, "voxel_num_points": self.npts, "voxel_coords": self.coords}


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def make_state(rng, C, use_abs, with_dist, use_norm, special=False):
    """Seeded PFN parameters.  A third of the BatchNorm scales are negative (the row max becomes a min).  ``special`` (group e; needs C >= 8, no distance):
    channels 3 / 4: the three summed xyz weights and the intensity weight are all exactly zero (the contraction's per-channel scale sees wmax == 0) with a
    nonzero / a zero BatchNorm shift; channels 6 / 7: the four summed weights are 1, 2^-7, 2^-14, 2^-20.  Channels 3 and 6 carry a negative scale."""
    cin = (4 if use_abs else 1) + 6 + (1 if with_dist else 0)
    B = 4 if use_abs else 1
    w = (rng.randn(C, cin) * 0.3).astype(np.float32)
    if special:
        assert C >= 8 and not with_dist
        for c in (3, 4):
            w[c, B + 3:B + 6] = -((w[c, 0:3] if use_abs else 0) + w[c, B:B + 3]).astype(np.float32)       # ((abs + cluster) + centre) == 0 exactly, in the kernels' order
            w[c, 3 if use_abs else 0] = 0.0
        for c in (6, 7):
            w[c] = 0.0
            w[c, B + 3:B + 6] = (1.0, 2.0 ** -7, 2.0 ** -14)
            w[c, 3 if use_abs else 0] = 2.0 ** -20
    sd = {PREFIX + "linear.weight": torch.from_numpy(w)}
    if use_norm:
        g = (rng.rand(C) + 0.5).astype(np.float32)
        g[::3] *= -1.0
        b, mu, var = (rng.randn(C) * 0.1).astype(np.float32), (rng.randn(C) * 0.1).astype(np.float32), (rng.rand(C) + 0.5).astype(np.float32)
        if special:
            b[4] = mu[4] = 0.0
        sd.update({PREFIX + "norm.weight": torch.from_numpy(g), PREFIX + "norm.bias": torch.from_numpy(b), PREFIX + "norm.running_mean": torch.from_numpy(mu),
                   PREFIX + "norm.running_var": torch.from_numpy(var)})
    else:
        sd[PREFIX + "linear.bias"] = torch.from_numpy((rng.randn(C) * 0.1).astype(np.float32))
    return sd


def _grid(n_agents, ny, nx, vz, z_min):
    return [0.4, 0.4, float(vz)], [-0.2 * nx, -0.2 * ny, float(z_min), 0.2 * nx, 0.2 * ny, float(z_min) + float(vz)]


def make_case(name, group, M, P=32, C=64, use_abs=True, with_dist=False, use_norm=True, vz=4.0, z_min=-3.0, n_agents=1, ny=8, nx=16, mode="uniform", special=False,
              info=None, counts=None):
    """Pillars in distinct cells (a seeded permutation of the canvas), points uniform inside 98 % of their cell, intensity in [0, 1], counts drawn from
    COUNT_POOL (cut to P, plus P - 1 and P) with the LAST pillar of an odd M full.  ``mode == "range"`` (group e) replaces the points pillar by pillar:
    i % 8 == 0 all points identical, 1 within 1e-4 m of each other, 2 on the four cell faces and the two z ends, 3 intensities 0 / 1 / 255; the first four pillars
    sit in the canvas corners."""
    rng = _rng(name)
    vs, rg = _grid(n_agents, ny, nx, vz, z_min)
    ncell = ny * nx
    assert 0 <= M <= n_agents * ncell, (name, M)
    cells = rng.permutation(n_agents * ncell)[:M]
    if mode == "range" and M >= 4:
        corners = [0, nx - 1, (ny - 1) * nx, ncell - 1]
        cells = np.concatenate([corners, [c for c in cells if c not in corners][:M - 4]]).astype(np.int64)
    coords = np.stack([cells // ncell, np.zeros(M, dtype=np.int64), (cells % ncell) // nx, cells % nx], 1).astype(np.int32)
    pool = sorted({n for n in COUNT_POOL + (P - 1, P) if 1 <= n <= P})
    npts = np.asarray(pool, dtype=np.int32)[rng.randint(0, len(pool), size=M)]
    if M % 2:
        npts[-1] = P
    if counts is not None:
        npts = np.asarray(counts, dtype=np.int32)
    ct = torch.from_numpy(coords)
    from tests.pillar_reference import cell_centres
    ctr = cell_centres(ct, vs, rg).numpy()                                                 # float32, as every implementation forms it
    half = np.array([0.2, 0.2, vz / 2], dtype=np.float32)
    off = (rng.rand(M, P, 3).astype(np.float32) * 2 - 1) * (half * np.float32(0.98))
    inten = rng.rand(M, P, 1).astype(np.float32)
    if mode == "range":
        for i in range(M):
            kind = i % 8
            if kind == 0:
                off[i] = off[i, :1]
                inten[i] = inten[i, :1]
            elif kind == 1:
                off[i] = off[i, :1] * np.float32(0.9) + (rng.rand(P, 3).astype(np.float32) - 0.5) * np.float32(1e-4)
            elif kind == 2:
                sign = np.where(rng.rand(P, 3) < 0.5, -1.0, 1.0).astype(np.float32)
                on_face = np.arange(P)[:, None] % 3 == np.arange(3)[None, :]              # point j lies on a face of axis j % 3, free on the others
                off[i] = np.where(on_face, sign * half, off[i])
            elif kind == 3:
                inten[i, :, 0] = np.asarray([0.0, 1.0, 255.0], dtype=np.float32)[np.arange(P) % 3]
    pts = np.concatenate([ctr[:, None, :] + off, inten], -1).astype(np.float32)
    pts *= (np.arange(P)[None, :] < npts[:, None])[..., None]                              # padding rows hold zeros, as the voxeliser leaves them
    sd = make_state(rng, C, use_abs, with_dist, use_norm, special)
    return PillarCase(name, group, torch.from_numpy(pts), torch.from_numpy(npts), ct, sd, use_abs, with_dist, vs, rg, n_agents, ny, nx, dict(info or {}))


# ---- the table: name -> keyword arguments of make_case
SMALL_M = (1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 39, 40, 41, 79, 80, 81)
SHAPE_P = (1, 5, 31, 32, 33, 64, 65)
SHAPE_C = (1, 3, 4, 32, 33, 60, 63, 64, 65, 128)
FLAG_SETS = [(a, d, n) for a in (True, False) for d in (False, True) for n in (True, False)]         # (use_absolute_xyz, with_distance, use_norm); [0] = the default
FULL_FLAG_SHAPES = ((32, 64), (5, 33), (33, 64), (65, 128))                                            # every flag set at these (P, C); one flag set per other pair
OPV2V_FULL = dict(n_agents=1, ny=200, nx=704, vz=4.0, z_min=-3.0)                                      # |x| up to 140.8 m (pointpillar_coalign.yaml)
DAIR_FULL = dict(n_agents=1, ny=200, nx=504, vz=5.0, z_min=-3.5)                                       # DAIR-V2X: 5 m cells


def _flag_name(a, d, n):
    return ("abs" if a else "noabs") + ("_dist" if d else "") + ("" if n else "_bias")


@functools.lru_cache(maxsize=None)
def table(cus=MI355X_CUS):
    t = {}
    for M in SMALL_M:
        t[f"a_M{M}"] = dict(group="a", M=M)
    big = dict(P=8, n_agents=2, ny=200, nx=704)
    for kind, counts in (("sparse", sparse_run_counts(cus)), ("dense", dense_run_counts())):
        for M, r in counts.items():
            tag = f"r{r}" if r else "above32"
            t[f"b_{kind}_{tag}"] = dict(group="b", M=M, info={"kind": kind, "run": r}, **big)
            t[f"b_{kind}_{tag}_odd"] = dict(group="b", M=M - 1, info={"kind": kind, "run": r}, **big)
    t["c_capacity"] = dict(group="c", M=12 * cus * 16, n_agents=1, ny=200, nx=704)
    i = 0
    for P in SHAPE_P:
        for C in SHAPE_C:
            sets = FLAG_SETS if (P, C) in FULL_FLAG_SHAPES else [FLAG_SETS[i % len(FLAG_SETS)]]
            for (a, d, n) in sets:
                vz, z_min = ((4.0, -3.0), (5.0, -3.5))[i % 2]
                t[f"d_P{P}_C{C}_{_flag_name(a, d, n)}"] = dict(group="d", M=41, P=P, C=C, use_abs=a, with_dist=d, use_norm=n, vz=vz, z_min=z_min)
                i += 1
    for gname, g in (("opv2v", OPV2V_FULL), ("dair", DAIR_FULL)):
        for a in (True, False):
            t[f"e_{gname}_{_flag_name(a, False, True)}_M41"] = dict(group="e", M=41, use_abs=a, mode="range", special=True, **g)
    t["e_opv2v_abs_sparse_r8_odd"] = dict(group="e", M=2 * 8 * 12 * cus - 1, mode="range", special=True, info={"kind": "sparse", "run": 8}, **OPV2V_FULL)
    return t


def names(group=None, cus=MI355X_CUS):
    return [k for k, v in table(cus).items() if group is None or v["group"] == group]


@functools.lru_cache(maxsize=4)
def get_case(name, cus=MI355X_CUS):
    return make_case(name, **table(cus)[name])


# ---------------------------------------------------------------------------------------------------------------- the two references of a case
def want64(case):
    """The float64 yardstick of a case."""
    from tests.pillar_reference import pfn_f64
    return pfn_f64(case.vf, case.npts, case.coords, case.sd, case.voxel_size, case.lidar_range, case.use_abs, case.with_dist)


def ref32(case, chunk=8192):
    """The reference's own float32 evaluation on the CPU: ``oracle.pillar_vfe`` (pinned to the reference's goldens by tests/test_oracle_golden.py) on the default
    flags, ``pfn_f32`` (pinned to tests/golden/pillar_variants.npz by tests/test_pillar_limits_cpu.py) on the flag sets the oracle lacks."""
    from tests.pillar_reference import pfn_f32
    if not case.default_flags:
        return pfn_f32(case.vf, case.npts, case.coords, case.sd, case.voxel_size, case.lidar_range, case.use_abs, case.with_dist)
    from oracle import coalign_oracle as oracle
    rows = [oracle.pillar_vfe(case.vf[m:m + chunk], case.npts[m:m + chunk], case.coords[m:m + chunk], case.sd, case.voxel_size, case.lidar_range)
            for m in range(0, case.M, chunk)]              # (row-independent: chunking changes no value, it bounds the [M, P, C] intermediate)
    return torch.cat(rows) if rows else torch.zeros((0, case.C))


def bound_errors(got, want, ref):
    """-> (error of ``got``, error of the float32 reference), both as max |. - want| over the case divided by the largest |want|."""
    scale = max(float(want.abs().max()), 1e-30)
    return float((got.double() - want).abs().max()) / scale, float((ref.double() - want).abs().max()) / scale


def assert_bound(got, want, ref, what):
    """The project's rule (tests/test_round3_gpu.py::test_matrix_core_encoder_against_float64): max error <= 2e-6 of the float64 output's largest magnitude AND
    <= 4 x the float32 reference's own max error + 2e-7 of that scale.  Prints both errors."""
    err, err_ref = bound_errors(got, want, ref)
    print(f"{what}: error {err:.2e}, float32 reference {err_ref:.2e} of the scale")
    assert err <= 2e-6, (what, err, err_ref)
    assert err <= 4 * err_ref + 2e-7, (what, err, err_ref)
    return err, err_ref
