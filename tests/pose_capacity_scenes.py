"""Scenes and graphs that fill online pose correction to its capacities (8 agents, 256 stored boxes per agent, 256 landmarks, 2048 edges), and every decision
the GPU file (tests/test_pose_capacity_gpu.py) takes about them -- all from seeds and from the references, nothing here touches the GPU:
  * ``box_align.build_pose_graph`` (host numpy) is the reference of the construction, ``oracle.pose_graph_lm`` (float64 restatement of g2o's LM) of the solution,
    ``oracle.box_alignment_relative_sample_np`` (pure CPU) of the whole chain; all three are cached per scene;
  * a scene is compared graph for graph only if it is ORDER-ROBUST by ``pose_correction_scenes.order_robust`` (the pile: by ``pile_seed_row``, see there);
    tests/test_pose_capacity_cpu.py asserts that for every scene below, and a scene that fails is replaced by another SEED here, on that CPU evidence alone;
  * ``shuffled`` re-orders the edges inside every landmark: the oracle on the shuffled graph is another summation order of the same problem, i.e. the
    reference's own error, which the CPU file holds inside one tenth of every bound the GPU file uses.
"""
import functools
import math

import numpy as np

from coalign_amd import box_align as ba
from coalign_amd.pose import generate_noise
from oracle import coalign_oracle as oracle
from tests.pose_correction_scenes import THRES, YAW_THRES, corners_of

MAX_AGENTS, STORE_BOXES, MAX_LANDMARKS = 8, 256, 256
NO_UNC = dict(use_uncertainty=False)
# the bounds of tests/test_hip_parity.py::test_pose_graph_solver_vs_reference_graphs_and_oracle and of test_pose_correction_gpu._compare_poses
XY_TOL, YAW_TOL, CHI_RTOL, CHAIN_XY_TOL, CHAIN_DEG_TOL = 1e-6, 1e-7, 1e-9, 1e-5, 1e-4


# ------------------------------------------------------------------------------------------------ scenes
def _boxes(xy, yaw):
    b = np.zeros((len(xy), 7))
    b[:, :2], b[:, 2], b[:, 3:6], b[:, 6] = xy, -1, [3.9, 1.6, 1.56], yaw
    return corners_of(b)


def _to_agent(world, pose):
    th = math.radians(pose[4])
    rot = np.array([[math.cos(th), math.sin(th)], [-math.sin(th), math.cos(th)]])
    return (world - pose[:2]) @ rot.T, th


def _eight_agents(rs):
    return [np.zeros(6)] + [np.array([rs.uniform(-15, 15), rs.uniform(-8, 8), 0, 0, rs.uniform(-30, 30), 0]) for _ in range(MAX_AGENTS - 1)]


@functools.lru_cache(maxsize=None)
def capacity(seed, nx, ny, n_obj=None):
    """8 agents (ego at the origin, the others within +-15 m, +-8 m, +-30 deg) looking at a grid of nx x ny objects, pitch 6 m x 9 m with +-1 m of
    jitter, yaw uniform in +-2.5 (``n_obj``: that many of them, drawn at random); every agent detects the objects inside |x| < 130, |y| < 60 of its frame with
    3 cm of noise and keeps at most the first 256; pose noise ``generate_noise(0.2, 0.2)``.  -> (corners per agent [K_i, 8, 3], noisy poses [8, 6])."""
    rs = np.random.RandomState(seed)
    clean = _eight_agents(rs)
    gx, gy = np.meshgrid((np.arange(nx) - (nx - 1) / 2) * 6.0, (np.arange(ny) - (ny - 1) / 2) * 9.0)
    world = np.stack([gx.ravel() + rs.uniform(-1, 1, gx.size), gy.ravel() + rs.uniform(-1, 1, gx.size)], 1)
    yaw_w = rs.uniform(-2.5, 2.5, len(world))
    if n_obj is not None:
        pick = np.sort(rs.permutation(len(world))[:n_obj])
        world, yaw_w = world[pick], yaw_w[pick]
    corners = []
    for p in clean:
        xy, th = _to_agent(world, p)
        xy = xy + rs.normal(0, 0.03, xy.shape)
        ins = np.nonzero((abs(xy[:, 0]) < 130) & (abs(xy[:, 1]) < 60))[0][:STORE_BOXES]
        corners.append(_boxes(xy[ins], yaw_w[ins] - th))
    noisy = np.array([p + generate_noise(0.2, 0.2, rng=rs) for p in clean])
    return tuple(corners), noisy


@functools.lru_cache(maxsize=None)
def one_over(seed):
    """257 objects, all in range of all 8 agents; agent i (mod 257) does not report object i: 256 boxes per agent (a full store, no overflow), 257 clusters."""
    rs = np.random.RandomState(seed)
    clean = _eight_agents(rs)
    gx, gy = np.meshgrid((np.arange(20) - 9.5) * 3.5, (np.arange(13) - 6) * 3.5)           # a denser grid: all of it inside every agent's range
    world = np.stack([gx.ravel() + rs.uniform(-0.5, 0.5, gx.size), gy.ravel() + rs.uniform(-0.5, 0.5, gx.size)], 1)[:257]
    yaw_w = rs.uniform(-2.5, 2.5, len(world))
    corners = []
    for i, p in enumerate(clean):
        xy, th = _to_agent(world, p)
        xy = xy + rs.normal(0, 0.03, xy.shape)
        assert bool(((abs(xy[:, 0]) < 130) & (abs(xy[:, 1]) < 60)).all())
        seen = np.arange(257) != i
        corners.append(_boxes(xy[seen], yaw_w[seen] - th))
    noisy = np.array([p + generate_noise(0.2, 0.2, rng=rs) for p in clean])
    return tuple(corners), noisy


PILE_VARIANTS = {"se2": {}, "adaptive": dict(adaptive_landmark=True), "unsure": dict(drop_unsure_edge=True)}
# WHY THE PILE NEEDS CARE.  The ego reports ONE box, so one edge pins the landmark and, through it, the common motion of the seven other agents, while chi2 at the
# optimum is ~1e3 .. 1e4 (1792 distinct boxes on one landmark).  Levenberg-Marquardt accepts a step while chi2 falls, and stops where the fall drowns in the
# rounding of chi2: with unit information (pinning eigenvalue 1) that is ~3e-7 rad and, over the 25 m to the agents, ~3e-6 m from the optimum (which has a closed
# form there) -- for the oracle itself, and differently for every summation order (``shuffled``: seed 3 ends 2.9e-6 m from itself, seeds 0 - 3 of a compact layout
# 0.6 .. 1.3e-6 m).  A bound of 1e-6 m between two correct solvers needs the pinning edge to outweigh chi2's rounding: in ``se2`` the ego's box is a confident
# detection (log-variance -14 against N(-4, 1): six shuffles of seeds 0 - 3 end at most 1.1e-7 m / 4.6e-9 rad apart, seed 1 at 4e-15 m).  ``adaptive`` is worse
# by nature -- every agent may turn about a single POINT landmark at no cost -- and most of its seeds end 1e-7 .. 1e-6 m from themselves (seeds 1 - 9, 11, 12);
# seed 10 ends at the same iteration under six shuffles, 1.5e-11 m apart.  ``unsure`` converges in 5 iterations (2e-13 m under six shuffles of seed 0).
PILE_SEEDS = {"se2": 1, "adaptive": 10, "unsure": 0}


@functools.lru_cache(maxsize=None)
def pile(seed, variant):
    """8 agents; the ego reports ONE box, each of the other seven 256 boxes in a ring of radius 0.3 .. 1.2 m around it; pose noise ``generate_noise(0.05, 0.05)``:
    one cluster of 1793 members (its seed: box 0), one landmark; uncertainties N(-4, 1).  ``se2``: yaw spread 0.114 rad (variance ~0.013), the ego's box at
    log-variance -14 (see PILE_SEEDS); ``adaptive``: yaw uniform in +-1.5: a point landmark with doubled certainty; ``unsure``: the small yaw spread, and
    ``drop_unsure_edge`` keeps about a third of the edges.  -> (corners, noisy, uncertainties)."""
    rs = np.random.RandomState(seed)
    clean = _eight_agents(rs)
    centre, yaw0 = np.array([12.0, -5.0]), 0.3
    corners, unc = [], []
    for i, p in enumerate(clean):
        k = 1 if i == 0 else STORE_BOXES
        r, phi = (np.zeros(1), np.zeros(1)) if i == 0 else (rs.uniform(0.3, 1.2, k), rs.uniform(-math.pi, math.pi, k))
        world = centre + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
        yaw_w = yaw0 + (rs.uniform(-1.5, 1.5, k) if variant == "adaptive" else rs.normal(0, 0.114, k))
        xy, th = _to_agent(world, p)
        corners.append(_boxes(xy, yaw_w - th))
        unc.append(rs.normal(-4.0, 1.0, (k, 3)))
    if variant == "se2":
        unc[0] = np.full((1, 3), -14.0)
    noisy = np.array([p + generate_noise(0.05, 0.05, rng=rs) for p in clean])
    return tuple(corners), noisy, tuple(unc)


def uncertainties(corners, seed):
    """Log-variances N(-4, 1) per component, one [K_i, 3] per agent."""
    rs = np.random.RandomState(seed)
    return tuple(rs.normal(-4.0, 1.0, (len(c), 3)) for c in corners)


UNC_FLAGS = {"unc_defaults": {}, "unc_adaptive_normalize": dict(adaptive_landmark=True, normalize_uncertainty=True),
             "unc_drop": dict(drop_hard_boxes=True, drop_unsure_edge=True), "unc_points": dict(landmark_SE2=False)}
# (seed, nx, ny, n_obj).  ``exactly256``: 256 of the 297 objects of a 33 x 9 grid; seeds 1, 4, 5, 7 give exactly 256 landmarks and are order-robust, 7 has the most
# boxes (2040, five agents at 256); seeds 0, 3, 6 are not order-robust and seed 2 gives 257 landmarks.
CAPACITY_SCENES = {"grid16_seed0": (0, 16, 16, None), "grid16_seed1": (1, 16, 16, None), "exactly256": (7, 33, 9, 256)}
LIMIT_SCENES = ("grid17_seed1", "one_over")          # more than 256 clusters without a store overflow
SOLVED_SCENES = tuple(CAPACITY_SCENES) + tuple(f"pile_{v}" for v in PILE_VARIANTS) + tuple(UNC_FLAGS)


def scene(name):
    """-> (corners per agent, noisy poses [8, 6], uncertainties per agent or None, flags of ``build_pose_graph``)."""
    if name in CAPACITY_SCENES:
        return (*capacity(*CAPACITY_SCENES[name]), None, dict(NO_UNC))
    if name.startswith("pile_"):
        return (*pile(PILE_SEEDS[name[5:]], name[5:]), dict(PILE_VARIANTS[name[5:]]))
    if name in UNC_FLAGS:
        corners, noisy = capacity(0, 16, 16)
        return corners, noisy, uncertainties(corners, 11), dict(UNC_FLAGS[name])
    if name == "grid17_seed1":                        # 289 objects, every agent sees fewer than 256 of them, together more than 256
        return (*capacity(1, 17, 17), None, dict(NO_UNC))
    if name == "one_over":
        return (*one_over(0), None, dict(NO_UNC))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ references, cached per scene
@functools.lru_cache(maxsize=None)
def host_graph(name):
    """``box_align.build_pose_graph`` on the scene (limits are not its business: a ``PoseGraph`` with more than 256 landmarks comes back as such)."""
    corners, noisy, unc, flags = scene(name)
    return ba.build_pose_graph(list(corners), noisy, None if unc is None else list(unc), **flags)


def edges_of(g):
    return (g.edge_agent, g.edge_landmark, g.edge_meas, g.edge_info)


@functools.lru_cache(maxsize=None)
def oracle_solution(name, max_iterations=1000):
    """``oracle.pose_graph_lm`` on the host graph -> (vertices [V, 3], stats); callers must not write into it."""
    g = host_graph(name)
    x, stats = oracle.pose_graph_lm(g.vertices, g.kinds, edges_of(g), max_iterations)
    x.setflags(write=False)
    return x, stats


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """``oracle.box_alignment_relative_sample_np``: the oracle's own construction and its own solver -> refined (x, y, yaw in degrees) [8, 3]."""
    corners, noisy, unc, flags = scene(name)
    ref = oracle.box_alignment_relative_sample_np(list(corners), np.array(noisy), None if unc is None else list(unc), **flags)
    ref.setflags(write=False)
    return ref


def shuffled(g, seed):
    """The same graph with the edges inside every landmark in another order (edges stay grouped by ascending landmark)."""
    rs = np.random.RandomState(seed)
    order = np.lexsort((rs.permutation(len(g.edge_agent)), g.edge_landmark))
    return ba.PoseGraph(g.vertices, g.kinds, g.edge_agent[order], g.edge_landmark[order], g.edge_meas[order], g.edge_info[order], g.n_agents)


def pose_error(x, ref, n):
    """Agents of two solutions: (max |dx|, |dy| in m, max |dyaw| modulo 2 pi in rad)."""
    return float(np.abs(x[:n, :2] - ref[:n, :2]).max()), float(np.abs(oracle._normalize_theta(x[:n, 2] - ref[:n, 2])).max())


def relative_to_first(x, n):
    """Agents' poses in the frame of agent 0 ([n, 3]): what a graph without a fixed vertex determines (its optimum is an orbit of the gauge group)."""
    c, s = math.cos(x[0, 2]), math.sin(x[0, 2])
    d = x[:n, :2] - x[0, :2]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], oracle._normalize_theta(x[:n, 2] - x[0, 2])], 1)


def pile_seed_row(corners, noisy):
    """The pile's order-robustness, on the SEED's row only.  ``order_robust`` looks at all pairs and refuses the pile for pairs the greedy pass never reads (boxes
    of two other agents a centimetre apart): after the first cluster no box is free.  -> (the float32 `near` row of box 0 equals the float64 one, the smallest
    |distance - thres| of that row, the smallest distance of |yaw variance - yaw_var_thres|), all from the host functions."""
    tfm = ba.pose_to_tfm(noisy)
    world = np.concatenate([ba.corner_to_center(ba._project_f32(c, tfm[i])) for i, c in enumerate(corners)], 0)
    c32 = np.ascontiguousarray(world[:, :3])
    c64 = c32.astype(np.float64)
    d64 = np.sqrt(((c64[1:] - c64[0]) ** 2).sum(-1))
    sq = (c32 * c32).sum(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        row = np.sqrt(sq + sq.T - 2 * c32 @ c32.T)[0, 1:]
    same = bool(np.array_equal(row < np.float32(THRES), d64 < THRES))
    yaw = world[:, 6]
    members = np.concatenate([[0], 1 + np.nonzero(d64 < THRES)[0]])
    return same, float(np.abs(d64 - THRES).min()), abs(float(np.var(yaw[members])) - YAW_THRES)


# ------------------------------------------------------------------------------------------------ graphs for the solver's entry point
def small_graph(seed, n_agents=3, n_obj=40, yaw_shift=0.0, det_sigma=0.03, pose_sigma=0.2):
    """A capacity-style graph built directly (SE(2) landmarks, unit information): ``n_agents`` agents see every one of ``n_obj`` objects.  With ``yaw_shift`` every
    yaw of the problem (agents, landmarks) is turned by it -- measurements are relative and stay -- and the agents' true yaws are squeezed to within 1e-3 of it:
    with ``yaw_shift = pi`` the true yaws sit at the seam of [-pi, pi) and the pose noise (0.2 deg = 3.5e-3 rad) carries the starting values across it."""
    rs = np.random.RandomState(seed)
    wrap = lambda t: (t + math.pi) % (2 * math.pi) - math.pi
    agents = np.array([[0, 0, 0]] + [[rs.uniform(-15, 15), rs.uniform(-8, 8), rs.uniform(-1e-3, 1e-3) if yaw_shift else math.radians(rs.uniform(-30, 30))]
                                      for _ in range(n_agents - 1)], dtype=np.float64)
    agents[:, 2] += yaw_shift
    if yaw_shift:
        agents[0, 2] -= 4e-4                                          # the fixed ego just below +pi, others on both sides
    objects = np.column_stack([rs.uniform(-50, 50, n_obj), rs.uniform(-30, 30, n_obj), rs.uniform(-2.5, 2.5, n_obj) + yaw_shift])
    e_agent, e_lm, e_meas = [], [], []
    for k, o in enumerate(objects):
        for a, p in enumerate(agents):
            c, s = math.cos(p[2]), math.sin(p[2])
            d = o[:2] - p[:2]
            e_agent.append(a); e_lm.append(n_agents + k)
            e_meas.append([c * d[0] + s * d[1] + rs.normal(0, det_sigma), -s * d[0] + c * d[1] + rs.normal(0, det_sigma), wrap(o[2] - p[2] + rs.normal(0, 0.01))])
    start = agents.copy()
    start[1:, :2] += rs.normal(0, pose_sigma, (n_agents - 1, 2))
    start[1:, 2] += np.radians(rs.normal(0, pose_sigma, n_agents - 1))
    lm = objects + np.column_stack([rs.normal(0, 0.1, (n_obj, 2)), rs.normal(0, 0.01, n_obj)])
    vertices = np.concatenate([start, lm])
    vertices[:, 2] = wrap(vertices[:, 2])
    kinds = np.ones(len(vertices), np.int32)
    kinds[0] = 0
    return ba.PoseGraph(vertices, kinds, e_agent, e_lm, e_meas, np.ones((len(e_agent), 3)), n_agents)


def with_arrays(g, **changes):
    """A copy of ``g`` with some arrays replaced (vertices, kinds, edge_agent, edge_landmark, edge_meas, edge_info, n_agents)."""
    f = dict(vertices=g.vertices.copy(), kinds=g.kinds.copy(), edge_agent=g.edge_agent.copy(), edge_landmark=g.edge_landmark.copy(), edge_meas=g.edge_meas.copy(),
             edge_info=g.edge_info.copy(), n_agents=g.n_agents)
    f.update(changes)
    return ba.PoseGraph(**f)


def empty_graph():
    """Three agents, no landmark, no edge."""
    return ba.PoseGraph(np.array([[0, 0, 0], [5, 1, 0.2], [-4, 2, -0.1]], dtype=np.float64), [0, 1, 1], [], [], np.zeros((0, 3)), np.zeros((0, 3)), 3)


def lonely_agent_graph(seed):
    """Two agents, every edge from the fixed ego: the only free agent has no edge, the reduced system has no column, the landmarks still move."""
    g = small_graph(seed, n_agents=2, n_obj=12)
    keep = g.edge_agent == 0
    return with_arrays(g, edge_agent=g.edge_agent[keep], edge_landmark=g.edge_landmark[keep], edge_meas=g.edge_meas[keep], edge_info=g.edge_info[keep])


def zero_information_agent_graph(seed):
    """``small_graph`` whose agent 1 measures with zero information: it has edges (a column of the reduced system) and nothing pulls on it."""
    g = small_graph(seed, n_agents=3, n_obj=20)
    info = g.edge_info.copy()
    info[g.edge_agent == 1] = 0.0
    return with_arrays(g, edge_info=info)


def refused_graphs():
    """Graphs ``coalign_pose_graph_optimize`` documents as refused (``stats[0] = -1``, vertices untouched), each inside fully allocated arrays, with the line of
    csrc/pose_graph.hip that refuses it BEFORE anything is indexed with the offending value:
      agent_index     an edge whose agent is NA                 :136  a >= NA
      landmark_index  an edge whose landmark is V               :136  l >= NL
      not_contiguous  landmark edges 2, 3, 2                    :142-145  whichever of the two runs of landmark 2 leaves lstart / lend, the ranges cover
                                                                4, 0 or 2 edges, never E = 3
      nine_agents     n_agents = 9 (12 vertices)                :130  NA > kMaxAgents
      landmarks_257   2 agents + 257 landmarks, one edge each   :130  NL > kMaxLandmarks"""
    base = small_graph(5, n_agents=2, n_obj=6)
    a, l = base.edge_agent.copy(), base.edge_landmark.copy()
    a[3] = base.n_agents
    l[-1] = len(base.vertices)
    three = with_arrays(base, edge_agent=np.array([0, 1, 0], np.int32), edge_landmark=np.array([2, 3, 2], np.int32), edge_meas=base.edge_meas[:3],
                        edge_info=base.edge_info[:3])
    nine = small_graph(6, n_agents=9, n_obj=3)
    many = 257
    rs = np.random.RandomState(8)
    v = np.concatenate([[[0, 0, 0], [4, 1, 0.1]], np.column_stack([rs.uniform(-50, 50, many), rs.uniform(-30, 30, many), rs.uniform(-2, 2, many)])])
    wide = ba.PoseGraph(v, [0] + [1] * (many + 1), np.arange(many) % 2, 2 + np.arange(many), rs.normal(0, 1, (many, 3)), np.ones((many, 3)), 2)
    return {"agent_index": with_arrays(base, edge_agent=a), "landmark_index": with_arrays(base, edge_landmark=l), "not_contiguous": three, "nine_agents": nine,
            "landmarks_257": wide}


@functools.lru_cache(maxsize=None)
def free_gauge_graph():
    """The capacity graph without a fixed vertex (``kinds[0] = 1``): 8 free agents, the full 24 x 24 reduced system; its optimum is a gauge orbit."""
    g = host_graph("grid16_seed0")
    kinds = g.kinds.copy()
    kinds[0] = 1
    return with_arrays(g, kinds=kinds)


@functools.lru_cache(maxsize=None)
def solution_of(which, max_iterations=1000):
    """``oracle.pose_graph_lm`` of one of the solver-entry graphs by name -> (vertices, stats); read-only."""
    if which in SCENE_GRAPHS:
        return oracle_solution(SCENE_GRAPHS[which], max_iterations)
    g = ENTRY_GRAPHS[which]()
    x, stats = oracle.pose_graph_lm(g.vertices, g.kinds, edges_of(g), max_iterations)
    x.setflags(write=False)
    return x, stats


def six_dof(noisy, seed):
    """Noisy poses with z, roll and pitch set and a common shift of up to 150 m (entries up to ~300 m), as ``test_corrected_matrices_against_the_host_functions``
    sets them."""
    rs = np.random.RandomState(seed)
    out = np.array(noisy, dtype=np.float64)
    n = len(out)
    out[:, 2], out[:, 3], out[:, 5] = rs.uniform(-0.3, 0.3, n), rs.uniform(-0.5, 0.5, n), rs.uniform(-0.5, 0.5, n)
    out[:, :2] += rs.uniform(-150, 150, 2)
    return out


SIX_DOF_SEEDS = {8: 9, 16: 16}                      # ``six_dof`` seed per max_cav of the matrix test: seeds that leave the scene order-robust (seed 8 does not)
SCENE_GRAPHS = {"capacity": "grid16_seed0", "pile": "pile_se2"}
ENTRY_GRAPHS = {"capacity": lambda: host_graph("grid16_seed0"), "small": lambda: small_graph(1), "pile": lambda: host_graph("pile_se2"), "empty": empty_graph,
                "lonely": lambda: lonely_agent_graph(2), "seam": lambda: small_graph(3, yaw_shift=math.pi), "zero_agent": lambda: zero_information_agent_graph(4),
                "free_gauge": free_gauge_graph}
BATCH = ("capacity", "small", "pile", "empty", "lonely")
