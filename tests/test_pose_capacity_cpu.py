"""The scenes and references of tests/test_pose_capacity_gpu.py, checked on their own (no GPU): every scene holds the counts the GPU file relies on (boxes in all four
wavefronts of the member pass, 237 .. 256 landmarks, a cluster of 1793 members, more than 256 clusters without a store overflow), is order-robust by the host
functions (the pile: on its seed's row), and the oracle agrees with ITSELF -- the same graph with the edges of every landmark in another order, and its own
construction against ``box_align.build_pose_graph`` -- inside one tenth of every bound the GPU file asks of the kernels.  What the device is held to is therefore
something the references meet with a decade to spare."""
import numpy as np
import pytest

from coalign_amd import box_align as ba
from oracle import coalign_oracle as oracle
from tests import pose_capacity_scenes as ps
from tests.pose_correction_scenes import MARGIN, YAW_MARGIN, order_robust

NA = ps.MAX_AGENTS


def _inputs(name):
    corners, noisy, unc, flags = ps.scene(name)
    return list(corners), noisy, None if unc is None else list(unc), flags


# ------------------------------------------------------------------------------------------------ counts and conditions
@pytest.mark.parametrize("name", tuple(ps.CAPACITY_SCENES) + tuple(ps.UNC_FLAGS) + ps.LIMIT_SCENES)
def test_grid_scenes_fill_the_kernels_and_are_order_robust(name):
    corners, noisy, unc, flags = _inputs(name)
    counts = [len(c) for c in corners]
    g = ps.host_graph(name)
    n_lm, E = len(g.vertices) - NA, len(g.edge_agent)
    assert len(corners) == NA and max(counts) <= ps.STORE_BOXES                       # 8 agents, no store overflow
    assert all(order_robust(corners, noisy, unc, **flags)), name                      # decided from the host functions, never from a device result
    assert sum(counts) > 3 * 512 + 64, "thread t of the member pass holds boxes 8 t .. 8 t + 7: boxes in all four wavefronts"
    assert len(np.unique(g.edge_agent)) == NA or name in ps.LIMIT_SCENES
    if name.startswith("grid16") or name in ps.UNC_FLAGS:
        assert 208 <= min(counts) and max(counts) <= 228 and 237 <= n_lm <= 246, (counts, n_lm)
        assert (E == 538 and len(np.unique(g.edge_landmark)) > 200) if name == "unc_drop" else 1720 <= E <= 1770, E
        assert (g.kinds[NA:] == (2 if name == "unc_points" else 1)).all()
    elif name == "exactly256":
        assert n_lm == ps.MAX_LANDMARKS and len(g.vertices) == 264 and counts.count(256) >= 4 and E == sum(counts) == 2040, (n_lm, counts, E)
    elif name == "one_over":
        assert counts == [256] * NA and n_lm == 257 and E == 2048                      # a full store in every slot, one cluster too many
    else:
        assert n_lm == 270 and max(counts) < 256, (n_lm, counts)                       # the natural frame with too many landmarks
    assert (n_lm > ps.MAX_LANDMARKS) == (name in ps.LIMIT_SCENES)                     # the status the host implies: solved, or too many landmarks


@pytest.mark.parametrize("variant", ps.PILE_VARIANTS)
def test_pile_is_one_cluster_and_robust_on_its_seed_row(variant):
    name = f"pile_{variant}"
    corners, noisy, unc, flags = _inputs(name)
    g = ps.host_graph(name)
    assert [len(c) for c in corners] == [1] + [256] * 7
    assert len(g.clusters) == 1 and len(g.clusters[0]) == 1793 and g.clusters[0][0] == 0 and g.clusters[0][-1] == 1792 and len(g.vertices) == NA + 1
    same, d_margin, var_margin = ps.pile_seed_row(corners, noisy)
    print(f"{name}: seed row margins {d_margin:.3f} m, yaw variance {var_margin:.3f} from the threshold")
    assert same and d_margin > MARGIN and var_margin >= YAW_MARGIN
    assert d_margin >= 0.12                                                           # (what the ring's radii 0.3 .. 1.2 m leave under thres = 1.5 m)
    if variant == "adaptive":
        assert g.kinds[NA] == 2 and len(g.edge_agent) == 1793 and not g.edge_info[:, 2].any()
        u = np.concatenate(unc)
        assert np.allclose(g.edge_info[:, 0], 2 * np.exp(-u[:, 0]) / ba.ANCHOR_DIAG_SQ, rtol=1e-12)      # doubled certainty
    elif variant == "unsure":
        assert g.kinds[NA] == 1 and 400 < len(g.edge_agent) < 800 and -(-1793 // 256) == 8   # kept edges are ranked in eight scan rounds of 256 members
    else:
        assert g.kinds[NA] == 1 and len(g.edge_agent) == 1793 and g.edge_agent[0] == 0
        assert g.edge_info[0, 2] == np.exp(14.0) > 10 * ps.oracle_solution(name)[1]["chi2"]          # the pinning edge outweighs chi2 (see PILE_SEEDS)


@pytest.mark.parametrize("max_cav", sorted(ps.SIX_DOF_SEEDS))
def test_matrix_scenes_are_solved_on_the_host(max_cav):
    corners, noisy, unc, flags = _inputs("grid16_seed0")
    poses = ps.six_dof(noisy, ps.SIX_DOF_SEEDS[max_cav])
    g = ba.build_pose_graph(corners, poses, unc, **flags)
    assert g is not None and len(g.vertices) - NA <= ps.MAX_LANDMARKS and float(np.abs(poses[:, :2]).max()) > 100
    assert all(order_robust(corners, poses, unc, **flags))                            # the landmark count does not hang on a summation order


# ------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("name", ps.SOLVED_SCENES)
def test_oracle_is_self_consistent_under_edge_shuffling(name):
    g = ps.host_graph(name)
    x, stats = ps.oracle_solution(name)
    assert stats["chi2"] < stats["chi2_initial"] and stats["iterations"] < 200 and np.array_equal(x[0], g.vertices[0])
    h = ps.shuffled(g, 1)
    assert not np.array_equal(h.edge_agent, g.edge_agent) and np.array_equal(h.edge_landmark, g.edge_landmark)
    y, again = oracle.pose_graph_lm(h.vertices, h.kinds, ps.edges_of(h))
    e_xy, e_yaw = ps.pose_error(x, y, NA)
    e_chi = abs(again["chi2"] - stats["chi2"]) / max(1.0, stats["chi2"])
    print(f"{name}: the oracle on shuffled edges {e_xy:.2e} m {e_yaw:.2e} rad chi2 {e_chi:.2e} (relative)")
    assert e_xy <= ps.XY_TOL / 10 and e_yaw <= ps.YAW_TOL / 10 and e_chi <= ps.CHI_RTOL / 10, (name, e_xy, e_yaw, e_chi)


@pytest.mark.parametrize("name", ps.SOLVED_SCENES)
def test_pure_cpu_chain_agrees_with_the_host_graph_and_the_oracle_solver(name):
    """``oracle.box_alignment_relative_sample_np`` (its own construction) against ``box_align.build_pose_graph`` + ``oracle.pose_graph_lm``."""
    corners, noisy, unc, flags = _inputs(name)
    g, og = ps.host_graph(name), oracle.build_pose_graph(corners, noisy, unc, **flags)
    assert np.array_equal(og["kinds"], g.kinds) and np.array_equal(og["edges"][0], g.edge_agent) and np.array_equal(og["edges"][1], g.edge_landmark)
    assert float(np.abs(og["edges"][2] - g.edge_meas).max()) <= 1e-13 and np.allclose(og["edges"][3], g.edge_info, rtol=1e-14, atol=0)
    x, _ = ps.oracle_solution(name)
    chain = ps.oracle_chain(name)
    e_xy = float(np.abs(chain[:, :2] - x[:NA, :2]).max())
    e_deg = float(np.abs((chain[:, 2] - np.rad2deg(x[:NA, 2]) + 180) % 360 - 180).max())
    print(f"{name}: the pure-CPU chain against host graph + oracle solver {e_xy:.2e} m {e_deg:.2e} deg")
    assert e_xy <= ps.CHAIN_XY_TOL / 10 and e_deg <= ps.CHAIN_DEG_TOL / 10, (name, e_xy, e_deg)


@pytest.mark.parametrize("which", [k for k in ps.ENTRY_GRAPHS if k not in ps.SCENE_GRAPHS])
def test_entry_graphs_and_their_oracle(which):
    g = ps.ENTRY_GRAPHS[which]()
    n = g.n_agents
    x, stats = ps.solution_of(which)
    if which == "empty":
        assert len(g.edge_agent) == 0 and np.array_equal(x, g.vertices) and stats["chi2"] == 0
        return
    h = ps.shuffled(g, 1)
    y, again = oracle.pose_graph_lm(h.vertices, h.kinds, ps.edges_of(h))
    if which == "free_gauge":                                                         # a gauge orbit: chi2 and the poses relative to agent 0
        assert n == NA and not (g.kinds == 0).any()
        d = ps.relative_to_first(np.asarray(x), n) - ps.relative_to_first(y, n)
        e_xy, e_yaw = float(np.abs(d[:, :2]).max()), float(np.abs(oracle._normalize_theta(d[:, 2])).max())
    else:
        e_xy, e_yaw = ps.pose_error(x, y, n)
    e_chi = abs(again["chi2"] - stats["chi2"]) / max(1.0, stats["chi2"])
    print(f"{which}: the oracle on shuffled edges {e_xy:.2e} m {e_yaw:.2e} rad chi2 {e_chi:.2e} (relative)")
    assert e_xy <= ps.XY_TOL / 10 and e_yaw <= ps.YAW_TOL / 10 and e_chi <= ps.CHI_RTOL / 10, (which, e_xy, e_yaw, e_chi)
    if which == "lonely":
        assert not (g.edge_agent == 1).any() and g.kinds[1] == 1 and np.array_equal(x[1], g.vertices[1]) and not np.array_equal(x[2:], g.vertices[2:])
    if which == "zero_agent":
        assert (g.edge_agent == 1).any() and not g.edge_info[g.edge_agent == 1].any() and g.edge_info[g.edge_agent != 1].all()
    if which == "seam":
        true_side = np.abs(np.abs(g.vertices[:n, 2]) - np.pi)
        assert (true_side < 1e-2).all() and len({np.sign(v) for v in g.vertices[:n, 2]}) == 2      # starting values on both sides of the seam
        assert (np.abs(np.abs(x[:n, 2]) - np.pi) < 2e-3).all() and (np.sign(x[1:n, 2]) != np.sign(g.vertices[1:n, 2])).any()   # and the solution crosses it


def test_one_iteration_of_the_oracle_is_self_consistent():
    g = ps.ENTRY_GRAPHS["capacity"]()
    x, stats = ps.solution_of("capacity", 1)
    h = ps.shuffled(g, 1)
    y, again = oracle.pose_graph_lm(h.vertices, h.kinds, ps.edges_of(h), 1)
    e_xy, e_yaw = ps.pose_error(x, y, NA)
    assert stats["iterations"] == 1 and stats["chi2"] < stats["chi2_initial"] and stats["chi2"] > 2 * ps.oracle_solution("grid16_seed0")[1]["chi2"]
    assert e_xy <= ps.XY_TOL / 10 and e_yaw <= ps.YAW_TOL / 10 and abs(again["chi2"] - stats["chi2"]) <= ps.CHI_RTOL / 10 * stats["chi2"]


def test_refused_graphs_stay_inside_their_arrays():
    """Each refused graph is refused for the one reason its name says, and every array is fully allocated: V vertex rows, E edge rows."""
    refused = ps.refused_graphs()
    assert list(refused) == ["agent_index", "landmark_index", "not_contiguous", "nine_agents", "landmarks_257"]
    for why, g in refused.items():
        V, E, n = len(g.vertices), len(g.edge_agent), g.n_agents
        assert g.vertices.shape == (V, 3) and len(g.kinds) == V and len(g.edge_landmark) == E and g.edge_meas.shape == (E, 3) and g.edge_info.shape == (E, 3) and V >= n
        bad_agent, bad_lm = (g.edge_agent < 0) | (g.edge_agent >= n), (g.edge_landmark < n) | (g.edge_landmark >= V)
        sorted_lm = bool(np.all(np.diff(g.edge_landmark) >= 0))
        reasons = {"agent_index": bool(bad_agent.any()), "landmark_index": bool(bad_lm.any()), "not_contiguous": not sorted_lm, "nine_agents": n > 8,
                   "landmarks_257": V - n > 256}
        assert [k for k, v in reasons.items() if v] == [why], (why, reasons)
    assert refused["agent_index"].edge_agent.max() == refused["agent_index"].n_agents and refused["landmark_index"].edge_landmark.max() == len(refused["landmark_index"].vertices)
    assert refused["not_contiguous"].edge_landmark.tolist() == [2, 3, 2] and refused["nine_agents"].n_agents == 9
    assert len(refused["landmarks_257"].vertices) - refused["landmarks_257"].n_agents == 257


def test_oracle_reaches_the_least_squares_optimum_on_a_small_graph():
    """As ``test_pose_graph_lm_reaches_the_least_squares_optimum``: an independent solver (scipy's trust region) on the same residuals, here on a generated graph."""
    from scipy.optimize import least_squares
    g = ps.ENTRY_GRAPHS["small"]()
    edges, n = ps.edges_of(g), g.n_agents
    x, stats = ps.solution_of("small")
    free = np.nonzero(g.kinds != 0)[0]

    def fun(p):
        v = g.vertices.copy()
        v[free] = p.reshape(-1, 3)
        return (oracle.pose_graph_residuals(v, g.kinds, edges) * np.sqrt(edges[3])).ravel()
    sol = least_squares(fun, g.vertices[free].ravel(), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    assert abs(2 * sol.cost - stats["chi2"]) <= 1e-9 * max(1.0, stats["chi2"])
    best = g.vertices.copy()
    best[free] = sol.x.reshape(-1, 3)
    np.testing.assert_allclose(x[:n, :2], best[:n, :2], rtol=0, atol=1e-6)
    assert np.abs(oracle._normalize_theta(x[:n, 2] - best[:n, 2])).max() < 1e-7
