"""The limit cases of V2X-ViT's three kernels, host side (no GPU): every case tests/test_v2x_limits_gpu.py runs is first held against float32 itself, the packers'
static range guarantee is tested at its edge, and the per-token yardstick is shown to refuse three restatements that are wrong in the way a kernel could be.

1. For every case of tests/v2x_limit_cases.py the float32 op-by-op layer on the CPU is within HALF of ``token_bound`` of the float64 restatement: the inputs never ask
   of a kernel what float32 cannot do.  Measured: agent attention at most 0.35 (q x 16; 0.07 elsewhere), window attention 0.23 (q x 12; 0.08 elsewhere),
   feed-forward 0.04.
2. ``ops.pack_v2x_weights``, ``ops.pack_v2x_window_weights`` and ``ops.pack_v2x_ffn_weights`` return an image at a static bound of 0.98 x 65504 and None at 1.05;
   ``V2XViTFusion`` then reports the reason and its forward equals its float64 route; the synthetic and the recorded cases' weights still pack.
3. ``token_bound`` passes the true float64 layer and refuses: the attention output (hidden vector) clamped at 65504 + 64 -- what an sp16 pair converted towards zero
   saturates to -- on the 1.05 weights with the aligned token; one zero-padded extra agent inside the softmax at n = 4, 6, 7; LayerNorm's eps left out on the token whose
   variance is below it."""
import copy

import pytest
import torch

import v2x_limit_cases as lc
from conftest import assert_elementwise
from coalign_amd import ops
from coalign_amd.fusion import V2XViTFusion
from coalign_amd.synthetic import v2xvit_parameters_
from coalign_amd.v2xvit import folded_agent_attention, folded_feed_forward, folded_window_attention
from v2xvit_reference import ARGS_A, ARGS_B, SEED_A, SEED_B, args, inputs

HALF = 0.5
CLAMP = lc.EDGE + 64.0                                                # the high half at 65504, the low half (x 2^-10) at 65504 / 1024
ARGS_W64 = args(64, 2, 32, [4, 2, 1], lc.DIM_HEADS, lc.WINDOWS, "naive", 2)


# ---- 1. float32 itself on every case -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", lc.AGENT_GROUPS)
@pytest.mark.parametrize("C", [64, 256])
def test_float32_agent_attention_is_within_half_the_bound(C, group):
    worst = 0.0
    for case in lc.agent_cases(C, group):
        layer = lc.agent_layer(C, case.variant)
        ref = lc.agent_reference(layer, case)
        ratio = lc.token_bound(lc.agent_op_by_op(layer, lc.agent_warped_f64(case).float()), ref)
        print(f"C={C} {case.name}: float32 op-by-op layer at {ratio:.3f} of the per-token bound")
        assert ratio <= HALF, (C, case.name, ratio)
        worst = max(worst, ratio)
    print(f"agent attention C={C} {group}: worst {worst:.3f}")


@pytest.mark.parametrize("config,group", lc.WINDOW_PARAMS)
def test_float32_window_attention_is_within_half_the_bound(config, group):
    worst = 0.0
    for case in lc.window_cases(config, group):
        layer = lc.window_layer(config, case.variant)
        ratio = lc.token_bound(lc.window_op_by_op(layer, case.x), lc.window_reference(layer, config, case.x))
        print(f"{config} {case.name}: float32 op-by-op layer at {ratio:.3f} of the per-token bound")
        assert ratio <= HALF, (config, case.name, ratio)
        worst = max(worst, ratio)
    print(f"window attention {config} {group}: worst {worst:.3f}")


@pytest.mark.parametrize("group", lc.FFN_GROUPS)
@pytest.mark.parametrize("shape", lc.FFN_SHAPES, ids=[f"C{C}_M{M}" for C, M in lc.FFN_SHAPES])
def test_float32_feed_forward_is_within_half_the_bound(shape, group):
    C, M = shape
    worst = 0.0
    for case in lc.ffn_cases(C, M, group):
        layer = lc.ffn_layer(C, M, case.variant)
        ratio = lc.token_bound(lc.ffn_op_by_op(layer, case.x), lc.ffn_reference(layer, case.x))
        print(f"C={C} M={M} {case.name}: float32 op-by-op layer at {ratio:.3f} of the per-token bound")
        assert ratio <= HALF, (shape, case.name, ratio)
        worst = max(worst, ratio)
    print(f"feed-forward C={C} M={M} {group}: worst {worst:.3f}")


def test_every_group_has_cases_and_every_planted_token_is_there():
    """No case and no planted token is skipped: every group yields cases (``fc2x40`` for split attention alone), and ``plant`` writes all seven tokens."""
    for C in (64, 256):
        assert all(lc.agent_cases(C, g) for g in lc.AGENT_GROUPS)
    assert len(lc.WINDOW_PARAMS) == 3 * len(lc.WINDOW_GROUPS) - 2 and ("C256_split_attn", "fc2x40") in lc.WINDOW_PARAMS
    assert all(lc.window_cases(config, g) for config, g in lc.WINDOW_PARAMS)
    for C, M in lc.FFN_SHAPES:
        assert all(lc.ffn_cases(C, M, g) for g in lc.FFN_GROUPS)
    assert sorted(len(c.x) for c in lc.agent_cases(64, "counts")) == sorted(2 * list(range(1, 9)))
    x = lc.plant(torch.full((2, 2, 7, 64), 7.0), torch.Generator().manual_seed(0))
    assert len(lc.PLANTED) == 7 and bool((x[0, 1] != 7.0).any(dim=-1).all()) and bool((x[0, 0] == 7.0).all()) and bool((x[1] == 7.0).all())
    assert bool((x[0, 1, 0] == 3.0).all()) and bool((x[0, 1, 1] == 0).all()) and float(x[0, 1, 4].abs().sum()) == 1e3
    assert float(x[0, 1, lc.TINY].var(unbiased=False)) < 1e-5 < float(x[0, 1, 6].var(unbiased=False))
    assert 9.0 < float(x[0, 1, 2].mean()) < 11.0 and 29.0 < float(x[0, 1, 3].mean()) < 31.0


def test_the_per_token_bound_sees_what_a_whole_tensor_scale_hides():
    """One token of mean 1e4 in a unit map: an error of 3e-5 in a unit token is inside ``assert_elementwise`` (floor 0.1) and 3 x outside ``token_bound``."""
    ref = torch.randn(1, 4, 4, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref[0, 0, 0] += 1e4
    got = ref.clone()
    k = int(ref[0, 2, 2].abs().argmin())
    got[0, 2, 2, k] += 3e-5 * float(ref[0, 2, 2].abs().max())
    assert_elementwise(got, ref, "whole-tensor scale")
    assert 2.5 < lc.token_bound(got, ref) <= 3.0
    assert lc.token_bound(ref, ref) == 0.0 and lc.token_bound(ref.float(), ref) < 1e-2
    bad = ref.clone(); bad[0, 1, 1, 0] = float("nan")
    assert lc.token_bound(bad, ref) == float("inf")


# ---- 2. the packers at the edge of their guarantee ---------------------------------------------------------------------------------------------------------------
def _pack_agent(layer):
    with torch.no_grad():
        return ops.pack_v2x_weights(*folded_agent_attention(layer.norm, layer.fn, True))


def _pack_window(layer):
    pw = layer.fn
    sa = pw.split_attn if pw.fuse_mehod == "split_attn" else None
    with torch.no_grad():
        return ops.pack_v2x_window_weights(*folded_window_attention(layer.norm, pw), split=None if sa is None else (sa.fc1.weight, sa.bn1.weight, sa.bn1.bias, sa.fc2.weight))


def _pack_ffn(layer):
    with torch.no_grad():
        return ops.pack_v2x_ffn_weights(*folded_feed_forward(layer.norm, layer.fn))


def test_packers_take_098_and_refuse_105_of_the_range():
    """The static bound of the layers ``edge`` and ``outside`` IS 0.98 and 1.05 of 65504 (every branch of the window layer), every single weight is far inside the
    range, the first packs and the second does not; the aligned token comes within 5 % of the bound (the mean-free part of a row is all LayerNorm lets through:
    0.964 at (C, M) = (64, 512), 0.997 - 1.000 elsewhere) where random tokens stay below half of it."""
    for C in (64, 256):
        for variant, frac in (("base", None), ("q16", None), ("edge", lc.INSIDE), ("outside", lc.OUTSIDE)):
            layer = lc.agent_layer(C, variant)
            w, b = lc.agent_value_rows(layer)
            if frac is not None:
                assert abs(float(lc.static_bound(w, b).max()) / lc.EDGE - frac) < 1e-5 and float(w.abs().max()) < lc.EDGE / 4
            assert (_pack_agent(layer) is None) == (variant == "outside"), (C, variant)
        w, b = lc.agent_value_rows(lc.agent_layer(C, "edge"))
        tok = lc.aligned_token(w, b).double()
        yhat = (tok - tok.mean()) / torch.sqrt(tok.var(unbiased=False) + 1e-5)
        reach = float((w @ yhat + b).abs().max()) / float(lc.static_bound(w, b).max())
        rand = torch.randn(200, C, dtype=torch.float64, generator=torch.Generator().manual_seed(C))
        rand = (rand - rand.mean(dim=1, keepdim=True)) / torch.sqrt(rand.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
        reach_random = float((rand @ w.t() + b).abs().max()) / float(lc.static_bound(w, b).max())
        print(f"agent attention C={C}: the aligned token reaches {reach:.4f} of the static bound, 200 random tokens {reach_random:.3f}")
        assert 0.95 <= reach <= 1.0 and reach_random < 0.5
    for config in lc.WINDOW_CONFIGS:
        for variant, frac in (("base", None), ("q12", None), ("pos30", None), ("edge", lc.INSIDE), ("outside", lc.OUTSIDE)):
            layer = lc.window_layer(config, variant)
            for b in range(3):
                w, bias = lc.window_value_rows(layer, b)
                if frac is not None:
                    assert abs(float(lc.static_bound(w, bias).max()) / lc.EDGE - frac) < 1e-5 and float(w.abs().max()) < lc.EDGE / 4
            assert (_pack_window(layer) is None) == (variant == "outside"), (config, variant)
        # one branch outside is enough
        one = copy.deepcopy(lc.window_layer(config, "edge"))
        with torch.no_grad():
            one.fn.pwmsa[1].to_qkv.weight[2 * one.fn.pwmsa[1].to_qkv.weight.shape[0] // 3:].mul_(lc.OUTSIDE / lc.INSIDE)
        assert _pack_window(one) is None, config
    assert _pack_window(lc.window_layer("C256_split_attn", "fc2x40")) is not None
    for C, M in lc.FFN_SHAPES:
        for variant, frac in (("base", None), ("edge", lc.INSIDE), ("outside", lc.OUTSIDE)):
            layer = lc.ffn_layer(C, M, variant)
            w, b = lc.ffn_hidden_rows(layer)
            if frac is not None:
                assert abs(float(lc.static_bound(w, b).max()) / lc.EDGE - frac) < 1e-5
            assert (_pack_ffn(layer) is None) == (variant == "outside"), (C, M, variant)
        w, b = lc.ffn_hidden_rows(lc.ffn_layer(C, M, "edge"))
        tok = lc.aligned_token(w, b).double()
        yhat = (tok - tok.mean()) / torch.sqrt(tok.var(unbiased=False) + 1e-5)
        reach = float((w @ yhat + b).abs().max()) / float(lc.static_bound(w, b).max())
        print(f"feed-forward C={C} M={M}: the aligned token reaches {reach:.4f} of the static bound")
        assert 0.95 <= reach <= 1.0, (C, M)


def test_packers_refuse_through_the_bias_alone_and_non_finite_values():
    layer = lc.agent_layer(64, "base")
    with torch.no_grad():
        wqkv, bqkv, wa, ba = folded_agent_attention(layer.norm, layer.fn, True)
    assert ops.pack_v2x_weights(wqkv, bqkv, wa, ba) is not None
    big = bqkv.clone(); big[2 * 64 + 5] = -65504.0                   # a value row's bias
    assert ops.pack_v2x_weights(wqkv, big, wa, ba) is None
    big = bqkv.clone(); big[5] = -65504.0; big[64 + 5] = 1e6         # a query's and a key's bias: no attention output depends on their size
    assert ops.pack_v2x_weights(wqkv, big, wa, ba) is not None
    nan = bqkv.clone(); nan[2 * 64] = float("nan")
    assert ops.pack_v2x_weights(wqkv, nan, wa, ba) is None
    row = wqkv.clone(); row[2 * 64 + 7] = 1024.0                      # ||row||_2 sqrt(C) = 1024 * 8 * 8 = 65536, every weight far inside
    assert ops.pack_v2x_weights(row, bqkv, wa, ba) is None
    row[2 * 64 + 7] = 1000.0                                          # 64000 + |b| < 65504
    assert ops.pack_v2x_weights(row, bqkv, wa, ba) is not None
    row = wqkv.clone(); row[7] = 1024.0                               # the same row among the queries
    assert ops.pack_v2x_weights(row, bqkv, wa, ba) is not None
    with pytest.raises(ValueError):
        ops.pack_v2x_weights(wqkv, bqkv[:64], wa, ba)
    wl = lc.window_layer("C64_naive", "base")
    with torch.no_grad():
        wqkv, bqkv, wout, bout, pos = folded_window_attention(wl.norm, wl.fn)
    assert ops.pack_v2x_window_weights(wqkv, bqkv, wout, bout, pos) is not None
    for b in range(3):
        big = bqkv.clone(); big[3 * 64 * b + 2 * 64 + 1] = 65504.0
        assert ops.pack_v2x_window_weights(wqkv, big, wout, bout, pos) is None, b
        big = bqkv.clone(); big[3 * 64 * b + 1] = 65504.0; big[3 * 64 * b + 64 + 1] = -1e6
        assert ops.pack_v2x_window_weights(wqkv, big, wout, bout, pos) is not None, b
        row = wqkv.clone(); row[3 * 64 * b + 2 * 64 + 9] = 1024.0
        assert ops.pack_v2x_window_weights(row, bqkv, wout, bout, pos) is None, b
    nan = bqkv.clone(); nan[-1] = float("inf")
    assert ops.pack_v2x_window_weights(wqkv, nan, wout, bout, pos) is None


def _module(a, seed):
    m = V2XViTFusion(copy.deepcopy(a))
    v2xvit_parameters_(m, seed=seed)
    return m.eval()


def push_one_agent_layer_outside_(m, layer_index=1):
    """The value projection of encoder layer ``layer_index``'s agent attention scaled to a static bound of 1.05 x 65504."""
    pre = m.fusion_net.encoder.layers[layer_index][0].layers[0][0]
    lc.scale_agent_values_(pre, lc.OUTSIDE)
    return m


def test_module_reports_the_reason_and_keeps_the_torch_route():
    """The synthetic weights (C = 64 with the kernels' windows, the recorded case B) pack and give no reason.  With one agent-attention layer at 1.05 the module reports
    the static bound, ``routes``' hooks call it a fallback, and its forward (float32) equals its float64 route; likewise the window layer's reason."""
    m = _module(ARGS_W64, 64)
    m.window_kernels = m.ffn_kernels = True
    assert len(m.packed()) == 2 and len(m.packed_windows()) == 2 and len(m.packed_ffn()) == 2
    assert m.kernel_weight_reason() is None and m.window_kernel_reason(64, (16, 32)) is None and m.ffn_kernel_reason(64) is None
    assert m.plan_fusion(64)[:2] == (m.KERNELS_WINDOW_FFN, False)
    for a, seed, C in ((ARGS_A, SEED_A, 32), (ARGS_B, SEED_B, 256)):      # the recorded cases' weights: A has no kernel (C = 32), B packs
        rec = _module(a, seed)
        if C == 256:
            assert rec.packed() is not None and rec.kernel_weight_reason() is None and rec.plan_fusion(256)[:2] == (rec.KERNELS, False)
        else:
            assert rec.kernel_shape_reason(32) is not None and rec.plan_fusion(32)[1] is True      # (the packer is never asked)
    push_one_agent_layer_outside_(m)
    reason = m.kernel_weight_reason()
    assert m.packed() is None and reason is not None and "or the static bound of an attention output" in reason
    line, fallback, _ = m.plan_fusion(64)
    assert fallback and reason in line and line.startswith(m.TORCH)
    assert m.plan_layer("fusion_net.encoder.layers.0.0.layers.0.0.fn.v_linears.0", m.fusion_net.encoder.layers[0][0].layers[0][0].fn.v_linears[0], 64)[1] is True
    assert m.kernel_route(64, 3, (16, 32))                               # (the static half does not look at the weights; ``forward`` does)
    x = torch.randn(4, 64, 16, 32, generator=torch.Generator().manual_seed(108))
    _, rl, A = inputs(64, 0)
    with torch.no_grad():
        got = m(x, rl, A)
        ref = copy.deepcopy(m).double().forward_torch(x.double(), rl, A)
    e = assert_elementwise(got, ref, "float32 forward with an unpackable agent-attention layer vs its float64 route")
    print(f"module with one agent-attention layer at 1.05: float32 forward at {e:.2e} of the scale from float64")
    w = _module(ARGS_W64, 64)
    w.window_kernels = True
    lc.scale_window_values_(w.fusion_net.encoder.layers[0][0].layers[0][1], lc.OUTSIDE)
    assert w.packed_windows() is None and w.packed() is not None
    assert "or the static bound of an attention output" in w.window_kernel_reason(64, (16, 32)) and w.plan_fusion(64)[:2] == (w.KERNELS, False)


# ---- 3. the yardstick can fail -------------------------------------------------------------------------------------------------------------------------------------
def _clamped(layer, modules):
    """The layer in float64 with the input of ``modules`` (the product that reads the LDS tile) clamped at +-(65504 + 64)."""
    hooks = [mod.register_forward_pre_hook(lambda _m, inp: (inp[0].clamp(-CLAMP, CLAMP),)) for mod in modules]
    return hooks


@pytest.mark.parametrize("C", [64, 256])
def test_yardstick_refuses_a_clamped_attention_output(C):
    """On the 1.05 weights with the aligned token (n = 1: o is v' of the token) the float64 module equals the restatement; with o clamped at 65504 + 64 it is refused."""
    layer = copy.deepcopy(lc.agent_layer(C, "outside")).double()
    x = torch.randn(1, 5, 7, C, generator=torch.Generator().manual_seed(C))
    x[0, 2, 3] = lc.aligned_token(*lc.agent_value_rows(layer))
    ref = lc.agent_reference(layer, lc.Case("", "", x))
    true = lc.token_bound(lc.agent_op_by_op(layer, x.double()), ref)
    hooks = _clamped(layer, [layer.fn.a_linears[0]])
    wrong = lc.token_bound(lc.agent_op_by_op(layer, x.double()), ref)
    for h in hooks:
        h.remove()
    print(f"agent attention C={C}: true float64 layer {true:.2e}, o clamped {wrong:.1f} of the per-token bound")
    assert true < 1e-6 and wrong > 1.0


def test_yardstick_refuses_clamped_window_outputs_and_a_clamped_hidden_vector():
    for config in lc.WINDOW_CONFIGS:
        C = lc.WINDOW_CONFIGS[config][0]
        layer = copy.deepcopy(lc.window_layer(config, "outside")).double()
        x = torch.randn(1, 16, 16, C, generator=torch.Generator().manual_seed(C))
        x[0, 4:8, 8:12] = lc.aligned_token(*lc.window_value_rows(layer, 0))
        ref = lc.window_reference(layer, config, x)
        true = lc.token_bound(lc.window_op_by_op(layer, x.double()), ref)
        hooks = _clamped(layer, [att.to_out[0] for att in layer.fn.pwmsa])
        wrong = lc.token_bound(lc.window_op_by_op(layer, x.double()), ref)
        for h in hooks:
            h.remove()
        print(f"window attention {config}: true float64 layer {true:.2e}, o_b clamped {wrong:.1f} of the per-token bound")
        assert true < 1e-6 and wrong > 1.0, config
    for C, M in ((64, 32), (256, 224)):
        layer = copy.deepcopy(lc.ffn_layer(C, M, "outside")).double()
        tok = lc.aligned_token(*lc.ffn_hidden_rows(layer))
        x = torch.randn(8, C, generator=torch.Generator().manual_seed(M))
        x[0], x[1] = tok, -tok
        ref = lc.ffn_reference(layer, x)
        true = lc.token_bound(lc.ffn_op_by_op(layer, x.double()), ref)
        hooks = _clamped(layer, [layer.fn.net[3]])
        wrong = lc.token_bound(lc.ffn_op_by_op(layer, x.double()), ref)
        for h in hooks:
            h.remove()
        print(f"feed-forward C={C} M={M}: true float64 layer {true:.2e}, hidden vector clamped {wrong:.1f} of the per-token bound")
        assert true < 1e-6 and wrong > 1.0, (C, M)


@pytest.mark.parametrize("n", [4, 6, 7])
@pytest.mark.parametrize("C", [64, 256])
def test_yardstick_refuses_a_zero_padded_agent_inside_the_softmax(C, n):
    """What a kernel with a live slot too many would compute: agent n + 1, all zero, a key like the others (LayerNorm(0) = beta)."""
    layer = copy.deepcopy(lc.agent_layer(C, "base")).double()
    case = [c for c in lc.agent_cases(C, "counts") if len(c.x) == n and c.theta is None][0]
    ref = lc.agent_reference(layer, case)
    true = lc.token_bound(lc.agent_op_by_op(layer, case.x.double()), ref)
    padded = torch.cat([case.x.double(), torch.zeros(1, *case.x.shape[1:], dtype=torch.float64)])
    wrong = lc.token_bound(lc.agent_op_by_op(layer, padded)[:n], ref)
    print(f"agent attention C={C} n={n}: true float64 layer {true:.2e}, one zero agent more {wrong:.1f} of the per-token bound")
    assert true < 1e-6 and wrong > 1.0


def test_yardstick_refuses_layernorm_without_eps():
    """On the token whose variance (1e-6) is below eps (1e-5), for all three layers; the other tokens of the map are ordinary."""
    def without_eps(layer):
        layer = copy.deepcopy(layer)
        layer.norm.eps = 0.0
        return layer
    C = 64
    g = torch.Generator().manual_seed(3)
    x = lc.plant(torch.randn(1, 16, 16, C, generator=g), g, only=(lc.TINY,))
    tiny = (0, 1, lc.TINY)
    assert float(x[tiny].var(unbiased=False)) < 1e-5
    layer = copy.deepcopy(lc.agent_layer(C, "base")).double()
    ref = lc.agent_reference(layer, lc.Case("", "", x))
    results = {"agent attention": (lc.agent_op_by_op(layer, x.double()), lc.agent_op_by_op(without_eps(layer), x.double()), ref)}
    layer = copy.deepcopy(lc.window_layer("C64_naive", "base")).double()
    results["window attention"] = (lc.window_op_by_op(layer, x.double()), lc.window_op_by_op(without_eps(layer), x.double()), lc.window_reference(layer, "C64_naive", x))
    layer = copy.deepcopy(lc.ffn_layer(C, 32, "base")).double()
    results["feed-forward"] = (lc.ffn_op_by_op(layer, x.double()), lc.ffn_op_by_op(without_eps(layer), x.double()), lc.ffn_reference(layer, x))
    for what, (true, wrong, ref) in results.items():
        t, w = lc.token_bound(true[tiny], ref[tiny]), lc.token_bound(wrong[tiny], ref[tiny])
        print(f"{what}: on the tiny token the true float64 layer {t:.2e}, without eps {w:.1f} of the per-token bound")
        assert t < 1e-6 and w > 1.0, what
        assert lc.token_bound(true, ref) < 1e-6, what
