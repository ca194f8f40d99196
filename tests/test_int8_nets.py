"""The int8 families of tests/int8_nets.py hold what they promise, on the CPU: the reference alone decides these conditions,
they are not measurements of any kernel.  tests/test_gpu_int8_exact.py holds the int8 engine to the same references' bits.

Exact family: nothing rounds, nothing clamps, and the int8 reference equals the unquantised float64 reference bit for bit.
Rounding family: at every quantised site ties in both directions, values that are no tie and clamps at +127, at the stem's
site clamps at -127 too, at most half of a site's values clamped; and every reference that quantises otherwise — truncation,
ties away from zero, a clamp at -128, X8 from f16(v), the residual in front of the ReLU, a site more, a site less — returns
other outputs, on every network of the family (N.ROUND_NETS: a network on which a mutant returned the reference's outputs
would have to be listed in N.EXACT_ONLY and run in the exact family alone).
Weight-rounding variant (N.WEIGHT_NETS): all of the above, and in every conv A weights that are ties in both directions and
weights that are no tie, quantised weights of -127, +127 and an odd value between; the references that truncate the weights
or round their ties away from zero return other outputs too — which is what makes the GPU case fail on a pack that does."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E
from tests import int8_nets as N

EXACT = [(net, d) for net in N.NETS for d in N.dense_positions(net)]
ROUND = list(N.ROUND_NETS)
WEIGHTS = list(N.WEIGHT_NETS)


def test_exponent_is_the_smallest_step_that_holds_the_maximum():
    for k in range(-20, 21):
        m = 127.0 * 2.0 ** k
        assert N.i8_exponent(m) == k
        assert N.i8_exponent(np.nextafter(np.float32(m), np.float32(np.inf))) == k + 1
        assert N.i8_exponent(np.nextafter(np.float32(m), np.float32(0))) == k
    assert N.i8_exponent(1.0) == -6 and N.i8_exponent(128.0) == 1 and N.i8_exponent(65504.0) == 10


def test_quant_rounds_to_nearest_even_and_never_produces_minus_128():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 1000.0, -127.5, -128.0, -1000.0, 0.49, -0.51])
    assert N.quant(v, 0).tolist() == [0, 2, 2, 0, -2, -2, 126, 127, 127, -127, -127, -127, 0, -1]
    assert N.quant(v * 8, 3).tolist() == N.quant(v, 0).tolist()
    assert N.quant(np.array([-128.0, -129.0]), 0, lo=-128.0).tolist() == [-128, -128]


@pytest.mark.parametrize("net,dense_at", EXACT, ids=[f"{n}-{d}" for n, d in EXACT])
def test_exact_family_equals_the_unquantised_reference(net, dense_at):
    b = N.build_exact(net, dense_at)
    depth = b.meta["tower_depth"]
    assert E.conditions_hold(b.plain_report)
    assert b.exps == [0 if b.step >= 1 else -1] * (2 * depth + 1)
    for site, (down, up, other, hi, lo, n) in b.report.counts.items():
        assert (down, up, other, hi, lo) == (0, 0, 0, 0, 0) and n > 0, site
    assert max(float(np.abs(v).max()) for k, v in b.report.sites.items() if not k.endswith(".x")) <= 127
    assert b.report.wq_max <= 127 and all(b.report.exact.values())
    assert N.head_conditions(b.heads, depth)
    assert np.array_equal(b.ref_scalars, b.plain_scalars) and np.array_equal(b.ref_policy, b.plain_policy)
    if dense_at is not None:  # the dense layer's weights are asymmetric and reach every lane of a k-step's fragments
        w = b.tensors[b_layer(b, dense_at) + ".weight"]
        assert len(np.unique(w)) >= 4
        cin = w.shape[1]
        assert all(np.abs(w[:, c0:c0 + 16]).sum() > 0 for c0 in range(0, cin, 16))


def b_layer(b, at):
    return E.layer_names(b.tensors)[at]


def test_boards_per_workgroup_rule():
    per = N.boards_per_workgroup
    assert [per(c, hw) for c, hw in ((256, 64), (128, 64), (128, 49), (128, 81))] == [1, 1, 2, 1]  # the six first networks
    assert [per(128, n * n) for n in (6, 5, 4, 3, 2)] == [3, 4, 7, 12, 28]
    assert [per(256, n * n) for n in (7, 6, 5, 4, 3, 2)] == [1, 1, 2, 4, 7, 16]
    assert per(96, 49) == 2 and per(200, 64) == 1  # widened: the rule takes 128 and 256


@pytest.mark.parametrize("net", list(N.NETS))
def test_plan_runs_the_network_on_the_int8_tower(net):
    """The host's plan, no GPU: every network of the table is accepted by the one-launch int8 tower, at both engine sizes of
    tests/test_gpu_int8_exact.py (which holds the engine's launch geometry to `boards_per_workgroup`)."""
    game, depth, channels, head, kw = N.NETS[net]
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
    quant = model.quantize_int8(np.full(2 * depth + 1, 127.0, np.float32))
    for max_batch in (64, 256):
        assert quant.plan(max_batch, capi.KZ_DTYPE_INT8)[0] == "tower_resident_i8", max_batch


def test_the_table_reaches_every_geometry_it_is_there_for():
    geo = {}
    for net, (game, depth, channels, head, kw) in N.NETS.items():
        spec = synth.game_spec(game)
        hw = spec["size"] ** 2
        chunks = (spec["n_scalar"] + spec["n_bool"] + 31) // 32
        geo[net] = (N.widened(channels), N.boards_per_workgroup(channels, hw), chunks, depth, channels != N.widened(channels))
    assert {g[:2] for g in geo.values()} >= {(128, n) for n in (1, 2, 3, 4, 7, 12, 28)} | {(256, n) for n in (1, 2, 4, 7, 16)}
    assert {(g[0], g[2]) for g in geo.values()} >= {(256, 1), (256, 2), (256, 3), (256, 4), (128, 1), (128, 2)}
    assert max(g[3] for g in geo.values()) >= 4  # three block boundaries
    assert {g[0] for g in geo.values() if g[4]} == {128, 256}  # a widened tower at either width


def test_every_network_is_in_a_family_and_the_widened_ones_round():
    assert set(ROUND) | N.EXACT_ONLY == set(N.NETS) and not set(ROUND) & N.EXACT_ONLY
    assert {"ataxx7_2x96", "chess_2x200_att"} & set(ROUND), "a widened network in the rounding family"
    assert set(WEIGHTS) <= set(ROUND)


def activation_floors(b):
    depth = b.meta["tower_depth"]
    assert len(b.report.counts) == 2 * depth
    for i, (site, (down, up, other, hi, lo, n)) in enumerate(b.report.counts.items()):
        assert down > 0 and up > 0 and other > 0 and hi > 0, (site, down, up, other, hi)
        assert 2 * (hi + lo) <= n, (site, hi, lo, n)
        assert (lo > 0) if i == 0 else True, site
    assert all(b.report.exact.values()), b.report.exact
    assert N.head_conditions(b.heads, depth)
    assert b.report.acc_max < 2 ** 31 and b.report.wq_max <= 127


@pytest.mark.parametrize("net", ROUND)
def test_rounding_family_meets_its_floors(net):
    b = N.build_round(net, None)
    activation_floors(b)
    for l, counts in b.report.wcounts.items():  # (the weights of this family are whole steps: the weight mutants are the reference)
        assert counts == (0, 0, 0), l
    assert "weights-truncate" not in N.mutants(b)


@pytest.mark.parametrize("net", WEIGHTS)
def test_weight_rounding_variant_meets_its_floors(net):
    b = N.build_round(net, None, "round")
    activation_floors(b)
    depth = b.meta["tower_depth"]
    for l in range(1, 2 * depth + 1):
        down, up, other = b.report.wcounts[l]
        if l % 2 == 0:  # conv B: whole steps, its output reaches the unquantised stream
            assert (down, up, other) == (0, 0, 0), l
            continue
        assert down > 0 and up > 0 and other > 0, (l, down, up, other)
        wq = b.report.wq[l]
        assert -127 in wq and 127 in wq and any(v % 2 == 1 for v in wq if abs(v) < 127), (l, wq)
    plain = N.build_round(net, None)
    assert not (np.array_equal(b.ref_scalars, plain.ref_scalars) and np.array_equal(b.ref_policy, plain.ref_policy))


def every_mutant_differs(b):
    for name, m in N.mutants(b).items():
        s, p = N.run_mutant(b, m)
        assert not (np.array_equal(s, b.ref_scalars) and np.array_equal(p, b.ref_policy)), name
    assert {"truncate", "half-away", "clamp-128", "from-f16", "residual-first", "one-site-more", "without-0"} <= set(N.mutants(b))


@pytest.mark.parametrize("net", ROUND)
def test_every_mutant_returns_other_outputs(net):
    every_mutant_differs(N.build_round(net, None))


@pytest.mark.parametrize("net", WEIGHTS)
def test_every_mutant_of_the_weight_variant_returns_other_outputs(net):
    b = N.build_round(net, None, "round")
    assert {"weights-truncate", "weights-half-away"} <= set(N.mutants(b))
    every_mutant_differs(b)
