"""The networks of tests/int8_board_nets.py hold what they promise, on the CPU: the reference alone decides these conditions,
they are not measurements of any kernel.  tests/test_gpu_int8_board_exact.py holds the per-layer int8 engine to the same
references' bits.  The floors are those of tests/test_int8_nets.py: exact family — nothing rounds, nothing clamps, the int8
reference equals the unquantised one; rounding family — at every quantised site ties in both directions, non-ties and clamps
at +127, at the stem's site clamps at -127 too, at most half of a site clamped, and every mutant reference returns other
outputs; the weight-rounding variant — conv A's weights tie in both directions, take -127, +127 and odd values between."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E
from tests import int8_board_nets as B
from tests import int8_nets as N
from tests.test_int8_nets import activation_floors, every_mutant_differs

EXACT = [(net, d) for net in B.NETS for d in B.dense_positions(net)]


def test_geometry_is_what_the_table_says():
    assert B.geometry(19, 19) == (23, 1, 11)   # one board, 23 tiles, skewed lines
    assert B.geometry(13, 13) == (11, 2, 11)   # two boards, two idle tiles
    assert B.geometry(9, 9) == (6, 4, 0)       # six tiles a board: boards straddle tiles
    assert B.geometry(7, 7) == (4, 6, 0)       # the skew would cost a board: unskewed lines, six boards
    assert B.geometry(8, 8)[0] == 4 and B.geometry(8, 8)[2] == 0
    assert [B.widened(c) for c in (64, 128, 192, 256, 384)] == [128, 128, 256, 256, 384]
    assert {B.widened(B.NETS[n][2]) // 128 for n in B.WEIGHT_NETS} == {1, 2, 3}  # one network per chunk count


@pytest.mark.parametrize("net", list(B.NETS) + [B.BOTH_PLANS])
def test_plan_runs_the_network_per_layer_and_dtype_5_refuses_it(net):
    game, depth, channels, head, kw = (B.NETS.get(net) or N.NETS[net])
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
    quant = model.quantize_int8(np.full(2 * depth + 1, 127.0, np.float32))
    if net == B.BOTH_PLANS:
        assert quant.plan(64, capi.KZ_DTYPE_INT8_ANY) == quant.plan(64, capi.KZ_DTYPE_INT8_HEADS)
        return
    assert not quant.supports_dtype(capi.KZ_DTYPE_INT8_HEADS)
    assert quant.plan(64, capi.KZ_DTYPE_INT8_ANY)[0] == "board_conv_i8"
    size = synth.game_spec(game)["size"]
    assert quant.launch_geometry(64, capi.KZ_DTYPE_INT8_ANY, B.BOARDS) == (B.workgroups(B.BOARDS, size, size, channels), 0)


@pytest.mark.parametrize("net,dense_at", EXACT, ids=[f"{n}-{d}" for n, d in EXACT])
def test_exact_family_equals_the_unquantised_reference(net, dense_at):
    b = B.build_exact(net, dense_at)
    depth = b.meta["tower_depth"]
    assert E.conditions_hold(b.plain_report)
    assert b.exps == [0 if b.step >= 1 else -1] * (2 * depth + 1)
    for site, (down, up, other, hi, lo, n) in b.report.counts.items():
        assert (down, up, other, hi, lo) == (0, 0, 0, 0, 0) and n > 0, site
    assert b.report.wq_max <= 127 and all(b.report.exact.values())
    assert N.head_conditions(b.heads, depth)
    assert np.array_equal(b.ref_scalars, b.plain_scalars) and np.array_equal(b.ref_policy, b.plain_policy)
    if dense_at is not None:  # asymmetric weights on every lane of a k-step's fragments
        w = b.tensors[E.layer_names(b.tensors)[dense_at] + ".weight"]
        assert len(np.unique(w)) >= 4
        assert all(np.abs(w[:, c0:c0 + 16]).sum() > 0 for c0 in range(0, w.shape[1], 16))


@pytest.mark.parametrize("net", list(B.NETS))
def test_rounding_family_meets_its_floors_and_every_mutant_differs(net):
    b = B.build_round(net)
    activation_floors(b)
    every_mutant_differs(b)


@pytest.mark.parametrize("net", B.WEIGHT_NETS)
def test_weight_rounding_variant_meets_its_floors(net):
    b = B.build_round(net, None, "round")
    activation_floors(b)
    depth = b.meta["tower_depth"]
    for l in range(1, 2 * depth + 1):
        down, up, other = b.report.wcounts[l]
        if l % 2 == 0:
            assert (down, up, other) == (0, 0, 0), l
            continue
        assert down > 0 and up > 0 and other > 0, (l, down, up, other)
        wq = b.report.wq[l]
        assert -127 in wq and 127 in wq and any(v % 2 == 1 for v in wq if abs(v) < 127), (l, wq)
    assert {"weights-truncate", "weights-half-away"} <= set(N.mutants(b))
    every_mutant_differs(b)
