"""The int8 families of tests/int8_nets.py hold what they promise, on the CPU: the reference alone decides these conditions,
they are not measurements of any kernel.  tests/test_gpu_int8_exact.py holds the int8 engine to the same references' bits.

Exact family: nothing rounds, nothing clamps, and the int8 reference equals the unquantised float64 reference bit for bit.
Rounding family: at every quantised site ties in both directions, values that are no tie and clamps at +127, at the stem's
site clamps at -127 too, at most half of a site's values clamped; and every reference that quantises otherwise — truncation,
ties away from zero, a clamp at -128, X8 from f16(v), the residual in front of the ReLU, a site more, a site less — returns
other outputs, on every case."""
import numpy as np
import pytest

from tests import exact_nets as E
from tests import int8_nets as N

EXACT = [(net, d) for net in N.NETS for d in N.dense_positions(net)]
ROUND = list(N.NETS)


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


@pytest.mark.parametrize("net", ROUND)
def test_rounding_family_meets_its_floors(net):
    b = N.build_round(net, None)
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
def test_every_mutant_returns_other_outputs(net):
    b = N.build_round(net, None)
    for name, m in N.mutants(b).items():
        s, p = N.run_mutant(b, m)
        assert not (np.array_equal(s, b.ref_scalars) and np.array_equal(p, b.ref_policy)), name
    assert {"truncate", "half-away", "clamp-128", "from-f16", "residual-first", "one-site-more", "without-0"} <= set(N.mutants(b))
