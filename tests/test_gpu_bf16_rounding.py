"""KZ_DTYPE_BF16 on the rounding family (tests/exact_nets.py, tests/test_round_nets.py): networks on which the launch does round,
at every site of `bf16_sites`, ties in both directions and values that are no tie, in the activations, the staged input and
the packed weights.  The engine must return the bits of the float64 reference that rounds at those sites to nearest even:
what a site rounds is one f32 value whatever the order of the sums in front of it, so there is no tolerance.  A truncating
conversion, ties away from zero, a rounding in front of the residual add, a site more or a site less each return other bits
(tests/test_round_nets.py shows that on the CPU, for every case here).

Depth 1 (the last-layer epilogue alone), 2 and 3 (two block boundaries, the weight ring across them), heads inside and
outside; 13 boards, one board, and boards per workgroup + 1.  Beside each input case an exact-f32 engine evaluates the same
model on the same boards and must return the unrounded reference's bits: the network and the boards are what the references
say, it is the bf16 launch that rounds.
"""
import numpy as np
import pytest

from kzero_amd import capi
from tests import exact_nets as E
from tests.test_gpu_exact import mismatch

pytestmark = pytest.mark.gpu

BF16, F32 = capi.KZ_DTYPE_BF16, capi.KZ_DTYPE_F32
MAX_BATCH = 64
# network: (bf16 path, boards per workgroup on an engine of 64, the exact-f32 engine's path)
PATHS = {
    "ataxx7_2x128": ("tower_resident_bf16g+heads", 2, "tower_resident_f32+heads"),
    "go9_3x128": ("tower_resident_bf16g+heads", 1, "tower_resident_f32+heads"),
    "chess_2x256_att": ("tower_resident_bf16g", 1, "tower_resident_f32"),
    "chess_1x192_att": ("tower_resident_bf16g", 1, "conv_igemm_f32"),
}
CASES = [(net, v) for net in E.ROUND_NETS for v in E.round_variants(net)]
IDS = [f"{net}-{E.round_id(v)}" for net, v in CASES]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def which_mutant(b, s, p, n):
    """The one-site-less references the engine's output equals on the first n boards, if any: that names the site."""
    hits = []
    for name, rounding in E.round_mutants(b).items():
        if name.startswith("without-"):
            ms, mp, _ = E.run_mutant(b, rounding)
            if np.array_equal(s, ms[:n]) and np.array_equal(p, mp[:n]):
                hits.append(name)
    return f"equals the reference {' / '.join(hits)}" if hits else "equals no one-site-less reference"


@pytest.mark.parametrize("net,variant", CASES, ids=IDS)
def test_bf16_engine_returns_the_rounding_reference_bits(dev, net, variant):
    path, per, f32_path = PATHS[net]
    b = E.build_round(net, variant)
    assert E.round_conditions_hold(b.report) and b.seed == E.SEED
    model = capi.Model(blob=b.blob)
    eng = capi.Engine(model, dev, MAX_BATCH, BF16)
    assert eng.tower_path == path
    assert path.endswith("+heads") == b.heads_inside
    assert eng.launch_geometry(E.BOARDS) == ((E.BOARDS + per - 1) // per, per)
    hw = b.meta["board_h"] * b.meta["board_w"]
    for n in (E.BOARDS, 1, per + 1):  # ragged: the last workgroup holds fewer boards than the others
        s, p = eng.eval_packed(b.bits[:n], b.scalars_in[:n])
        if not (np.array_equal(s, b.ref_scalars[:n]) and np.array_equal(p, b.ref_policy[:n])):
            print(f"[round] {net} {variant}, {n} boards: {which_mutant(b, s, p, n)}")
        assert np.array_equal(s, b.ref_scalars[:n]), f"{n} boards, scalars: " + mismatch(s, b.ref_scalars[:n], 5)
        assert np.array_equal(p, b.ref_policy[:n]), f"{n} boards, policy: " + mismatch(p, b.ref_policy[:n], hw)
    if variant[0] == "input":
        assert E.round_conditions_hold(b.plain_report)
        exact = capi.Engine(model, dev, MAX_BATCH, F32)
        assert exact.tower_path == f32_path
        s, p = exact.eval_packed(b.bits, b.scalars_in)
        assert np.array_equal(s, b.plain_scalars), "exact f32, scalars: " + mismatch(s, b.plain_scalars, 5)
        assert np.array_equal(p, b.plain_policy), "exact f32, policy: " + mismatch(p, b.plain_policy, hw)
