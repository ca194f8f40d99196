"""The f16 and split16 board-tile kernels (kz_board_conv.hip: "board_conv_f16", "board_conv_split16") to the bit on every
geometry of tests/board_nets.py: raw scalars and logits through eval_packed must be the float64 reference's bits.  The networks
are exact (tests/test_board_nets.py holds the conditions without a GPU), so a difference is a wrong address, pad, pack or batch
offset — in a chunk that is neither first nor last, an output-channel quarter past the second, a buffer rotation that wraps, a
tile that straddles two boards or lies idle, a board group behind the XCD wrap.

Each network three ways: every narrow position (no dense layer, the stem dense, each tower convolution dense) through an f16 and
a split16 engine; every wide variant that touches the tower through the split16 engine; the same variants through the exact-f32
engine of the same model, which shows that the network is exact and not the kernel lenient.  Three launches per case
(`board_nets.launches`): nine board groups with one board in the last, two groups, one board alone; the path and every launch's
workgroup count are asserted.  The three small Ataxx boards at 128 channels run in f16 only — the split16 selector sends them to
its one-launch tower; their 320-channel twins run all three ways (board_nets.NETS) —, Go 13x13 1x128 in split16 only:
tests/test_gpu_exact.py runs its f16 engine."""
import numpy as np
import pytest

from kzero_amd import capi
from tests import board_nets as B
from tests import exact_nets as E
from tests.test_gpu_exact import make_engine, mismatch

pytestmark = pytest.mark.gpu

F16, F32, SPLIT = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
F16_ELSEWHERE = ("go13_1x128",)
F32_PATH = "conv_igemm_f32"  # the exact-f32 engine of every network with wide variants: none is a shape of the one-launch f32 tower


def engines(net, wide):
    """(id, dtype, switches, tower path) of the engines a case runs, in the order given above."""
    f16 = [] if wide or net in F16_ELSEWHERE else [("f16", F16, B.NETS[net][7], "board_conv_f16")]
    split = [("split16", SPLIT, {}, "board_conv_split16")] if B.NETS[net][8] else []
    return f16 + split + ([("f32", F32, {}, F32_PATH)] if wide else [])


# ordered by network and model: board_nets.build keeps the last few, every engine of one model runs in a row
CASES = [(net, d, None, e) for net in B.NETS for d in B.dense_positions(net) for e in engines(net, False)]
CASES += [(net, None, w, e) for net in B.NETS for w in B.wide_positions(net) for e in engines(net, True)]
CASES.sort(key=lambda c: list(B.NETS).index(c[0]))  # (stable: a network's narrow cases, then its wide ones)
IDS = [f"{net}-{e[0]}-{E.wide_id(w) if w else 'none' if d is None else d}" for net, d, w, e in CASES]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@pytest.mark.parametrize("net,dense_at,wide,engine", CASES, ids=IDS)
def test_board_kernel_returns_the_reference_bits(dev, net, dense_at, wide, engine):
    name, dtype, switches, path = engine
    b = B.build(net, dense_at, wide)
    eng = make_engine(capi.Model(blob=b.blob), dev, B.NETS[net][6], dtype, switches)
    assert eng.tower_path == path
    hw = b.meta["board_h"] * b.meta["board_w"]
    for n in B.launches(net):
        assert n <= B.NETS[net][6]
        geometry = eng.launch_geometry(n)
        if dtype != F32:
            assert geometry == (B.workgroups(net, n), 0), f"{n} boards"
        # the thirteen distinct boards, repeated from the fourth on so that no workgroup starts the cycle; one board alone: the last
        idx = np.array([B.BOARDS - 1]) if n == 1 else np.arange(3, 3 + n) % B.BOARDS
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        what = f"{net} {name} dense_at={dense_at} {E.wide_id(wide) if wide else ''}, {n} boards in {geometry[0]} workgroups"
        assert np.array_equal(s, b.ref_scalars[idx]), f"{what}, scalars: " + mismatch(s, b.ref_scalars[idx], 5)
        assert np.array_equal(p, b.ref_policy[idx]), f"{what}, policy: " + mismatch(p, b.ref_policy[idx], hw)
