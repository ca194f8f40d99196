"""The chess f16 one-launch tower with two boards per workgroup issues the MFMAs of a k-step in the boustrophedon of
kzero_amd/csrc/kz_tower_mfma_order.hpp (tests/test_tower_mfma_order_cpp.py holds the table itself).  Every accumulator
still receives one MFMA per k-step in the same k order, so no sum changes: the launch must return the bits of the
one-board-per-workgroup instance of the same library (KZ_TOWER_NB=1), which keeps the ascending order.  What the order can
get wrong is an accumulator that misses its MFMA or gets another's, a wrong B register, or the bias entering at a position
of the order instead of at the accumulator's first MFMA.

Depth 1 is the smallest network that runs a full three-dx layer followed by the last conv B; depth 2 crosses a seam between
two layers of the layer loop.  Batches 1, 2 and 3: a missing partner, a full pair, a ragged tail behind a full pair.  The
chess-history network (47 input planes) is the WIDE instantiation (test_wide_instance says what it can be held to)."""
import os

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O

NOFUSE = {"KZ_NO_FUSED_HEADS": "1"}
BATCHES = (1, 2, 3)
F16_REL, F16_RMS = 3.5e-3, 6e-4  # tests/test_gpu_parity.py's assert_f16, restated


def make_engine(model, dev, max_batch, switches):
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        return capi.Engine(model, dev, max_batch, capi.KZ_DTYPE_F16)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Ref:
    """A network, its boards and the oracle's outputs at the largest batch: computed once per module, never written to."""
    _cache = {}

    def __init__(self, game, depth):
        self.blob = synth.random_model(game, depth, 256, "attention", seed=410 + depth)
        self.bits, self.scalars_in = synth.random_boards(game, max(BATCHES), seed=420 + depth)
        net = O.OracleNet(self.blob)
        x = O.encode_input_full(self.bits, self.scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        self.s, self.p = net.forward(x)
        for a in (self.bits, self.scalars_in, self.s, self.p):
            a.setflags(write=False)

    @classmethod
    def get(cls, game, depth):
        if (game, depth) not in cls._cache:
            cls._cache[game, depth] = cls(game, depth)
        return cls._cache[game, depth]


def assert_f16(actual, ref, what):
    scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    rel = float((np.abs(actual - ref) / scale).max())
    rms = float(np.sqrt(np.mean(((actual - ref) / scale) ** 2)))
    print(f"[mfma order] {what}: max |delta| / scale = {rel:.3e}, rms = {rms:.3e}")
    assert rel <= F16_REL, f"{what}: max |delta| / scale = {rel:.3e} > {F16_REL}"
    assert rms <= F16_RMS, f"{what}: rms |delta| / scale = {rms:.3e} > {F16_RMS}"


def check_bits(game, depth, switches, path, batches, one_board_instance=True):
    assert capi.device_count() >= 1
    ref = Ref.get(game, depth)
    model = capi.Model(blob=ref.blob)
    two = make_engine(model, 0, 4, switches)
    one = make_engine(model, 0, 4, dict(switches, KZ_TOWER_NB="1"))
    assert two.tower_path == one.tower_path == path
    out = {}
    for batch in batches:
        assert two.launch_geometry(batch) == ((batch + 1) // 2, 2)
        assert one.launch_geometry(batch) == ((batch, 1) if one_board_instance else two.launch_geometry(batch))
        s2, p2 = two.eval_packed(ref.bits[:batch], ref.scalars_in[:batch])
        s1, p1 = one.eval_packed(ref.bits[:batch], ref.scalars_in[:batch])
        ds, dp = np.abs(s1 - s2).max(), np.abs(p1 - p2).max()
        print(f"[mfma order] {game} depth {depth} {path} batch {batch}: max |d scalars| {ds:g}, max |d policy| {dp:g}")
        assert np.isfinite(p2).all() and np.abs(p2).max() > 0 and np.abs(s2).max() > 0
        assert np.array_equal(s1, s2), f"scalars differ at batch {batch}: max |d| {ds:g}"
        assert np.array_equal(p1, p2), f"policy differs at batch {batch}: max |d| {dp:g}"
        out[batch] = (s2, p2)
    return ref, out


@pytest.mark.gpu
@pytest.mark.parametrize("switches,path", [({}, "tower_resident_f16+heads"), (NOFUSE, "tower_resident_f16")],
                         ids=["heads", "nofuse"])
@pytest.mark.parametrize("depth", [1, 2])
def test_boustrophedon_returns_the_bits_of_the_ascending_order(depth, switches, path):
    ref, out = check_bits("chess", depth, switches, path, BATCHES)
    s, p = out[3]
    assert_f16(s, ref.s, f"depth {depth} {path} batch 3, scalars vs oracle")
    assert_f16(p, ref.p, f"depth {depth} {path} batch 3, policy vs oracle")


@pytest.mark.gpu
def test_wide_instance():
    """The wide stem has no one-board-per-workgroup instance: KZ_TOWER_NB=1 leaves such a network on the two-board launch, so
    the comparison of the two engines holds the launch to itself only (a second engine of the same model, the same bits).
    What holds the WIDE instantiation's sums is the oracle here, within the f16 tolerances, and the exact chess-history
    networks of tests/test_gpu_exact.py at zero error."""
    ref, out = check_bits("chess-hist-2", 1, {}, "tower_resident_f16+heads", (2,), one_board_instance=False)
    s, p = out[2]
    assert_f16(s, ref.s[:2], "chess-hist-2 depth 1 batch 2, scalars vs oracle")
    assert_f16(p, ref.p[:2], "chess-hist-2 depth 1 batch 2, policy vs oracle")
