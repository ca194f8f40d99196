"""The layer boundary of the chess f16 one-launch tower with two boards per workgroup (kz_tower_boundary_body.hpp): the
first MFMA into an accumulator adds the bias instead of an initialisation pass, the coming layer's bias and first row
addresses are produced inside the k-loop, and conv A's ReLU runs on the packed f16 bits.  None of it changes a sum or a
rounding point, so the launch must return the bits of the one-board-per-workgroup instance of the same library
(KZ_TOWER_NB=1), which keeps the plain boundary: accumulators := bias, one address block per layer, ReLU on the f32 bits.

Depth 1 is a conv A and the last conv B with the final BN; depth 2 adds a plain conv B; depth 3 goes through the layer loop
a second time with the bias and the row addresses the first trip left behind.  Batches 1, 2, 3 and 5: a missing partner,
a full workgroup, a ragged last workgroup behind a full one and behind two."""
import os

import numpy as np
import pytest

from kzero_amd import capi, synth

NOFUSE = {"KZ_NO_FUSED_HEADS": "1"}
BATCHES = (1, 2, 3, 5)


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


@pytest.mark.gpu
@pytest.mark.parametrize("switches,path", [({}, "tower_resident_f16+heads"), (NOFUSE, "tower_resident_f16")],
                         ids=["heads", "nofuse"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_two_boards_per_workgroup_return_the_bits_of_one(depth, switches, path):
    assert capi.device_count() >= 1
    model = capi.Model(blob=synth.random_model("chess", depth, 256, "attention", seed=170 + depth))
    bits, scalars_in = synth.random_boards("chess", max(BATCHES), seed=180 + depth)
    two = make_engine(model, 0, 8, switches)
    one = make_engine(model, 0, 8, dict(switches, KZ_TOWER_NB="1"))
    assert two.tower_path == one.tower_path == path
    for batch in BATCHES:
        assert two.launch_geometry(batch) == ((batch + 1) // 2, 2) and one.launch_geometry(batch) == (batch, 1)
        s2, p2 = two.eval_packed(bits[:batch], scalars_in[:batch])
        s1, p1 = one.eval_packed(bits[:batch], scalars_in[:batch])
        ds, dp = np.abs(s1 - s2).max(), np.abs(p1 - p2).max()
        print(f"[boundary] depth {depth} {path} batch {batch}: max |d scalars| {ds:g}, max |d policy| {dp:g}")
        assert np.isfinite(p2).all() and np.abs(p2).max() > 0 and np.abs(s2).max() > 0
        assert np.array_equal(s1, s2), f"scalars differ at batch {batch}: max |d| {ds:g}"
        assert np.array_equal(p1, p2), f"policy differs at batch {batch}: max |d| {dp:g}"
