"""The chess f16 one-launch tower (kz_tower.hip) with two boards per workgroup reads each line fragment of the LDS image
once per (dx, chunk) and uses it for all three tap rows: tile mt at dy reads what tile mt + dy reads at dy = 0.  What that
can get wrong, and a reference with the same k-step order would share, is a fragment of the wrong board or line, or a
skipped tile that was needed.  Every board of a workgroup has its own MFMA columns and a fixed summation order, so a
board's outputs do not depend on its partner, its place in the workgroup or the batch, bit for bit; and one board per
workgroup (one LDS read per tap and tile, nothing shared) sums in the same order as two."""
import os

import numpy as np
import pytest

from kzero_amd import capi, synth

# two f16 paths of this library against each other on shallow nets (restated from tests/test_gpu_parity.py)
F16_PATHS_ATOL = 2e-3
GENERIC = {"KZ_FORCE_GENERIC": "1", "KZ_NO_BOARD_CONV": "1"}
NOFUSE = {"KZ_NO_FUSED_HEADS": "1"}


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


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("game,switches,path", [
    ("chess", {}, "tower_resident_f16+heads"),
    ("chess", NOFUSE, "tower_resident_f16"),
    ("chess-hist-2", {}, "tower_resident_f16+heads"),  # 47 input planes: the wide stem
    ("chess-hist-2", NOFUSE, "tower_resident_f16"),
], ids=["chess", "chess-nofuse", "chesshist2", "chesshist2-nofuse"])
def test_a_board_does_not_depend_on_its_partner(dev, game, switches, path):
    """Board A alone, as board 0 of a pair, as board 1 of a pair, and as board 0 of a ragged last workgroup."""
    model = capi.Model(blob=synth.random_model(game, 1, 256, "attention", seed=91))
    bits, scalars_in = synth.random_boards(game, 3, seed=92)
    eng = make_engine(model, dev, 4, switches)
    assert eng.tower_path == path and eng.launch_geometry(3) == (2, 2)
    A, B, C = 0, 1, 2
    rows = []
    for order in ([A], [A, B], [B, A], [C, B, A]):
        idx = np.array(order)
        s, p = eng.eval_packed(bits[idx], scalars_in[idx])
        assert np.isfinite(s).all() and np.isfinite(p).all()
        at = order.index(A)
        rows.append((order, s[at].copy(), p[at].copy()))
    assert np.abs(rows[0][2]).max() > 0
    _, s0, p0 = rows[0]
    for order, s, p in rows[1:]:
        ds, dp = np.abs(s - s0).max(), np.abs(p - p0).max()
        print(f"[row reuse] {game} {path} A in {order} against A alone: max |d scalars| {ds:g}, max |d policy| {dp:g}")
        assert np.array_equal(s, s0), f"A's scalars in {order} differ from A alone: max |d| {ds:g}"
        assert np.array_equal(p, p0), f"A's policy in {order} differs from A alone: max |d| {dp:g}"


@pytest.mark.gpu
def test_one_board_per_workgroup_equals_two(dev):
    """Reused line fragments (two boards per workgroup) against one LDS read per tap and tile (KZ_TOWER_NB=1), both in the
    product library.  The commit before the row reuse (both instances with plain reads, k-steps in tap order) is
    bit-identical on these inputs: max |d scalars| 0, max |d policy| 0 — a tile that falls off the board adds exact zeros
    with one board per workgroup and is left out with two.  So the bound is equality."""
    game = "chess"
    model = capi.Model(blob=synth.random_model(game, 2, 256, "attention", seed=93))
    bits, scalars_in = synth.random_boards(game, 5, seed=94)
    two = make_engine(model, dev, 8, {})
    one = make_engine(model, dev, 8, {"KZ_TOWER_NB": "1"})
    assert two.tower_path == one.tower_path == "tower_resident_f16+heads"
    assert two.launch_geometry(5) == (3, 2)
    assert one.launch_geometry(5) == (5, 1)
    s2, p2 = two.eval_packed(bits, scalars_in)
    s1, p1 = one.eval_packed(bits, scalars_in)
    ds, dp = np.abs(s1 - s2).max(), np.abs(p1 - p2).max()
    print(f"[row reuse] {game} one board per workgroup against two: max |d scalars| {ds:g}, max |d policy| {dp:g}")
    assert np.isfinite(p2).all() and np.abs(p2).max() > 0
    assert np.array_equal(s1, s2) and np.array_equal(p1, p2)


@pytest.fixture(scope="module")
def depth1(dev):
    """A depth-1 network, three boards, and the per-layer implicit-GEMM path's outputs (computed once)."""
    model = capi.Model(blob=synth.random_model("chess", 1, 256, "attention", seed=95))
    bits, scalars_in = synth.random_boards("chess", 3, seed=96)
    gen = make_engine(model, dev, 4, GENERIC)
    assert gen.tower_path == "conv_igemm_f16"
    sg, pg = gen.eval_packed(bits, scalars_in)
    return model, bits, scalars_in, sg, pg


@pytest.mark.gpu
@pytest.mark.parametrize("nb", ["1", "2"])
def test_depth_1_agrees_with_the_per_layer_path(dev, depth1, nb):
    """Two tower layers and the heads, batch 3 (a full and a ragged workgroup), against conv_igemm_f16: same operands and
    rounding points, another summation order — the bound the project holds for the depth-2 case."""
    model, bits, scalars_in, sg, pg = depth1
    eng = make_engine(model, dev, 4, {"KZ_TOWER_NB": nb})
    assert eng.tower_path == "tower_resident_f16+heads"
    assert eng.launch_geometry(3) == ((3, 1) if nb == "1" else (2, 2))
    s, p = eng.eval_packed(bits, scalars_in)
    ds, dp = np.abs(sg - s).max(), np.abs(pg - p).max()
    print(f"[row reuse] depth 1, NB={nb} vs implicit GEMM f16: max |d scalars| {ds:.2e}, max |d policy| {dp:.2e}")
    assert ds < F16_PATHS_ATOL and dp < F16_PATHS_ATOL
