"""Zero-tolerance parity: every kernel instance with addressing of its own evaluates the exactly representable networks of
tests/exact_nets.py and must return the bits of the float64 reference — raw scalars and logits through eval_packed; the
inexact tanh / softmax of the decode are held to a float64 softmax of the same exact logits, within derived bounds, by
tests/test_gpu_decode_exact.py.  On these networks no arithmetic of the library rounds (weights, inputs and
stored intermediates are short dyadic numbers within half of f16's integer range, every sum stays within 2^22 steps:
tests/test_exact_nets.py holds both for every case here), so any difference is a wrong address, pad, pack or batch
offset: exactly the errors that sit below the f16 bounds of tests/test_gpu_parity.py.

Every engine runs with the fully dense layer at each position of its network and with none.  The split16 engines, whose lo
halves are all zero on those networks, run the wide family as well, with the exact-f32 engines of the same networks beside them.  Launches are ragged on
purpose — boards per workgroup x k + 1 boards, and one board alone; the instances that need a full chip before the
engine picks them get that many boards, the thirteen distinct ones repeated.

The board-tile kernel runs here on three networks of depth 1 and at most 128 channels, Go 13x13 in f16 only: one or two
chunks, one or two output-channel quarters, one setting of most of its runtime geometry.  tests/test_gpu_board_exact.py holds
both of its instances to the bit on a table chosen by geometry (tests/board_nets.py), the split16 engines of go9_1x256 and
go13_1x128 with their wide variants among them.
"""
import os

import numpy as np
import pytest

from kzero_amd import capi
from tests import exact_nets as E

F16, F32, SPLIT = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
GENERIC = {"KZ_FORCE_GENERIC": "1", "KZ_NO_BOARD_CONV": "1"}
NOFUSE = {"KZ_NO_FUSED_HEADS": "1"}

# (id, network, dtype, max_batch, switches, tower path, boards per workgroup of the ragged launch or None, its boards)
# Path names: tests/golden/path_table.json and the existing tests (tests/test_exact_nets.py holds them to the selector
# without a GPU).  Boards per workgroup is asserted for every launch that holds whole boards (None: the per-layer paths, whose workgroups hold tiles).
ENGINES = [
    # the chess f16 one-launch kernel (kz_tower.hip): both residual epilogues, one and two boards per workgroup, heads in and out
    ("chess256-f16-nb2", "chess_2x256_att", F16, 64, {}, "tower_resident_f16+heads", 2, 5),
    ("chess256-f16-nb1", "chess_2x256_att", F16, 64, {"KZ_TOWER_NB": "1"}, "tower_resident_f16+heads", 1, 3),
    ("chess256-f16-nb2-nofuse", "chess_2x256_att", F16, 64, NOFUSE, "tower_resident_f16", 2, 5),
    ("chess256-f16-nb1-nofuse", "chess_2x256_att", F16, 64, dict(NOFUSE, KZ_TOWER_NB="1"), "tower_resident_f16", 1, 3),
    ("chesshist1-f16", "chesshist1_1x256_att", F16, 64, {}, "tower_resident_f16+heads", 2, 5),   # 34 planes: the wide stem, two chunks
    ("chesshist3-f16", "chesshist3_1x256_att", F16, 64, {}, "tower_resident_f16+heads", 2, 5),   # 60 planes
    # the other arithmetics on the chess network
    ("chess256-split16", "chess_2x256_att", SPLIT, 64, {}, "tower_resident_split16+heads", 1, 9),
    ("chess256-split16-nofuse", "chess_2x256_att", SPLIT, 64, NOFUSE, "tower_resident_split16", 1, 9),
    ("chess256-f32", "chess_2x256_att", F32, 64, {}, "tower_resident_f32", 1, 9),
    # kz_tower_pairs.hpp in plain f16 and in split arithmetic
    ("chess128-f16g-1", "chess_1x128_att", F16, 64, {}, "tower_resident_f16g", 1, 3),
    ("chess128-f16g-2", "chess_1x128_att", F16, 256, {}, "tower_resident_f16g", 2, 255),
    ("chess128-f16g-4", "chess_1x128_att", F16, 2048, {}, "tower_resident_f16g", 4, 2045),
    ("chess128-split16", "chess_1x128_att", SPLIT, 64, {}, "tower_resident_split16", 1, 9),
    ("chess192-f16g-2", "chess_1x192_att", F16, 256, {}, "tower_resident_f16g", 2, 255),
    ("chess192-split16", "chess_1x192_att", SPLIT, 64, {}, "tower_resident_split16", 1, 9),
    ("ataxx7x128-f16g-2", "ataxx7_1x128", F16, 64, {}, "tower_resident_f16g+heads", 2, 5),
    ("ataxx7x128-f16g-4", "ataxx7_1x128", F16, 512, {}, "tower_resident_f16g+heads", 4, 509),
    ("ataxx7x128-split16", "ataxx7_1x128", SPLIT, 64, {}, "tower_resident_split16+heads", 2, 9),
    ("ataxx5x128-f16g", "ataxx5_1x128", F16, 64, {}, "tower_resident_f16g+heads", 4, 9),
    ("ataxx5x128-split16", "ataxx5_1x128", SPLIT, 64, {}, "tower_resident_split16+heads", 4, 9),
    ("go9x128-f16g-1", "go9_1x128", F16, 64, {}, "tower_resident_f16g+heads", 1, 3),
    ("go9x128-f16g-2", "go9_1x128", F16, 256, {}, "tower_resident_f16g+heads", 2, 255),
    ("go9x128-f16g-3", "go9_1x128", F16, 2048, {}, "tower_resident_f16g+heads", 3, 1534),
    ("go9x128-split16", "go9_1x128", SPLIT, 64, {}, "tower_resident_split16+heads", 1, 9),
    ("go9x256-f16g", "go9_1x256", F16, 64, {}, "tower_resident_f16g", 1, 9),
    ("ataxx7x64-f16g", "ataxx7_1x64", F16, 64, {}, "tower_resident_f16g", 2, 9),
    ("ataxx7x64-split16", "ataxx7_1x64", SPLIT, 64, {}, "tower_resident_split16", 2, 9),
    ("chess512-f16g", "chess_1x512_att", F16, 64, {}, "tower_resident_f16g", 1, 9),
    # the exact-f32 launch with the conv heads inside
    ("ataxx7x128-f32", "ataxx7_1x128", F32, 64, {}, "tower_resident_f32+heads", 2, 9),
    ("go9x128-f32", "go9_1x128", F32, 64, {}, "tower_resident_f32+heads", 1, 9),
    ("ataxx6x128-sh96-f32", "ataxx6_1x128_sh96", F32, 64, {}, "tower_resident_f32+heads", 3, 10),  # boards x hidden units > threads
    # the board-tile kernel, both instances
    ("go19x64-board-f16", "go19_1x64", F16, 256, {}, "board_conv_f16", None, 9),
    ("go19x64-board-split16", "go19_1x64", SPLIT, 256, {}, "board_conv_split16", None, 9),
    ("go19x128-board-f16", "go19_1x128", F16, 256, {}, "board_conv_f16", None, 9),               # two output-channel quarters
    ("go19x128-board-split16", "go19_1x128", SPLIT, 256, {}, "board_conv_split16", None, 9),     # ... in split arithmetic
    ("go13x128-f16g", "go13_1x128", F16, 64, {}, "tower_resident_f16g+heads", 1, 9),          # (where the table sends 13x13)
    ("go13x128-board-f16", "go13_1x128", F16, 256, {"KZ_NO_RESIDENT_F16G": "1"}, "board_conv_f16", None, 9),
    # the generic per-layer path
    ("chess256x1-igemm-f16", "chess_1x256_att", F16, 64, GENERIC, "conv_igemm_f16", None, 9),
    ("chess256x1-igemm-f32", "chess_1x256_att", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
    ("go9x96-igemm-f16", "go9_1x96", F16, 64, GENERIC, "conv_igemm_f16", None, 9),
    ("go9x96-igemm-f32", "go9_1x96", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
    ("ataxx7x48-igemm-f16", "ataxx7_1x48", F16, 64, GENERIC, "conv_igemm_f16", None, 9),          # channels no multiple of 32
    ("ataxx7x48-igemm-f32", "ataxx7_1x48", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
    ("go9x128-nof16g-f16", "go9_1x128", F16, 64, {"KZ_NO_RESIDENT_F16G": "1"}, "conv_igemm_f16", None, 9),
    # the generic heads, one network per policy head kind
    ("chess128-dense-f16", "chess_1x128_dense", F16, 64, GENERIC, "conv_igemm_f16", None, 9),
    ("chess128-dense-f32", "chess_1x128_dense", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
    ("arimaa96-f16", "arimaa_1x96", F16, 64, GENERIC, "conv_igemm_f16", None, 9),
    ("arimaa96-f32", "arimaa_1x96", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
    ("ttt32-dense-f16", "ttt_1x32_dense", F16, 64, GENERIC, "conv_igemm_f16", None, 9),
    ("ttt32-dense-f32", "ttt_1x32_dense", F32, 64, GENERIC, "conv_igemm_f32", None, 9),
]

# (ordered by network and position: exact_nets.build keeps the last few models, every engine of one model runs in a row)
CASES = [(e, pos) for net in E.NETS for pos in E.positions(net) for e in ENGINES if e[1] == net]
IDS = [f"{e[0]}-{'none' if pos is None else pos}" for e, pos in CASES]


# The wide family (tests/exact_nets.py: lo halves that are not zero): every split16 engine, and every exact-f32 engine of the same
# networks — the cross-check that the network is exact, not the kernel lenient.  The f16 engines do not run it.
WIDE_CASES = [(e, wide) for net in E.WIDE_NETS for wide in E.wide_positions(net) for e in ENGINES if e[1] == net and e[2] in (SPLIT, F32)]
WIDE_IDS = [f"{e[0]}-{E.wide_id(wide)}" for e, wide in WIDE_CASES]


def make_engine(model, dev, max_batch, dtype, switches):
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        return capi.Engine(model, dev, max_batch, dtype)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def mismatch(out, ref, hw):
    """Where two tensors differ: boards, and for a per-square policy the squares — the pattern locates the fault."""
    bad = np.argwhere(out != ref)
    boards = sorted(set(int(b) for b in bad[:, 0]))
    cols = sorted(set(int(c) for c in bad[:, 1]))
    worst = float(np.abs(out.astype(np.float64) - ref).max())
    return (f"{len(bad)} of {out.size} differ, max |d| {worst:g}; boards {boards[:12]}{'...' if len(boards) > 12 else ''}; "
            f"columns {cols[:12]}{'...' if len(cols) > 12 else ''} (columns mod {hw}: {sorted(set(c % hw for c in cols))[:12]})")


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("engine,pos", CASES, ids=IDS)
def test_engine_returns_the_reference_bits(dev, engine, pos):
    returns_the_reference_bits(dev, engine, E.build(engine[1], pos), f"dense_at={pos}")


@pytest.mark.gpu
@pytest.mark.parametrize("engine,wide", WIDE_CASES, ids=WIDE_IDS)
def test_engine_returns_the_reference_bits_on_a_wide_network(dev, engine, wide):
    """Activations or weights with lo halves that are not zero: a lo fragment read from the wrong board, tap, chunk, tile
    or ring stage changes the bits."""
    returns_the_reference_bits(dev, engine, E.build(engine[1], None, wide), E.wide_id(wide))


def returns_the_reference_bits(dev, engine, b, label):
    name, net, dtype, max_batch, switches, path, per, batch = engine
    eng = make_engine(capi.Model(blob=b.blob), dev, max_batch, dtype, switches)
    assert eng.tower_path == path
    geometry = eng.launch_geometry(batch)
    print(f"[exact] {name} {label}: {eng.tower_path}, {batch} boards in {geometry[0]} workgroups of {geometry[1]}")
    if per is not None:
        assert geometry == ((batch + per - 1) // per, per)
        assert batch % per == 1 or per == 1, "ragged: the last workgroup holds one board"
    hw = b.meta["board_h"] * b.meta["board_w"]
    # the ragged launch (thirteen distinct boards, repeated from the fourth on so that no workgroup starts the cycle), then one board alone
    for idx in (np.arange(3, 3 + batch) % E.BOARDS, np.array([E.BOARDS - 1])):
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        assert np.array_equal(s, b.ref_scalars[idx]), "scalars: " + mismatch(s, b.ref_scalars[idx], 5)
        assert np.array_equal(p, b.ref_policy[idx]), "policy: " + mismatch(p, b.ref_policy[idx], hw)


@pytest.mark.gpu
def test_one_process_runs_both_chess_instances_in_either_order(dev):
    """KZ_TOWER_NB is read per engine: 2, 1, 2 boards per workgroup in one process, each exact."""
    b = E.build("chess_2x256_att", 2)
    model = capi.Model(blob=b.blob)
    for nb, want in (("2", (19, 2)), ("1", (37, 1)), ("2", (19, 2)), (None, (19, 2))):
        eng = make_engine(model, dev, 64, F16, {} if nb is None else {"KZ_TOWER_NB": nb})
        assert eng.tower_path == "tower_resident_f16+heads" and eng.launch_geometry(37) == want
        idx = np.arange(37) % E.BOARDS
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        assert np.array_equal(s, b.ref_scalars[idx]) and np.array_equal(p, b.ref_policy[idx])


@pytest.mark.gpu
def test_the_split_1x1_kernel_is_among_the_exact_cases(dev):
    """kz_conv1x1_split (the f16 / split engines' 1x1 head convolutions where the plan sends them through it) is reached by
    the cases above: at least one of them launches it, by its profiled kernel name — and in split arithmetic on a wide
    network whose tower output carries lo halves (the stem's weights wide)."""
    reached = []
    for name, net, dtype, max_batch, switches, path, _, _ in ENGINES:
        if dtype == F32 or path.endswith("+heads"):
            continue
        wide = next(w for w in E.wide_positions(net) if w[0] == 0) if dtype == SPLIT else None
        b = E.build(net, None, wide)
        if wide is not None:
            heads = [p for p in b.layers if not p.startswith("common.") and b.tensors[p + ".weight"].ndim == 4]
            assert heads and all(b.report.lo_in[p][0] >= E.LIVE_SHARE and b.report.lo_in[p][1] for p in heads)
        eng = make_engine(capi.Model(blob=b.blob), dev, max_batch, dtype, switches)
        eng.set_profiling(True)
        s, p = eng.eval_packed(b.bits[:3], b.scalars_in[:3])
        _, launches = eng.kernel_time("kz_conv1x1_split")
        eng.set_profiling(False)
        assert np.array_equal(s, b.ref_scalars[:3]) and np.array_equal(p, b.ref_policy[:3]), name
        if launches:
            reached.append((name, wide))
    print(f"[exact] kz_conv1x1_split runs in: {reached}")
    assert reached
    assert any(wide is not None for _, wide in reached), "no wide network reaches kz_conv1x1_split"
