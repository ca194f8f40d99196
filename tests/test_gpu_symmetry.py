"""Board symmetries inside the launch (kz_engine_set_symmetries + the `_sym` decoded entries, include/kz_hip.h): the
reference's RandomSymmetryNetwork (rust/kz-core/src/network/symmetry.rs:18-68,126-148) as two permutations done by the
launch — the bool planes on the way in (kz_encode_dev.hpp), the policy indices on the way out (kz_decode_dev.hpp).

The yardstick is the HOST route through the existing entry: the mapped inputs are built here in numpy (planes permuted and
re-packed, move indices mapped, move order kept) and go through submit_packed_decoded; the new entry gets the original inputs
plus one id per board.  Both run the same kernels on the same planes and sum in the same order, so values and probabilities
must be np.array_equal — no tolerance.  The 2 x 128 Ataxx networks are additionally held to the oracle at the project's stated
bounds for the decoded boundary (tests/test_gpu_parity.py)."""
import os

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O
from tests.test_gpu_parity import F16_PROB_ATOL, F16_VALUE_ATOL, F32_ATOL, assert_f16, assert_f32

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F16, F32, SPLIT16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


# ---- tables -------------------------------------------------------------------------------------------------------------
def ataxx_tables(size):
    """The reference's own tables (tests/golden/ataxx_symmetry.txt: size index transpose flip_x flip_y n map_mv[0..n)): a row
    is policy_map; its first `area` entries (the copy moves) say where tile i lands, square_src is that map's inverse."""
    area = size * size
    rows = [ln.split() for ln in open(os.path.join(GOLDEN, "ataxx_symmetry.txt")) if ln.split()[0] == str(size)]
    assert [int(r[1]) for r in rows] == list(range(8))
    policy_map = np.array([[int(v) for v in r[6:]] for r in rows], np.int32)
    assert policy_map.shape == (8, 17 * area + 1)
    square_src = np.empty((8, area), np.int32)
    for s in range(8):
        square_src[s, policy_map[s, :area]] = np.arange(area)
    return square_src, policy_map


def go_tables(size):
    """D4 of the Go grid from the formula (transpose, then flip x, then flip y: board-game's D4Symmetry, index = 4 transpose +
    2 flip_x + flip_y): tile (x, y) lands on its image, policy index 0 (pass) is fixed, 1 + tile maps with the tile."""
    area = size * size
    square_src = np.empty((8, area), np.int32)
    policy_map = np.empty((8, 1 + area), np.int32)
    for s in range(8):
        policy_map[s, 0] = 0
        for y in range(size):
            for x in range(size):
                nx, ny = (y, x) if s & 4 else (x, y)
                if s & 2:
                    nx = size - 1 - nx
                if s & 1:
                    ny = size - 1 - ny
                square_src[s, ny * size + nx] = y * size + x
                policy_map[s, 1 + y * size + x] = 1 + ny * size + nx
    return square_src, policy_map


def synthetic_tables(hw, policy_len, n_sym, seed):
    """Chess has no symmetry, but the mechanism is a pair of tables: seeded random permutations of the squares and of the
    policy indices."""
    rng = np.random.default_rng(seed)
    return (np.stack([rng.permutation(hw) for _ in range(n_sym)]).astype(np.int32),
            np.stack([rng.permutation(policy_len) for _ in range(n_sym)]).astype(np.int32))


# ---- the host route -----------------------------------------------------------------------------------------------------
def map_bits(bits, n_bool, hw, square_src, ids):
    """plane'[s'] = plane[square_src[id][s']] on the unpacked BitBuffer bits (LSB-first), packed again."""
    planes = np.unpackbits(bits, axis=1, bitorder="little")[:, :n_bool * hw].reshape(len(bits), n_bool, hw)
    mapped = np.stack([planes[b][:, square_src[ids[b]]] for b in range(len(bits))])
    out = np.packbits(mapped.reshape(len(bits), -1), axis=1, bitorder="little")
    assert out.shape == bits.shape
    return out


def map_moves(moves, policy_map, ids):
    return [policy_map[ids[b]][m].astype(np.int32) for b, m in enumerate(moves)]


def move_lists(rng, valid, batch, finished):
    """Distinct valid policy indices in arbitrary order, 1..60 per board; board `finished` has none (a finished game)."""
    lists = [rng.permutation(valid)[:int(n)].astype(np.int32) for n in rng.integers(1, min(len(valid), 61), size=batch)]
    lists[finished] = np.zeros(0, np.int32)
    return lists


class Case:
    def __init__(self, dev, game, depth, channels, head, dtype, path, max_batch, tables=None, seed=5, **model_kw):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed, **model_kw)
        self.game, self.hw, self.n_bool, self.n_scalar, self.policy_len = game, g["size"] ** 2, g["n_bool"], g["n_scalar"], g["policy_len"]
        self.eng = capi.Engine(capi.Model(blob=self.blob), dev, max_batch, dtype)
        assert self.eng.tower_path == path
        if tables == "ataxx":
            tables = ataxx_tables(g["size"])
        elif tables == "go":
            tables = go_tables(g["size"])
        elif tables is None:
            tables = synthetic_tables(self.hw, self.policy_len, 3, seed=77)
        self.square_src, self.policy_map = tables
        self.n_sym = len(self.square_src)
        self.valid = np.flatnonzero(self.policy_map[0] >= 0)  # (an off-board Ataxx jump is off-board under every symmetry)
        self.eng.set_symmetries(self.square_src, self.policy_map)

    def inputs(self, batch, seed):
        rng = np.random.default_rng(seed)
        bits, scalars = synth.random_boards(self.game, batch, seed=seed)
        ids = np.concatenate([np.arange(self.n_sym), rng.integers(0, self.n_sym, size=batch)])[:batch].astype(np.uint8)
        ids = ids[rng.permutation(batch)]  # every symmetry occurs, anywhere in the batch
        return bits, scalars, move_lists(rng, self.valid, batch, finished=int(rng.integers(0, batch))), ids

    def mapped(self, bits, moves, ids):
        return map_bits(bits, self.n_bool, self.hw, self.square_src, ids), map_moves(moves, self.policy_map, ids)

    def check(self, batch, seed, slot=0):
        """The new entry on the original inputs + ids == the existing entry on the mapped inputs, bit for bit."""
        bits, scalars, moves, ids = self.inputs(batch, seed)
        assert len(set(ids.tolist())) == self.n_sym and any(m.size == 0 for m in moves)
        m_bits, m_moves = self.mapped(bits, moves, ids)
        v_ref, p_ref = self.eng.wait_decoded(slot, self.eng.submit_packed_decoded(slot, m_bits, scalars, m_moves))
        v, p = self.eng.wait_decoded(slot, self.eng.submit_packed_decoded(slot, bits, scalars, moves, sym=ids))
        assert np.array_equal(v, v_ref)
        assert len(p) == batch and all(np.array_equal(a, b) for a, b in zip(p, p_ref))
        assert all(a.shape == m.shape for a, m in zip(p, moves))
        if np.any(ids != 0):  # (the symmetry does something: the unmapped evaluation differs)
            v0, _ = self.eng.wait_decoded(slot, self.eng.submit_packed_decoded(slot, bits, scalars, moves))
            assert not np.array_equal(v0, v)
        return bits, scalars, moves, ids, v, p


def against_oracle(case, dtype, bits, scalars, moves, ids, v, p):
    """OracleNet.forward on the mapped planes, O.decode_output with the mapped lists: the decoded boundary's stated bounds."""
    net = O.OracleNet(case.blob)
    m_bits, m_moves = case.mapped(bits, moves, ids)
    s_ora, p_ora = net.forward(O.encode_input_full(m_bits, scalars, net.n_scalar, net.n_bool, net.h, net.w))
    v_ora, probs_ora = O.decode_output(s_ora, p_ora, m_moves)
    worst_p = max(float(np.abs(a - b).max()) for a, b in zip(p, probs_ora) if a.size)
    worst_v = float(np.abs(v[:, :4] - v_ora[:, :4]).max())
    print(f"[symmetry vs oracle, {case.eng.tower_path}] max |dprob| {worst_p:.2e}, max |dvalue, dwdl| {worst_v:.2e}")
    if dtype == F16:
        assert worst_p <= F16_PROB_ATOL and worst_v <= F16_VALUE_ATOL
        assert_f16(v[:, 4:], v_ora[:, 4:], "moves_left")  # a raw network output: the logit tolerance
    else:
        assert worst_p <= F32_ATOL and worst_v <= F32_ATOL
        assert_f32(v[:, 4:], v_ora[:, 4:], "moves_left")


# ---- Ataxx 7x7 with the reference's own tables --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", [(F16, "tower_resident_f16g+heads"), (F32, "tower_resident_f32+heads"),
                                        (SPLIT16, "tower_resident_split16+heads")], ids=["f16", "f32", "split16"])
def test_ataxx_2x128_one_launch_paths_and_oracle(dev, dtype, path):
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", dtype, path, 64, tables="ataxx")
    against_oracle(case, dtype, *case.check(37, seed=11))


def test_ataxx_2x64_heads_and_decode_as_separate_launches(dev):
    """tower_resident_f16g without fused heads: the launch's own encode, then the stand-alone kz_decode_output."""
    Case(dev, "ataxx-7", 2, 64, "ataxx_conv", F16, "tower_resident_f16g", 64, tables="ataxx").check(37, seed=12)


def test_ataxx_2x64_per_layer_path_stand_alone_encode(dev, monkeypatch):
    """KZ_FORCE_GENERIC=1: the stand-alone kz_encode_packed in front of the per-layer convolutions."""
    monkeypatch.setenv("KZ_FORCE_GENERIC", "1")
    Case(dev, "ataxx-7", 2, 64, "ataxx_conv", F16, "conv_igemm_f16", 64, tables="ataxx").check(37, seed=13)


def test_ataxx_2x128_several_boards_per_workgroup(dev):
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", 512, tables="ataxx")
    wgs, per = case.eng.launch_geometry(203)
    assert per > 1 and wgs > 1
    case.check(203, seed=14)


# ---- Go 9x9, tables from the formula ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", [(F16, "tower_resident_f16g+heads"), (SPLIT16, "tower_resident_split16+heads")],
                         ids=["f16", "split16"])
def test_go9_2x128(dev, dtype, path):
    case = Case(dev, "go-9", 2, 128, "conv", dtype, path, 64, tables="go")
    assert np.all(case.policy_map[:, 0] == 0)  # pass is index 0 and every symmetry fixes it
    _, _, moves, _, _, _ = case.check(37, seed=21)
    assert any(0 in m for m in moves)


# ---- chess: no symmetry of its own, three synthetic ones ----------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", [(F16, "tower_resident_f16+heads"), (SPLIT16, "tower_resident_split16+heads")],
                         ids=["f16", "split16"])
def test_chess_2x256_attention_head_on_all_slots(dev, dtype, path):
    case = Case(dev, "chess", 2, 256, "attention", dtype, path, 64)
    eng = case.eng
    # all four slots in flight with different ids, waited out of order; the references afterwards, slot by slot
    batches = [case.inputs(37 - 3 * k, seed=30 + k) for k in range(capi.KZ_ENGINE_SLOTS)]
    offs = [eng.submit_packed_decoded(k, b[0], b[1], b[2], sym=b[3]) for k, b in enumerate(batches)]
    got = {k: eng.wait_decoded(k, offs[k]) for k in (2, 0, 3, 1)}
    for k, (bits, scalars, moves, ids) in enumerate(batches):
        m_bits, m_moves = case.mapped(bits, moves, ids)
        v_ref, p_ref = eng.wait_decoded(k, eng.submit_packed_decoded(k, m_bits, scalars, m_moves))
        assert np.array_equal(got[k][0], v_ref) and all(np.array_equal(a, b) for a, b in zip(got[k][1], p_ref))
    case.check(37, seed=35)


@pytest.mark.parametrize("dtype,path", [(F16, "tower_resident_f16+heads"), (SPLIT16, "tower_resident_split16+heads")],
                         ids=["f16", "split16"])
def test_chess_2x256_two_boards_per_workgroup_one_odd_board(dev, dtype, path):
    Case(dev, "chess", 2, 256, "attention", dtype, path, 256).check(201, seed=36)


@pytest.mark.parametrize("dtype,path", [(F16, "attention_tower_f16"), (F32, "attention_tower_f32")], ids=["f16", "f32"])
def test_attention_tower_chess_2x128(dev, dtype, path):
    """kz_att_tower_mfma's encode (the heads and the decode are separate launches)."""
    Case(dev, "chess", 2, 128, "dense", dtype, path, 256, attention=(8, 16, 16, 128)).check(201, seed=41)


# ---- identity -----------------------------------------------------------------------------------------------------------
def test_identity_tables_and_no_ids_are_the_existing_entry(dev):
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", 64,
                tables=(np.arange(49, dtype=np.int32)[None], np.arange(17 * 49 + 1, dtype=np.int32)[None]))
    eng = case.eng
    bits, scalars, moves, _ = case.inputs(37, seed=51)
    v_ref, p_ref = eng.wait_decoded(0, eng.submit_packed_decoded(0, bits, scalars, moves))
    for sym in (np.zeros(37, np.uint8), None):
        v, p = eng.wait_decoded(1, eng.submit_packed_decoded(1, bits, scalars, moves, sym=sym))
        assert np.array_equal(v, v_ref) and all(np.array_equal(a, b) for a, b in zip(p, p_ref))
        v, p = eng.eval_packed_decoded(bits, scalars, moves, sym=sym)
        assert np.array_equal(v, v_ref) and all(np.array_equal(a, b) for a, b in zip(p, p_ref))


# ---- errors: a message each, no device fault, and the engine evaluates correctly afterwards -----------------------------
@pytest.mark.parametrize("channels,path", [(128, "tower_resident_f16g+heads"), (64, "tower_resident_f16g")],
                         ids=["decode_in_launch", "decode_kernel"])
def test_errors(dev, channels, path):
    g = synth.game_spec("ataxx-7")
    blob = synth.random_model("ataxx-7", 2, channels, "ataxx_conv", seed=5)
    eng = capi.Engine(capi.Model(blob=blob), dev, 64, F16)
    assert eng.tower_path == path
    square_src, policy_map = ataxx_tables(7)
    valid = np.flatnonzero(policy_map[0] >= 0)
    rng = np.random.default_rng(61)
    bits, scalars = synth.random_boards("ataxx-7", 37, seed=61)
    moves = move_lists(rng, valid, 37, finished=4)
    ids = rng.integers(0, 8, size=37).astype(np.uint8)

    def good():
        m_bits = map_bits(bits, g["n_bool"], 49, square_src, ids)
        v_ref, p_ref = eng.wait_decoded(0, eng.submit_packed_decoded(0, m_bits, scalars, map_moves(moves, policy_map, ids)))
        v, p = eng.wait_decoded(2, eng.submit_packed_decoded(2, bits, scalars, moves, sym=ids))
        assert np.array_equal(v, v_ref) and all(np.array_equal(a, b) for a, b in zip(p, p_ref))

    # ids before any tables are set
    with pytest.raises(capi.KzError, match="no tables set"):
        eng.submit_packed_decoded(0, bits, scalars, moves, sym=ids)
    with pytest.raises(capi.KzError, match="no tables set"):
        eng.eval_packed_decoded(bits, scalars, moves, sym=ids)
    # tables the library must refuse
    h = capi.load()
    not_a_permutation = square_src.copy()
    not_a_permutation[3, 10] = not_a_permutation[3, 11]
    with pytest.raises(capi.KzError, match="not a permutation"):
        eng.set_symmetries(not_a_permutation, policy_map)
    with pytest.raises(capi.KzError, match="n_sym"):
        capi.check(h.kz_engine_set_symmetries(eng._h, 0, square_src.ctypes.data, policy_map.ctypes.data))
    with pytest.raises(capi.KzError, match="n_sym"):
        capi.check(h.kz_engine_set_symmetries(eng._h, 256, square_src.ctypes.data, policy_map.ctypes.data))
    too_large = policy_map.copy()
    too_large[7, 100] = policy_map.shape[1]
    with pytest.raises(capi.KzError, match="policy_map"):
        eng.set_symmetries(square_src, too_large)
    with pytest.raises(capi.KzError, match="no tables set"):  # (a refused call has set nothing)
        eng.submit_packed_decoded(0, bits, scalars, moves, sym=ids)
    eng.set_symmetries(square_src, policy_map)
    good()
    # a batch in flight: the tables cannot change under it
    off = eng.submit_packed_decoded(1, bits, scalars, moves, sym=ids)
    with pytest.raises(capi.KzError, match="in flight"):
        eng.set_symmetries(square_src, policy_map)
    eng.wait_decoded(1, off)
    # an id equal to n_sym (clamped for the reads): on a board with moves, and on the finished one
    for board in (20, 4):
        bad = ids.copy()
        bad[board] = 8
        off = eng.submit_packed_decoded(1, bits, scalars, moves, sym=bad)
        with pytest.raises(capi.KzError, match="symmetry id"):
            eng.wait_decoded(1, off)
    good()
    # a listed move whose policy_map entry is -1 (a jump from off the board)
    gone = [m.copy() for m in moves]
    gone[36][0] = np.flatnonzero(policy_map[0] < 0)[0]
    off = eng.submit_packed_decoded(3, bits, scalars, gone, sym=ids)
    with pytest.raises(capi.KzError, match="no image under"):
        eng.wait_decoded(3, off)
    good()
    # the tables may be replaced while nothing is in flight: fewer symmetries, then id 3 is out of range
    eng.set_symmetries(square_src[:3], policy_map[:3])
    off = eng.submit_packed_decoded(1, bits, scalars, moves, sym=np.full(37, 3, np.uint8))
    with pytest.raises(capi.KzError, match="symmetry id"):
        eng.wait_decoded(1, off)
    eng.set_symmetries(square_src, policy_map)
    good()
