"""Per-board status and the exact-f32 range fallback (include/kz_hip.h: KZ_BOARD_*, kz_engine_wait_decoded_status,
kz_engine_eval_packed_decoded_status, kz_engine_set_range_fallback).

Every case is the smallest network that reaches one family of flag sites (the path name is asserted), with a ragged batch of
37 boards: with two or three boards per workgroup an odd board is left over.  The range cause is scalars_in[b, 0] = 3e5 on
boards {0, 5, 36}: finite in f32, inf as f16, so it reaches every f16 / split16 range check through the stem while the oracle
and the exact-f32 engine stay finite (asserted on the CPU first).  The decode causes sit on three other boards: a move index
equal to policy_len, a symmetry id equal to n_sym, a listed move whose policy_map entry is -1.

Bounds.  Results of boards with status 0 are compared with np.array_equal to the same engine's results on the batch whose bad
boards were replaced by benign ones; fell-back boards with np.array_equal to a separate KZ_DTYPE_F32 engine.  Against the
oracle's decode the fell-back boards are held to the project's 1e-4 (tests/test_gpu_parity.py: F32_ATOL) on everything
decode_output bounds — tanh(value), the wdl softmax, the move probabilities.  moves_left passes through the decode raw, and with
a scalar plane of 3e5 it is of order 1e4 (Ataxx 3 x 128: 2.0e4), where two neighbouring f32 numbers are 2e-3 apart: an absolute
1e-4 is not representable there, so it is held to 1e-4 of max(1, |reference|), the same bound at the scale of the number."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O
from tests.test_gpu_parity import F32_ATOL
from tests.test_gpu_symmetry import ataxx_tables, map_bits, map_moves, move_lists, synthetic_tables

pytestmark = pytest.mark.gpu

F16, F32, SPLIT16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
OK, BAD_DECODE, NONFINITE, FELL_BACK = capi.KZ_BOARD_OK, capi.KZ_BOARD_BAD_DECODE, capi.KZ_BOARD_NONFINITE, capi.KZ_BOARD_FELL_BACK
BATCH = 37
RANGE = [0, 5, 36]
B_INDEX, B_ID, B_HOLE = 3, 7, 20  # the three decode causes
DECODE = [B_INDEX, B_ID, B_HOLE]
NONFINITE_MSG, SOFTMAX_MSG = "non-finite activation", "Softmax input sum must be strictly positive"


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Case:
    """A network, an engine of `dtype` on the asserted path, three synthetic symmetries (seeded permutations; policy_map[1] has
    one hole) and two batches of 37 boards: `clean`, and `bad` = clean with the range and decode causes planted."""

    def __init__(self, dev, game, depth, channels, head, dtype, path, max_batch=64, seed=5, **model_kw):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed, **model_kw)
        self.game, self.hw, self.n_bool, self.policy_len = game, g["size"] ** 2, g["n_bool"], g["policy_len"]
        self.model = capi.Model(blob=self.blob)
        self.dev, self.dtype = dev, dtype
        self.eng = capi.Engine(self.model, dev, max_batch, dtype)
        assert self.eng.tower_path == path
        self.square_src, self.policy_map = synthetic_tables(self.hw, self.policy_len, 3, seed=77)
        self.hole = 11
        self.policy_map[1, self.hole] = -1
        self.n_sym = 3
        self.eng.set_symmetries(self.square_src, self.policy_map)
        valid = np.array([i for i in range(self.policy_len) if i != self.hole])
        rng = np.random.default_rng(seed + 100)
        self.bits, self.scalars = synth.random_boards(game, BATCH, seed=seed + 1)
        assert self.scalars.shape[1] >= 1
        self.moves = move_lists(rng, valid, BATCH, finished=10)
        self.ids = rng.integers(0, self.n_sym, size=BATCH).astype(np.uint8)
        self.ids[RANGE] = [1, 2, 1]  # the range boards under non-identity ids (no synthetic row is the identity)
        # the causes
        self.scalars_bad = self.scalars.copy()
        self.scalars_bad[RANGE, 0] = np.inf if dtype == F32 else 3e5
        self.moves_bad = [m.copy() for m in self.moves]
        self.moves_bad[B_INDEX][0] = self.policy_len
        self.moves_bad[B_HOLE][0] = self.hole
        self.ids_bad = self.ids.copy()
        self.ids_bad[B_ID] = self.n_sym
        self.ids_bad[B_HOLE] = 1
        self.ids_hole = self.ids.copy()  # (the benign batch keeps board B_HOLE's id: only its move changes)
        self.ids_hole[B_HOLE] = 1

    def decoded(self, eng, slot, scalars, moves, ids, status=False):
        off = eng.submit_packed_decoded(slot, self.bits, scalars, moves, sym=ids)
        return eng.wait_decoded_status(slot, off) if status else eng.wait_decoded(slot, off)

    def oracle_decode(self, boards):
        """O.decode_output of the oracle's forward pass on the mapped boards `boards` of the bad batch (range causes only)."""
        net = O.OracleNet(self.blob)
        ids = self.ids[boards]
        m_bits = map_bits(self.bits[boards], self.n_bool, self.hw, self.square_src, ids)
        m_moves = map_moves([self.moves[b] for b in boards], self.policy_map, ids)
        s, p = net.forward(O.encode_input_full(m_bits, self.scalars_bad[boards], net.n_scalar, net.n_bool, net.h, net.w))
        assert np.isfinite(s).all() and np.isfinite(p).all(), "the oracle must be finite on the range boards"
        return O.decode_output(s, p, m_moves)


def same_board(a, b, board):
    return np.array_equal(a[0][board], b[0][board]) and np.array_equal(a[1][board], b[1][board])


CASES = [
    ("ataxx-7", 3, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", {}, {}, 64),
    ("ataxx-7", 3, 128, "ataxx_conv", SPLIT16, "tower_resident_split16+heads", {}, {}, 64),
    ("chess", 2, 256, "attention", F16, "tower_resident_f16+heads", {}, {}, 64),
    ("chess", 2, 256, "attention", SPLIT16, "tower_resident_split16+heads", {}, {}, 64),
    ("chess", 2, 256, "attention", F16, "tower_resident_f16", {"KZ_NO_FUSED_HEADS": "1"}, {}, 64),  # + kz_att_heads
    ("go-9", 2, 64, "conv", F16, "tower_resident_f16g", {}, {}, 64),  # kz_scalar_head, stand-alone kz_decode_output
    # (the board-tile kernel wants a batch that fills the chip: an engine of 256 for the same 37 boards)
    ("go-19", 1, 64, "conv", F16, "board_conv_f16", {}, {}, 256),
    ("chess", 2, 64, "attention", F16, "conv_igemm_f16", {"KZ_FORCE_GENERIC": "1"}, {}, 64),
    ("chess", 2, 128, "dense", F16, "attention_tower_f16", {}, {"attention": (8, 16, 16, 128)}, 64),
    ("go-9", 2, 100, "none", F16, "dense_network_f32", {}, {"dense_network": True}, 64),  # (the sweep's DenseNetwork with scalar planes)
]
IDS = ["ataxx_f16", "ataxx_split16", "chess_f16", "chess_split16", "chess_f16_att_heads", "go9_f16_decode_kernel", "go19_board_conv",
       "chess_generic", "attention_tower_f16", "dense_network"]


@pytest.mark.parametrize("game,depth,channels,head,dtype,path,env,model_kw,max_batch", CASES, ids=IDS)
def test_status_and_range_fallback(dev, monkeypatch, game, depth, channels, head, dtype, path, env, model_kw, max_batch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = Case(dev, game, depth, channels, head, dtype, path, max_batch, **model_kw)
    eng = c.eng
    v_ora, p_ora = c.oracle_decode(RANGE)  # (asserts the oracle finite on them, before anything runs on the GPU)

    # ---- fallback off: the status names the boards, nobody else is disturbed, the old entries fail as they always did ----
    bad = c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad, status=True)
    st = bad[2]
    print(f"[{eng.tower_path}] status {st.tolist()}")
    assert st.dtype == np.uint8 and st.shape == (BATCH,)
    assert sorted(np.flatnonzero(st).tolist()) == sorted(RANGE + DECODE)
    assert all(st[b] & NONFINITE and not st[b] & FELL_BACK for b in RANGE)  # (usually 1 | 2: the softmax sum is NaN too)
    assert all(st[b] == BAD_DECODE for b in DECODE)
    # the same slot, a clean batch next: no status word survives (and this is the benign batch of the comparison)
    clean = c.decoded(eng, 0, c.scalars, c.moves, c.ids_hole, status=True)
    assert not clean[2].any()
    assert all(same_board(clean, c.decoded(eng, 1, c.scalars, c.moves, c.ids_hole), b) for b in range(BATCH))
    good = [b for b in range(BATCH) if st[b] == OK]
    assert all(same_board(bad, clean, b) for b in good)
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad)
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        eng.eval_packed_decoded(c.bits, c.scalars_bad, c.moves, sym=c.ids)
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        eng.eval_packed(c.bits, c.scalars_bad)
    with pytest.raises(capi.KzError, match=SOFTMAX_MSG):
        c.decoded(eng, 2, c.scalars, c.moves_bad, c.ids_bad)
    # the synchronous status entry, without ids (sym == NULL): the range boards and the move index
    _, _, st_plain = eng.eval_packed_decoded_status(c.bits, c.scalars_bad, c.moves_bad)
    assert sorted(np.flatnonzero(st_plain).tolist()) == sorted(RANGE + [B_INDEX]) and st_plain[B_INDEX] == BAD_DECODE

    # ---- all four slots in flight, different bad boards per slot: each slot reports its own ----
    offs = []
    for k in range(capi.KZ_ENGINE_SLOTS):
        scalars, moves = c.scalars.copy(), [m.copy() for m in c.moves]
        scalars[k + 1, 0] = 3e5
        moves[20 + k][0] = c.policy_len
        offs.append(eng.submit_packed_decoded(k, c.bits, scalars, moves, sym=c.ids))
    for k in (2, 0, 3, 1):
        _, _, sk = eng.wait_decoded_status(k, offs[k])
        assert sorted(np.flatnonzero(sk).tolist()) == [k + 1, 20 + k] and sk[k + 1] & NONFINITE and sk[20 + k] == BAD_DECODE

    # ---- fallback on: the range boards come back as the exact-f32 engine's, the decode errors stay the caller's ----
    eng.set_range_fallback(F32)
    eng32 = capi.Engine(c.model, dev, 64, F32)
    eng32.set_symmetries(c.square_src, c.policy_map)
    ref32 = eng32.eval_packed_decoded(c.bits[RANGE], c.scalars_bad[RANGE], [c.moves[b] for b in RANGE], sym=c.ids[RANGE])
    fb = c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad, status=True)
    assert all(fb[2][b] == FELL_BACK for b in RANGE) and all(fb[2][b] == BAD_DECODE for b in DECODE)
    assert sorted(np.flatnonzero(fb[2]).tolist()) == sorted(RANGE + DECODE)
    assert all(same_board(fb, clean, b) for b in good)
    for i, b in enumerate(RANGE):
        assert np.array_equal(fb[0][b], ref32[0][i]) and np.array_equal(fb[1][b], ref32[1][i])
        dv = float(np.abs(fb[0][b][:4] - v_ora[i][:4]).max())
        dp = float(np.abs(fb[1][b] - p_ora[i]).max()) if fb[1][b].size else 0.0
        dm = float(abs(fb[0][b][4] - v_ora[i][4]) / max(1.0, abs(v_ora[i][4])))
        print(f"[{eng.tower_path}] fell-back board {b} vs oracle: |dvalue, dwdl| {dv:.2e} |dprob| {dp:.2e} |dmoves_left|/scale {dm:.2e} "
              f"(moves_left {v_ora[i][4]:.4g})")
        assert dv <= F32_ATOL and dp <= F32_ATOL and dm <= F32_ATOL
    with pytest.raises(capi.KzError, match=SOFTMAX_MSG):  # the decode errors still fail the calls without a status
        c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad)
    # range causes alone: every call that returns the batch succeeds
    got = c.decoded(eng, 3, c.scalars_bad, c.moves, c.ids_hole)
    got_eval = eng.eval_packed_decoded(c.bits, c.scalars_bad, c.moves, sym=c.ids_hole)
    ref32h = eng32.eval_packed_decoded(c.bits[RANGE], c.scalars_bad[RANGE], [c.moves[b] for b in RANGE], sym=c.ids_hole[RANGE])
    for i, b in enumerate(RANGE):
        assert np.array_equal(got[0][b], ref32h[0][i]) and np.array_equal(got[1][b], ref32h[1][i])
    assert all(same_board(got, got_eval, b) for b in range(BATCH)) and all(same_board(got, clean, b) for b in good + DECODE)
    s32, p32 = eng32.eval_packed(c.bits[RANGE], c.scalars_bad[RANGE])
    s_clean, p_clean = eng.eval_packed(c.bits, c.scalars)
    rest = [b for b in range(BATCH) if b not in RANGE]
    for s, p in (eng.eval_packed(c.bits, c.scalars_bad), eng.wait_view(1, eng.submit_packed(1, c.bits, c.scalars_bad))):
        assert np.array_equal(s[RANGE], s32) and np.array_equal(p[RANGE], p32)
        assert np.array_equal(s[rest], s_clean[rest]) and np.array_equal(p[rest], p_clean[rest])
    # off again: the old failure is back
    eng.set_range_fallback(-1)
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        eng.eval_packed(c.bits, c.scalars_bad)


def test_f32_engine_reports_and_refuses_the_fallback(dev):
    """tower_resident_f32+heads (kz_conv_heads.hpp behind kz_tower_f32.hip): nothing finite is out of range in exact f32, so the
    range cause is an infinite scalar plane."""
    c = Case(dev, "ataxx-7", 3, 128, "ataxx_conv", F32, "tower_resident_f32+heads")
    eng = c.eng
    bad = c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad, status=True)
    st = bad[2]
    assert sorted(np.flatnonzero(st).tolist()) == sorted(RANGE + DECODE)
    assert all(st[b] & NONFINITE for b in RANGE) and all(st[b] == BAD_DECODE for b in DECODE)
    clean = c.decoded(eng, 0, c.scalars, c.moves, c.ids_hole, status=True)
    assert not clean[2].any()
    assert all(same_board(bad, clean, b) for b in range(BATCH) if st[b] == OK)
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        c.decoded(eng, 0, c.scalars_bad, c.moves_bad, c.ids_bad)
    with pytest.raises(capi.KzError, match="evaluates in KZ_DTYPE_F32 already"):
        eng.set_range_fallback(F32)
    with pytest.raises(capi.KzError, match="evaluates in KZ_DTYPE_F32 already"):
        eng.set_range_fallback(-1)


def test_set_range_fallback_argument_errors(dev):
    c = Case(dev, "ataxx-7", 3, 128, "ataxx_conv", F16, "tower_resident_f16g+heads")
    eng = c.eng
    with pytest.raises(capi.KzError, match="dtype must be KZ_DTYPE_F32"):
        eng.set_range_fallback(F16)
    off = eng.submit_packed_decoded(2, c.bits, c.scalars, c.moves, sym=c.ids)
    with pytest.raises(capi.KzError, match="a batch is in flight"):
        eng.set_range_fallback(F32)
    eng.wait_decoded(2, off)
    eng.set_range_fallback(F32)
    eng.set_range_fallback(F32)  # (on twice is on)
    eng.set_symmetries(c.square_src, c.policy_map)  # reaches the sibling
    _, _, st = c.decoded(eng, 0, c.scalars_bad, c.moves, c.ids_hole, status=True)
    assert sorted(np.flatnonzero(st).tolist()) == RANGE and all(st[b] == FELL_BACK for b in RANGE)
    # batch == 0: the same no-op, with a status view
    v, p, st0 = eng.wait_decoded_status(1, eng.submit_packed_decoded(1, c.bits[:0], c.scalars[:0], []))
    assert v.shape == (0, 5) and p == [] and st0.shape == (0,)
    with pytest.raises(capi.KzError, match="nothing submitted with a move list"):
        eng.wait_decoded_status(1, np.zeros(1, np.int64))


@pytest.mark.parametrize("channels,path", [(128, "tower_resident_f16g+heads"), (64, "tower_resident_f16g")],
                         ids=["decode_in_launch", "decode_kernel"])
def test_averaged_entries(dev, channels, path):
    """Ataxx D4, 8 boards in an engine of 64 (= 64 virtual boards): a source board is flagged when ONE virtual board is, and a
    fell-back board is the exact-f32 engine's averaged result."""
    blob = synth.random_model("ataxx-7", 2, channels, "ataxx_conv", seed=5)
    model = capi.Model(blob=blob)
    eng = capi.Engine(model, dev, 64, F16)
    assert eng.tower_path == path
    square_src, policy_map = ataxx_tables(7)
    valid = np.flatnonzero((policy_map >= 0).all(axis=0))
    rng = np.random.default_rng(71)
    bits, scalars = synth.random_boards("ataxx-7", 8, seed=71)
    moves = move_lists(rng, valid, 8, finished=4)
    one_only = policy_map.copy()
    gone = next(int(m) for m in moves[7] if all(m not in moves[b] for b in range(7)))  # a move only board 7 lists
    one_only[5, gone] = -1  # board 7 loses it under symmetry 5 only
    eng.set_symmetries(square_src, one_only)
    scalars_bad = scalars.copy()
    scalars_bad[2, 0] = 3e5

    def avg(e, s, status=False):
        off = e.submit_packed_decoded_avg(1, bits, s, moves)
        return e.wait_decoded_status(1, off) if status else e.wait_decoded(1, off)

    bad = avg(eng, scalars_bad, status=True)
    assert sorted(np.flatnonzero(bad[2]).tolist()) == [2, 7] and bad[2][2] & NONFINITE and bad[2][7] == BAD_DECODE
    with pytest.raises(capi.KzError, match=NONFINITE_MSG):
        avg(eng, scalars_bad)
    with pytest.raises(capi.KzError, match="no image under"):
        avg(eng, scalars)
    benign = avg(eng, scalars, status=True)
    assert np.flatnonzero(benign[2]).tolist() == [7]
    assert all(same_board(bad, benign, b) for b in range(8) if b not in (2, 7))
    eng.set_range_fallback(F32)
    eng32 = capi.Engine(model, dev, 64, F32)
    eng32.set_symmetries(square_src, one_only)
    ref32 = eng32.eval_packed_decoded_avg(bits[2:3], scalars_bad[2:3], moves[2:3])
    fb = avg(eng, scalars_bad, status=True)
    assert fb[2][2] == FELL_BACK and fb[2][7] == BAD_DECODE and sorted(np.flatnonzero(fb[2]).tolist()) == [2, 7]
    assert np.array_equal(fb[0][2], ref32[0][0]) and np.array_equal(fb[1][2], ref32[1][0])
    assert all(same_board(fb, benign, b) for b in range(8) if b not in (2, 7))
    eng.set_symmetries(square_src, policy_map)  # board 7's move is back, on the sibling too: the averaged calls succeed
    eng32.set_symmetries(square_src, policy_map)
    ok = avg(eng, scalars_bad)
    ref32 = eng32.eval_packed_decoded_avg(bits[2:3], scalars_bad[2:3], moves[2:3])
    assert np.array_equal(ok[0][2], ref32[0][0]) and np.array_equal(ok[1][2], ref32[1][0])
    assert same_board(ok, eng.eval_packed_decoded_avg(bits, scalars_bad, moves), 2)
