"""Every board under every symmetry, averaged inside the engine (the `_avg` decoded entries, include/kz_hip.h): the reference's
AverageSymmetryNetwork (rust/kz-core/src/network/symmetry.rs:70-124,150-184) as a fan-out kernel in front of the unchanged
network launches and an averaging kernel behind them (kzero_amd/csrc/kz_symmetry_avg.hip).

The yardstick is the existing `_sym` entry on the same engine, fed np.repeat-ed boards, repeated move lists and ids
tile(arange(n_sym)): that replicated batch has the size and the order of the virtual batch the new entry builds on the device,
so the same kernels see the same planes at the same positions.  Its per-symmetry results are averaged here in numpy float32
in the order the header states (average_f32), and the new entry must be np.array_equal to that — no tolerance.  The 2 x 128
Ataxx networks are additionally held to the oracle at the bounds tests/test_gpu_parity.py states for the decoded boundary: an
average of eight results that each meet a bound meets it too."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O
from tests.test_gpu_parity import F16_PROB_ATOL, F16_VALUE_ATOL, F32_ATOL, assert_f16, assert_f32
from tests.test_gpu_symmetry import ataxx_tables, go_tables, map_bits, map_moves, move_lists, synthetic_tables

pytestmark = pytest.mark.gpu

F16, F32, SPLIT16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


# ---- the arithmetic, as include/kz_hip.h states it ----------------------------------------------------------------------
def average_f32(values, probs, n_sym):
    """values [batch * n_sym, 5] and probs (one array per virtual board), virtual board b * n_sym + k = board b under symmetry
    k -> ([batch, 5], [one array per board]), all float32:
        value = (((0 + v_0) + v_1) + ... + v_{n-1}) / n         probability = ((0 + p_0 / n) + p_1 / n) + ..."""
    values = np.asarray(values, np.float32)
    batch, n = len(values) // n_sym, np.float32(n_sym)
    assert len(values) == batch * n_sym == len(probs)
    acc = np.zeros((batch, 5), np.float32)
    for k in range(n_sym):
        acc = acc + values[k::n_sym]
    out_v = acc / n
    out_p = []
    for b in range(batch):
        acc = np.zeros(len(probs[b * n_sym]), np.float32)
        for k in range(n_sym):
            acc = acc + np.asarray(probs[b * n_sym + k], np.float32) / n
        out_p.append(acc)
    assert out_v.dtype == np.float32 and all(p.dtype == np.float32 for p in out_p)
    return out_v, out_p


def replicated(bits, scalars, moves, n_sym):
    """The virtual batch, built on the host: what the `_sym` entry is fed."""
    ids = np.tile(np.arange(n_sym), len(bits)).astype(np.uint8)
    return np.repeat(bits, n_sym, axis=0), np.repeat(scalars, n_sym, axis=0), [m for m in moves for _ in range(n_sym)], ids


def same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


class Case:
    def __init__(self, dev, game, depth, channels, head, dtype, path, max_batch, tables=None, seed=5):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed)
        self.game, self.hw, self.n_bool = game, g["size"] ** 2, g["n_bool"]
        self.eng = capi.Engine(capi.Model(blob=self.blob), dev, max_batch, dtype)
        assert self.eng.tower_path == path
        if tables == "ataxx":
            tables = ataxx_tables(g["size"])
        elif tables == "go":
            tables = go_tables(g["size"])
        elif tables is None:
            tables = synthetic_tables(self.hw, g["policy_len"], 3, seed=77)
        self.square_src, self.policy_map = tables
        self.n_sym = len(self.square_src)
        self.valid = np.flatnonzero((self.policy_map >= 0).all(axis=0))  # moves with an image under every symmetry
        self.eng.set_symmetries(self.square_src, self.policy_map)

    def inputs(self, batch, seed, finished=None):
        rng = np.random.default_rng(seed)
        bits, scalars = synth.random_boards(self.game, batch, seed=seed)
        return bits, scalars, move_lists(rng, self.valid, batch, finished=int(rng.integers(0, batch)) if finished is None else finished)

    def yardstick(self, bits, scalars, moves, slot=0):
        r = replicated(bits, scalars, moves, self.n_sym)
        v, p = self.eng.wait_decoded(slot, self.eng.submit_packed_decoded(slot, r[0], r[1], r[2], sym=r[3]))
        return average_f32(v, p, self.n_sym)

    def check(self, batch, seed, slot=0):
        bits, scalars, moves = self.inputs(batch, seed)
        assert any(m.size == 0 for m in moves) and any(m.size for m in moves)
        ref = self.yardstick(bits, scalars, moves, slot)
        got = self.eng.wait_decoded(slot, self.eng.submit_packed_decoded_avg(slot, bits, scalars, moves))
        assert same(got, ref)
        assert same(self.eng.eval_packed_decoded_avg(bits, scalars, moves), ref)
        assert all(a.shape == m.shape for a, m in zip(got[1], moves))
        if self.n_sym > 1:  # (the average does something: the plain evaluation differs)
            v0, _ = self.eng.eval_packed_decoded(bits, scalars, moves)
            assert not np.array_equal(v0, got[0])
        return bits, scalars, moves, got


def against_oracle(case, dtype, bits, scalars, moves, got):
    """OracleNet.forward on the mapped boards of every symmetry, O.decode_output with the mapped lists, averaged in float64."""
    net = O.OracleNet(case.blob)
    r_bits, r_scalars, r_moves, ids = replicated(bits, scalars, moves, case.n_sym)
    m_bits, m_moves = map_bits(r_bits, case.n_bool, case.hw, case.square_src, ids), map_moves(r_moves, case.policy_map, ids)
    s_ora, p_ora = net.forward(O.encode_input_full(m_bits, r_scalars, net.n_scalar, net.n_bool, net.h, net.w))
    v_k, p_k = O.decode_output(s_ora, p_ora, m_moves)
    n = case.n_sym
    v_ora = np.asarray(v_k, np.float64).reshape(len(bits), n, 5).mean(axis=1)
    probs_ora = [np.mean([np.asarray(p_k[b * n + k], np.float64) for k in range(n)], axis=0) for b in range(len(bits))]
    v, p = got
    worst_p = max(float(np.abs(a - b).max()) for a, b in zip(p, probs_ora) if a.size)
    worst_v = float(np.abs(v[:, :4] - v_ora[:, :4]).max())
    print(f"[average vs oracle, {case.eng.tower_path}] max |dprob| {worst_p:.2e}, max |dvalue, dwdl| {worst_v:.2e}")
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
    assert case.n_sym == 8 and case.eng.max_batch // case.n_sym == 8
    against_oracle(case, dtype, *case.check(8, seed=11))  # exactly max_batch / n_sym
    against_oracle(case, dtype, *case.check(5, seed=12))


def test_ataxx_2x64_heads_and_decode_as_separate_launches(dev):
    """tower_resident_f16g without fused heads: the stand-alone kz_decode_output between the two new kernels."""
    case = Case(dev, "ataxx-7", 2, 64, "ataxx_conv", F16, "tower_resident_f16g", 64, tables="ataxx")
    case.check(8, seed=13)
    case.check(5, seed=14)


def test_ataxx_2x64_per_layer_path_stand_alone_encode(dev, monkeypatch):
    """KZ_FORCE_GENERIC=1: the stand-alone kz_encode_packed reads the virtual batch."""
    monkeypatch.setenv("KZ_FORCE_GENERIC", "1")
    case = Case(dev, "ataxx-7", 2, 64, "ataxx_conv", F16, "conv_igemm_f16", 64, tables="ataxx")
    case.check(8, seed=15)
    case.check(5, seed=16)


def test_ataxx_2x128_several_boards_per_workgroup(dev):
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", 512, tables="ataxx")
    wgs, per = case.eng.launch_geometry(200)
    assert per > 1 and wgs > 1
    case.check(25, seed=17)  # 200 virtual boards


# ---- Go 9x9, tables from the formula ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", [(F16, "tower_resident_f16g+heads"), (SPLIT16, "tower_resident_split16+heads")],
                         ids=["f16", "split16"])
def test_go9_2x128(dev, dtype, path):
    case = Case(dev, "go-9", 2, 128, "conv", dtype, path, 64, tables="go")
    assert np.all(case.policy_map[:, 0] == 0)  # pass is index 0 and every symmetry fixes it
    for batch, seed in ((8, 21), (5, 22)):
        _, _, moves, _ = case.check(batch, seed)
        assert any(0 in m for m in moves)


# ---- chess: no symmetry of its own, three synthetic ones; every slot in flight ------------------------------------------
def test_chess_2x256_attention_head_on_all_slots(dev):
    case = Case(dev, "chess", 2, 256, "attention", F16, "tower_resident_f16+heads", 64)
    eng, n = case.eng, case.n_sym
    assert n == 3
    # all four slots in flight with different batches, waited out of order; the references afterwards, slot by slot
    batches = [case.inputs(21 - 4 * k, seed=30 + k) for k in range(capi.KZ_ENGINE_SLOTS)]
    offs = [eng.submit_packed_decoded_avg(k, *b) for k, b in enumerate(batches)]
    got = {k: eng.wait_decoded(k, offs[k]) for k in (2, 0, 3, 1)}
    refs = [case.yardstick(*b, slot=k) for k, b in enumerate(batches)]
    for k in range(capi.KZ_ENGINE_SLOTS):
        assert same(got[k], refs[k]), k
    # an averaged submit and a plain `_sym` submit side by side on neighbouring slots (the two streams of the "+heads" paths)
    r = replicated(*batches[1], n)
    off_avg = eng.submit_packed_decoded_avg(0, *batches[0])
    off_sym = eng.submit_packed_decoded(1, r[0], r[1], r[2], sym=r[3])
    off_avg2 = eng.submit_packed_decoded_avg(2, *batches[2])
    assert same(average_f32(*eng.wait_decoded(1, off_sym), n), refs[1])
    assert same(eng.wait_decoded(2, off_avg2), refs[2])
    assert same(eng.wait_decoded(0, off_avg), refs[0])
    case.check(21, seed=35)  # 63 of 64 virtual boards


# ---- identity -----------------------------------------------------------------------------------------------------------
def test_one_identity_symmetry_is_the_plain_decoded_entry(dev):
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", 64,
                tables=(np.arange(49, dtype=np.int32)[None], np.arange(17 * 49 + 1, dtype=np.int32)[None]))
    eng = case.eng
    bits, scalars, moves = case.inputs(37, seed=51)
    ref = eng.wait_decoded(0, eng.submit_packed_decoded(0, bits, scalars, moves))
    assert same(eng.wait_decoded(1, eng.submit_packed_decoded_avg(1, bits, scalars, moves)), ref)
    assert same(eng.eval_packed_decoded_avg(bits, scalars, moves), ref)
    # batch == 0: the same no-op as for the other decoded entries
    v, p = eng.eval_packed_decoded_avg(bits[:0], scalars[:0], [])
    assert v.shape == (0, 5) and p == []
    v, p = eng.wait_decoded(2, eng.submit_packed_decoded_avg(2, bits[:0], scalars[:0], []))
    assert v.shape == (0, 5) and p == []


# ---- the move arrays of the virtual batch grow on demand ----------------------------------------------------------------
def test_move_scratch_grows_and_a_small_batch_follows(dev):
    """The first scratch holds max_batch * 64 = 4096 virtual moves; 7 boards of 520 moves need 8 * 3640."""
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", F16, "tower_resident_f16g+heads", 64, tables="ataxx")
    eng = case.eng
    case.check(5, seed=61, slot=1)  # the first scratch of slot 1
    rng = np.random.default_rng(62)
    bits, scalars = synth.random_boards("ataxx-7", 8, seed=62)
    assert len(case.valid) >= 520
    moves = [rng.permutation(case.valid)[:520].astype(np.int32) for _ in range(8)]
    moves[3] = np.zeros(0, np.int32)
    assert case.n_sym * sum(len(m) for m in moves) > eng.max_batch * 64
    ref = case.yardstick(bits, scalars, moves, slot=0)
    assert same(eng.wait_decoded(1, eng.submit_packed_decoded_avg(1, bits, scalars, moves)), ref)
    case.check(3, seed=63, slot=1)


# ---- errors: a message each, no device fault, and the engine evaluates correctly afterwards -----------------------------
@pytest.mark.parametrize("channels,path", [(128, "tower_resident_f16g+heads"), (64, "tower_resident_f16g")],
                         ids=["decode_in_launch", "decode_kernel"])
def test_errors(dev, channels, path):
    blob = synth.random_model("ataxx-7", 2, channels, "ataxx_conv", seed=5)
    eng = capi.Engine(capi.Model(blob=blob), dev, 64, F16)
    assert eng.tower_path == path
    square_src, policy_map = ataxx_tables(7)
    valid = np.flatnonzero((policy_map >= 0).all(axis=0))
    rng = np.random.default_rng(71)
    bits, scalars = synth.random_boards("ataxx-7", 9, seed=71)
    moves = move_lists(rng, valid, 9, finished=4)

    def good():
        r = replicated(bits[:8], scalars[:8], moves[:8], 8)
        ref = average_f32(*eng.wait_decoded(0, eng.submit_packed_decoded(0, r[0], r[1], r[2], sym=r[3])), 8)
        assert same(eng.wait_decoded(2, eng.submit_packed_decoded_avg(2, bits[:8], scalars[:8], moves[:8])), ref)

    # before any tables are set
    with pytest.raises(capi.KzError, match="no tables set"):
        eng.submit_packed_decoded_avg(0, bits[:8], scalars[:8], moves[:8])
    with pytest.raises(capi.KzError, match="no tables set"):
        eng.eval_packed_decoded_avg(bits[:8], scalars[:8], moves[:8])
    eng.set_symmetries(square_src, policy_map)
    good()
    # batch * n_sym = max_batch + n_sym: the message carries the limit max_batch / n_sym
    with pytest.raises(capi.KzError, match=r"max_batch / n_sym = 8\b"):
        eng.submit_packed_decoded_avg(0, bits, scalars, moves)
    with pytest.raises(capi.KzError, match=r"max_batch / n_sym = 8\b"):
        eng.eval_packed_decoded_avg(bits, scalars, moves)
    # a bad slot, bad offsets, null arguments: as for the other decoded submits
    with pytest.raises(capi.KzError, match="bad slot"):
        eng.submit_packed_decoded_avg(capi.KZ_ENGINE_SLOTS, bits[:8], scalars[:8], moves[:8])
    h = capi.load()
    offsets = np.array([0, 3, 2], np.int64)
    idx = np.zeros(3, np.int32)
    with pytest.raises(capi.KzError, match="non-decreasing"):
        capi.check(h.kz_engine_submit_packed_decoded_avg(eng._h, 0, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 2,
                                                         offsets.ctypes.data, idx.ctypes.data))
    with pytest.raises(capi.KzError, match="null argument"):
        capi.check(h.kz_engine_submit_packed_decoded_avg(eng._h, 0, None, bits.shape[1], scalars.ctypes.data, 2, offsets.ctypes.data,
                                                         idx.ctypes.data))
    # a slot still in flight; and the tables cannot change under an averaged batch
    off = eng.submit_packed_decoded_avg(1, bits[:8], scalars[:8], moves[:8])
    with pytest.raises(capi.KzError, match="still in flight"):
        eng.submit_packed_decoded_avg(1, bits[:8], scalars[:8], moves[:8])
    with pytest.raises(capi.KzError, match="in flight"):
        eng.set_symmetries(square_src, policy_map)
    eng.wait_decoded(1, off)
    good()
    # a listed move whose policy_map entry is -1 under ONE symmetry only
    one_only = policy_map.copy()
    gone = int(moves[7][0])
    one_only[5, gone] = -1
    eng.set_symmetries(square_src, one_only)
    off = eng.submit_packed_decoded_avg(3, bits[:8], scalars[:8], moves[:8])
    with pytest.raises(capi.KzError, match="no image under"):
        eng.wait_decoded(3, off)
    eng.set_symmetries(square_src, policy_map)
    good()
    # a move index equal to policy_len
    outside = [m.copy() for m in moves[:8]]
    outside[2][1] = policy_map.shape[1]
    off = eng.submit_packed_decoded_avg(3, bits[:8], scalars[:8], outside)
    with pytest.raises(capi.KzError, match="move index is out of range"):
        eng.wait_decoded(3, off)
    with pytest.raises(capi.KzError, match="move index is out of range"):
        eng.eval_packed_decoded_avg(bits[:8], scalars[:8], outside)
    good()
