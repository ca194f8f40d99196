"""KZ_DTYPE_INT8_HEADS on the GPU: "tower_resident_i8+heads" — dtype 4's int8 tower with the conv policy heads, the scalar
head and decode_output inside its launch — on ordinary networks (synth.random_model, depth 2) and through the engine surface.
tests/test_gpu_int8_heads_exact.py holds its arithmetic to the bit; this file is the contract beside it.

Networks: tests/test_gpu_int8.py's ataxx7x128 (two boards in seven tiles) and go9x128 (one board in six, with its pass move),
and ataxx-7 2x256 (one board in four tiles at 256 channels); batch 37 on an engine of 64.

1. Parity with the CPU oracle, calibrated on the evaluated boards (headroom 1) and on a disjoint sample (headroom 2): the two
   128-channel networks are held to tests/test_gpu_int8.py's own_bounds(MEASURED) and own_bounds(MEASURED_ELSEWHERE) — figures
   measured on dtype 4, whose heads are other kernels: the in-launch tail is the plain-f16 launch's, whose error against the
   oracle (the f16 columns of MEASURED) is a tenth of the int8 tower's, so the 1.5 x margin holds it.  The 256-channel network
   has no row there: 1.5 x what a dtype-4 engine of the same model measures in the same test.
2. Against dtype 4 on the same calibrated model and boards.  The towers are bit-identical, so the difference is the two head
   arithmetics' — the f16 MFMA tail in the launch against the separate f16 head kernels.  The same difference exists between
   the f16 engine with its heads inside ("tower_resident_f16g+heads") and the f16 engine created under KZ_NO_FUSED_HEADS=1; it
   is measured here on the same boards, max and rms per output tensor, and dtype 5 - dtype 4 must stay within 2 x that (2: the
   tower outputs that feed the heads are other values and round differently).  Measured on the MI355X,
   (scalars max, scalars rms, policy max, policy rms) of |dtype 5 - dtype 4| over that of |f16 fused - f16 unfused|:
       ataxx7x128   1.975e-05 7.982e-06 9.025e-05 2.179e-05   over   1.971e-05 7.935e-06 9.007e-05 2.180e-05
       go9x128      5.137e-05 1.761e-05 3.796e-05 6.993e-06   over   5.136e-05 1.762e-05 3.792e-05 6.992e-06
       ataxx7x256   1.858e-05 5.753e-06 5.618e-05 1.488e-05   over   1.860e-05 5.734e-06 5.621e-05 1.486e-05
   (every ratio within 1 %: the bound of 2 is not what the code is tuned to.)
3. One launch: with set_profiling, N decoded batches are exactly N launches in total, all named kz_tower_resident_i8; the
   dtype-4 engine of the same model launches more.
4. Decode: on one exact network per tail geometry (int8_nets' ataxx7_2x128 and go9_3x128) the raw entry returns the reference's
   bits, and eval_packed_decoded_status on lists in the style of tests/decode_cases.py — all moves, an empty list, a list with
   repeated indices longer than a wave's staging (a quarter of the X image: XIMG / 16 floats) so that the re-read tail runs —
   meets decode_cases' derived bounds against the float64 decode of those known logits; status 0 everywhere; a board with one
   move index outside the policy gets KZ_BOARD_BAD_DECODE alone.
5. Engine surface: all four slots in flight; `_sym` with mixed ids against the host route (tests/test_gpu_symmetry.py); `_avg`
   against the exact-f32 engine's averaged results; a prefix batch and one board reproduce the full batch's bits; a dtype-4, a
   dtype-5 and an f16 engine of one model alive together each return the bits they return alone.
6. Range: the 2^12-scaled stream of an amplifying Ataxx network leaves the f16 range on every board: the launch's own tail
   reports KZ_BOARD_NONFINITE per board; with the range fallback on, the exact-f32 results come back with KZ_BOARD_FELL_BACK.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import decode_cases as D
from tests import exact_nets as E
from tests import int8_nets as N
from tests import oracle_lib as O
from tests.test_gpu_bf16 import max_and_rms, scaled_stream
from tests.test_gpu_int8 import BATCH, MAX_BATCH, MEASURED, MEASURED_ELSEWHERE, PREFIX, Ref, own_bounds
from tests.test_gpu_int8_exact import same_bits
from tests.test_gpu_symmetry import Case, ataxx_tables

pytestmark = pytest.mark.gpu

HEADS, INT8, F16, F32 = capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32
PATH = "tower_resident_i8+heads"
NAMES = ("ataxx7x128", "go9x128", "ataxx7x256")
PER = {"ataxx7x128": 2, "go9x128": 1, "ataxx7x256": 1}


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref256(Ref):
    """ataxx-7 2x256, which tests/test_gpu_int8.py's table does not have: the same draws (seeds 5 and 3), computed once."""

    def __init__(self):
        self.game, self.per, self.wide = "ataxx-7", 1, None
        self.blob = synth.random_model(self.game, 2, 256, "ataxx_conv", seed=5)
        self.bits, self.scalars_in = synth.random_boards(self.game, BATCH, seed=3)
        net = O.OracleNet(self.blob)
        self.x = O.encode_input_full(self.bits, self.scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        self.s, self.p = net.forward(self.x)
        self.policy_len = net.policy_len
        for a in (self.bits, self.scalars_in, self.x, self.s, self.p):
            a.setflags(write=False)


_REF256 = []


def ref_of(name):
    if name != "ataxx7x256":
        return Ref.get(name)
    if not _REF256:
        _REF256.append(Ref256())
    return _REF256[0]


def engine(model, dev, dtype=HEADS, max_batch=MAX_BATCH):
    eng = capi.Engine(model, dev, max_batch, dtype)
    assert eng.tower_path == (PATH if dtype == HEADS else "tower_resident_i8" if dtype == INT8 else eng.tower_path)
    return eng


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elsewhere", [False, True], ids=["own-boards", "elsewhere"])
@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_oracle(dev, name, elsewhere):
    r = ref_of(name)
    model = r.calibrated(dev, elsewhere)
    eng = engine(model, dev)
    assert eng.launch_geometry(BATCH) == ((BATCH + PER[name] - 1) // PER[name], PER[name])
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    assert np.isfinite(s).all() and np.isfinite(p).all()
    worst, rms = max_and_rms(s, p, r.s, r.p)
    if name == "ataxx7x256":
        s4, p4 = engine(model, dev, INT8).eval_packed(r.bits, r.scalars_in)
        worst4, rms4 = max_and_rms(s4, p4, r.s, r.p)
        own_rel, own_rms = 1.5 * worst4, 1.5 * rms4
    else:
        own_rel, own_rms = own_bounds(MEASURED_ELSEWHERE if elsewhere else MEASURED, name)
    print(f"[int8+heads] {name}{' (calibrated elsewhere, headroom 2)' if elsewhere else ''}: max {worst:.3e} (bound {own_rel:.3e}) "
          f"rms {rms:.3e} (bound {own_rms:.3e})")
    assert worst <= own_rel and rms <= own_rms, f"{name}: max {worst:.3e} (bound {own_rel:.3e}), rms {rms:.3e} (bound {own_rms:.3e})"


# ---- 2. against dtype 4 -----------------------------------------------------------------------------------------------------
def max_rms(a, b):
    """(max, rms) of |a - b| over one output tensor, in the outputs' own units: both sides of the comparison are the same
    network on the same boards."""
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


@pytest.mark.parametrize("name", NAMES)
def test_the_difference_to_dtype_4_is_the_two_head_arithmetics(dev, name, monkeypatch):
    r = ref_of(name)
    model = r.calibrated(dev)
    s5, p5 = engine(model, dev).eval_packed(r.bits, r.scalars_in)
    s4, p4 = engine(model, dev, INT8).eval_packed(r.bits, r.scalars_in)
    fused = capi.Engine(model, dev, MAX_BATCH, F16)
    monkeypatch.setenv("KZ_NO_FUSED_HEADS", "1")
    unfused = capi.Engine(model, dev, MAX_BATCH, F16)
    monkeypatch.delenv("KZ_NO_FUSED_HEADS")
    assert fused.tower_path == "tower_resident_f16g+heads" and unfused.tower_path == "tower_resident_f16g"
    sf, pf = fused.eval_packed(r.bits, r.scalars_in)
    su, pu = unfused.eval_packed(r.bits, r.scalars_in)
    got = max_rms(s5, s4) + max_rms(p5, p4)
    base = max_rms(sf, su) + max_rms(pf, pu)
    print(f"[int8+heads - int8] {name}: scalars max {got[0]:.3e} rms {got[1]:.3e}, policy max {got[2]:.3e} rms {got[3]:.3e}; "
          f"f16 fused - unfused: scalars max {base[0]:.3e} rms {base[1]:.3e}, policy max {base[2]:.3e} rms {base[3]:.3e}")
    assert all(b > 0 for b in base), base  # (the two f16 head arithmetics do differ: the yardstick measures something)
    for what, g, b in zip(("scalars max", "scalars rms", "policy max", "policy rms"), got, base):
        assert g <= 2 * b, f"{name}, {what}: |dtype 5 - dtype 4| = {g:.3e} > 2 x {b:.3e}"


# ---- 3. one launch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "go9x128"])
def test_a_decoded_batch_is_one_launch(dev, name):
    r = ref_of(name)
    model = r.calibrated(dev)
    rng = np.random.default_rng(2)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    counts = {}
    for dtype in (HEADS, INT8):
        eng = engine(model, dev, dtype)
        eng.eval_packed_decoded(r.bits, r.scalars_in, moves)  # (first use)
        eng.set_profiling(True)
        before, before_tower = eng.kernel_time("")[1], eng.kernel_time("kz_tower_resident_i8")[1]
        for _ in range(3):
            eng.eval_packed_decoded(r.bits, r.scalars_in, moves)
        counts[dtype] = (eng.kernel_time("")[1] - before, eng.kernel_time("kz_tower_resident_i8")[1] - before_tower)
        eng.set_profiling(False)
    print(f"[launches] {name}: (all, kz_tower_resident_i8) of three decoded batches: dtype 5 {counts[HEADS]}, dtype 4 {counts[INT8]}")
    assert counts[HEADS] == (3, 3), counts  # exactly one launch per batch, and it is the tower's
    assert counts[INT8][1] == 3 and counts[INT8][0] > 3, counts  # the same tower, then the head kernels and the decode
    assert model.plan(MAX_BATCH, HEADS) == (PATH, 1)


# ---- 4. decode --------------------------------------------------------------------------------------------------------------
# (exact network, bytes of the X image = the decode's staging: ROWS * (2 C + 16))
@pytest.mark.parametrize("net,ximg", [("ataxx7_2x128", 112 * 272), ("go9_3x128", 96 * 272)])
def test_decode_inside_the_launch_on_known_logits(dev, net, ximg):
    b = N.build_exact(net, None)
    eng = engine(capi.Model(blob=b.blob).quantize_int8(b.site_max), dev)
    s, p = eng.eval_packed(b.bits, b.scalars_in)
    same_bits(b, s, p, np.arange(N.BOARDS), f"{net}, raw")
    policy_len, cap = b.ref_policy.shape[1], ximg // 16
    rng = np.random.default_rng(3)
    n_long = cap + 130
    lists = []
    for board in range(N.BOARDS):
        kind = board % 3
        if kind == 0:
            lists.append(np.arange(policy_len, dtype=np.int32))          # all moves
        elif kind == 1:
            lists.append(np.zeros(0, np.int32))                           # a finished board
        else:                                                             # repeated indices, longer than the staging
            lists.append(np.resize(rng.permutation(policy_len), n_long).astype(np.int32))
    assert any(len(m) > cap for m in lists) and any(len(m) == 0 for m in lists)
    values, probs, status = eng.eval_packed_decoded_status(b.bits, b.scalars_in, lists)
    assert (status == 0).all(), status
    ref_values, ref_probs = E.decode_ref(b.ref_scalars, b.ref_policy, lists)
    worst = D.Worst()
    why = D.values_errors(values, ref_values, b.ref_scalars[:, 4], worst)
    for board, (out, ref) in enumerate(zip(probs, ref_probs)):
        assert out.shape == ref.shape
        if len(ref):
            why += [f"board {board}: {x}" for x in D.probs_errors(out, ref, worst)]
    print(f"[int8+heads decode] {net}: {worst}")
    assert not why, why
    # one index outside the policy on one board: that board alone is flagged, and with the decode's bit alone
    bad = [m.copy() for m in lists]
    victim = 3  # (an all-moves board)
    bad[victim][5] = policy_len
    _, probs_bad, status = eng.eval_packed_decoded_status(b.bits, b.scalars_in, bad)
    assert status[victim] == capi.KZ_BOARD_BAD_DECODE and (np.delete(status, victim) == 0).all(), status
    assert all(np.array_equal(a, c) for i, (a, c) in enumerate(zip(probs_bad, probs)) if i != victim)


# ---- 5. engine surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "ataxx7x256"])
def test_decoded_entries_on_all_slots(dev, name):
    """The four slots in flight at once (two streams, zero-copy staging), against the oracle's decode_output of the oracle's
    logits: a logit off by d moves a softmax's probability, and tanh, by at most exp(2 d) - 1; d is the bound of test 1 on
    these boards times the scale — and every slot returns the bits the synchronous entry returns for its boards."""
    r = ref_of(name)
    model = r.calibrated(dev)
    eng = engine(model, dev)
    if name == "ataxx7x256":
        s4, p4 = engine(model, dev, INT8).eval_packed(r.bits, r.scalars_in)
        rel = 1.5 * max_and_rms(s4, p4, r.s, r.p)[0]
    else:
        rel = own_bounds(MEASURED, name)[0]
    rng = np.random.default_rng(21)
    jobs = []
    for slot in range(4):
        lo, n = 5 * slot, 7 + 5 * slot
        moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=n)]
        jobs.append((slot, lo, n, moves, eng.submit_packed_decoded(slot, r.bits[lo:lo + n], r.scalars_in[lo:lo + n], moves)))
    got = [eng.wait_decoded(slot, offsets) for slot, _, _, _, offsets in jobs]
    for (slot, lo, n, moves, _), (values, probs) in zip(jobs, got):
        v_ref, p_ref = O.decode_output(r.s[lo:lo + n], r.p[lo:lo + n], moves)
        d = rel * max(1.0, float(np.abs(r.p[lo:lo + n]).max()), float(np.abs(r.s[lo:lo + n]).max()))
        bound = float(np.expm1(2 * d))
        assert np.abs(values[:, :4] - v_ref[:, :4]).max() <= bound, slot
        assert np.abs(values[:, 4] - v_ref[:, 4]).max() <= d, slot
        assert all(a.shape == c.shape for a, c in zip(probs, p_ref))
        assert max(float(np.abs(a - c).max()) for a, c in zip(probs, p_ref)) <= bound, slot
        v_one, p_one = eng.eval_packed_decoded(r.bits[lo:lo + n], r.scalars_in[lo:lo + n], moves)
        assert np.array_equal(v_one, values) and all(np.array_equal(a, c) for a, c in zip(p_one, probs)), slot


class CalibratedCase(Case):
    """tests/test_gpu_symmetry.py's Case on a dtype-5 engine: the same network, calibrated on boards of its own."""

    def __init__(self, dev, game, depth, channels, head, max_batch, seed=5):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed)
        self.game, self.hw, self.n_bool, self.n_scalar, self.policy_len = game, g["size"] ** 2, g["n_bool"], g["n_scalar"], g["policy_len"]
        bits, scalars = synth.random_boards(game, 32, seed=9)
        self.model = capi.calibrate_int8(capi.Model(blob=self.blob), dev, bits, scalars, headroom=2.0)
        self.eng = engine(self.model, dev, HEADS, max_batch)
        self.square_src, self.policy_map = ataxx_tables(g["size"])
        self.n_sym = len(self.square_src)
        self.valid = np.flatnonzero(self.policy_map[0] >= 0)
        self.eng.set_symmetries(self.square_src, self.policy_map)


def test_sym_entry_with_mixed_ids_and_the_averaged_entry(dev):
    case = CalibratedCase(dev, "ataxx-7", 2, 128, "ataxx_conv", MAX_BATCH)
    for slot, (batch, seed) in enumerate([(BATCH, 1), (9, 2)]):
        case.check(batch, seed, slot=slot)
    # `_avg`: every board under the eight symmetries, averaged inside the engine, against the exact-f32 engine's averaged
    # results.  The model is calibrated on a disjoint sample with headroom 2, and the mapped boards are boards it has not seen:
    # the situation of MEASURED_ELSEWHERE, so a logit is off by at most d = 1.5 x that table's max times the scale on every
    # virtual board, a probability and tanh by exp(2 d) - 1, and an average of such values by no more.
    bits, scalars, moves, _ = case.inputs(MAX_BATCH // case.n_sym, 4)
    f32 = capi.Engine(case.model, dev, MAX_BATCH, F32)
    f32.set_symmetries(case.square_src, case.policy_map)
    s32, p32 = f32.eval_packed(bits, scalars)
    d = own_bounds(MEASURED_ELSEWHERE, "ataxx7x128")[0] * max(1.0, float(np.abs(s32).max()), float(np.abs(p32).max()))
    bound = float(np.expm1(2 * d))
    v_ref, p_ref = f32.eval_packed_decoded_avg(bits, scalars, moves)
    values, probs = case.eng.wait_decoded(1, case.eng.submit_packed_decoded_avg(1, bits, scalars, moves))
    assert np.abs(values[:, :4] - v_ref[:, :4]).max() <= bound and np.abs(values[:, 4] - v_ref[:, 4]).max() <= d
    assert all(a.shape == c.shape for a, c in zip(probs, p_ref))
    assert max(float(np.abs(a - c).max()) for a, c in zip(probs, p_ref) if a.size) <= bound
    again = case.eng.eval_packed_decoded_avg(bits, scalars, moves)
    assert np.array_equal(again[0], values) and all(np.array_equal(a, c) for a, c in zip(again[1], probs))


@pytest.mark.parametrize("name", NAMES)
def test_prefix_batches_and_coexistence(dev, name):
    r = ref_of(name)
    model = r.calibrated(dev)
    alone = {dt: capi.Engine(model, dev, MAX_BATCH, dt).eval_packed(r.bits, r.scalars_in) for dt in (HEADS, INT8, F16)}
    engines = {dt: capi.Engine(model, dev, MAX_BATCH, dt) for dt in (INT8, HEADS, F16)}
    assert engines[HEADS].tower_path == PATH and engines[INT8].tower_path == "tower_resident_i8"
    assert engines[F16].tower_path == "tower_resident_f16g+heads"
    for _ in range(2):
        for dt in (F16, HEADS, INT8):
            got = engines[dt].eval_packed(r.bits, r.scalars_in)
            assert all(np.array_equal(x, y) for x, y in zip(got, alone[dt])), dt
    assert not np.array_equal(alone[HEADS][1], alone[F16][1])
    s, p = alone[HEADS]
    for n in (PREFIX, 1):
        s_pre, p_pre = engines[HEADS].eval_packed(r.bits[:n], r.scalars_in[:n])
        assert np.array_equal(s_pre, s[:n]) and np.array_equal(p_pre, p[:n]), n


# ---- 6. range ---------------------------------------------------------------------------------------------------------------
def test_range_beyond_f16_is_reported_from_inside_the_launch_and_falls_back(dev):
    blob = scaled_stream(synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=5, block_gain=64.0))
    bits, scalars = synth.random_boards("ataxx-7", BATCH, seed=3)
    policy_len = synth.game_spec("ataxx-7")["policy_len"]
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, bits, scalars)  # (the profile is exact f32: finite maxima)
    rng = np.random.default_rng(9)
    moves = [rng.permutation(policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    _, _, status16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed_decoded_status(bits, scalars, moves)
    assert ((status16 & capi.KZ_BOARD_NONFINITE) != 0).all(), status16  # (the network does leave the f16 range on every board)
    eng = engine(model, dev)
    _, _, status = eng.eval_packed_decoded_status(bits, scalars, moves)
    assert ((status & capi.KZ_BOARD_NONFINITE) != 0).all(), status
    eng.set_range_fallback(F32)
    values, probs, status = eng.eval_packed_decoded_status(bits, scalars, moves)
    assert ((status & capi.KZ_BOARD_FELL_BACK) != 0).all(), status
    v32, p32, _ = capi.Engine(model, dev, MAX_BATCH, F32).eval_packed_decoded_status(bits, scalars, moves)
    assert np.array_equal(values, v32) and all(np.array_equal(a, c) for a, c in zip(probs, p32))
