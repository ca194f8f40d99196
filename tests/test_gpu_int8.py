"""KZ_DTYPE_INT8 on the GPU: the one-launch ResTower on the i8 matrix cores (kz_tower_i8.hip) behind f16 tensors, on a
calibrated model (kz_model_quantize_int8).  tests/test_gpu_int8_exact.py holds its arithmetic to the bit; this file is the
contract on ordinary networks (synth.random_model, depth 2) and the engine surface.

1. Parity with the CPU oracle through eval_packed, calibrated on the evaluated boards with headroom 1 (capi.calibrate_int8),
   batch 37 on an engine of 64; a prefix batch and, at 256 channels, the two-board launch reproduce the same boards bit for
   bit.  Tolerance, per board and per output tensor, the form of tests/test_gpu_bf16.py:
       max |delta| <= INT8_REL * max(1, max |ref|),  rms |delta| <= INT8_RMS * max(1, max |ref|)
   = 1.5 x the largest value measured on these networks on the MI355X against the oracle (MEASURED) — and, since one amplifying
   network sets those two and the others lie a factor of thirty below it, every network is also held to 1.5 x ITS OWN measured
   pair (`own_bounds`).  On top of it the int8 rms divided by the f16 engine's rms on the same boards lies in [2, 4 x the
   network's own measured ratio] (at most RATIO_MAX): below 2 nothing is being quantised.
2. Calibration from elsewhere: calibrated on a disjoint board sample with headroom 2 — a step twice as coarse, maxima the
   evaluated boards may exceed — the same form of bound with constants of its own (MEASURED_ELSEWHERE), per network too.
3. Engine surface: the decoded entries on all four slots against the oracle's decode_output of the oracle's logits, `_sym`
   with mixed ids, the audit against an exact-f32 sibling.
4. Range: the 2^12-scaled chess network of tests/test_gpu_bf16.py's range case leaves the f16 range on every board: the int8
   engine's residual stream is f16 and reports KZ_BOARD_NONFINITE per board like the f16 engine; with the range fallback on,
   the boards come back with the exact-f32 results.
5. Coexistence: an f16 engine and an int8 engine of one calibrated model, alive together, each return the bits they return
   alone (the weights cache keys them apart).

The weights are random-init: the error of a trained network is the caller's to measure with kz_engine_set_audit.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O
from tests.test_gpu_bf16 import max_and_rms, scaled_stream
from tests.test_gpu_symmetry import Case, ataxx_tables

pytestmark = pytest.mark.gpu

INT8, F16, F32, SPLIT16 = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
PATH = "tower_resident_i8"
BATCH, MAX_BATCH, PREFIX = 37, 64, 11

# (id, game, channels, head, synth keywords, boards per workgroup at batch 37, wide launch (engine max_batch, boards, per) or None)
NETS = [
    ("chess256", "chess", 256, "attention", {"block_gain": 64.0}, 1, (256, 255, 2)),  # tests/test_gpu_bf16.py's amplifying network
    ("ataxx7x128", "ataxx-7", 128, "ataxx_conv", {}, 2, None),        # two boards in seven tiles
    ("go9x128", "go-9", 128, "conv", {}, 1, None),                    # one board in six tiles
    ("chess128", "chess", 128, "attention", {}, 1, None),             # four tiles at 128 channels
    ("chesshist2x256", "chess-hist-2", 256, "attention", {}, 1, None),  # two stem chunks
]
NET = {n[0]: n for n in NETS}

# Measured on the MI355X against the CPU oracle, scalars and policy together (the figures `measure` below prints): name: (int8 max |delta| / scale, int8 rms / scale, f16 max, f16 rms, int8 rms / f16 rms)
# chess256 is the worst of every column, as in tests/test_gpu_bf16.py: its blocks amplify (block_gain 64: logits of several
# hundred); the four plain networks are a factor of thirty below it.
MEASURED = {
    "chess256": (7.970e-2, 1.505e-2, 2.190e-3, 3.973e-4, 37.88),
    "ataxx7x128": (2.544e-3, 4.917e-4, 2.740e-4, 4.870e-5, 10.10),
    "go9x128": (1.420e-3, 3.393e-4, 1.557e-4, 3.049e-5, 11.13),
    "chess128": (1.073e-3, 2.245e-4, 1.440e-4, 2.473e-5, 9.08),
    "chesshist2x256": (1.052e-3, 2.264e-4, 1.197e-4, 2.319e-5, 9.76),
}
MEASURED_ELSEWHERE = {  # calibrated on a disjoint sample (seed 103, 64 boards), headroom 2: (int8 max, int8 rms)
    "chess256": (1.451e-1, 2.707e-2),
    "ataxx7x128": (4.405e-3, 9.476e-4),
    "go9x128": (2.066e-3, 4.907e-4),
    "chess128": (3.338e-3, 5.553e-4),
    "chesshist2x256": (2.218e-3, 4.385e-4),
}
INT8_REL = 1.2e-1         # 1.5 x 7.970e-2, the worst max of MEASURED
INT8_RMS = 2.3e-2         # 1.5 x 1.505e-2, the worst rms of MEASURED
ELSEWHERE_REL = 2.2e-1    # 1.5 x 1.451e-1, the worst max of MEASURED_ELSEWHERE
ELSEWHERE_RMS = 4.1e-2    # 1.5 x 2.707e-2, the worst rms of MEASURED_ELSEWHERE
RATIO_MIN, RATIO_MAX = 2.0, 152.0  # the upper end: 4 x 37.88, the largest ratio of MEASURED


def own_bounds(table, name):
    """1.5 x the network's own measured (max, rms): the arithmetic is deterministic, so the margin is for another box's f16 heads
    and calibration profile, not for noise."""
    return 1.5 * table[name][0], 1.5 * table[name][1]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its boards and the oracle's outputs: computed once per module, never written to."""
    _cache = {}

    def __init__(self, name):
        _, self.game, channels, head, kw, self.per, self.wide = NET[name]
        self.blob = synth.random_model(self.game, 2, channels, head, seed=5, **kw)
        self.bits, self.scalars_in = synth.random_boards(self.game, BATCH, seed=3)
        net = O.OracleNet(self.blob)
        self.x = O.encode_input_full(self.bits, self.scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        self.s, self.p = net.forward(self.x)
        self.policy_len = net.policy_len
        for a in (self.bits, self.scalars_in, self.x, self.s, self.p):
            a.setflags(write=False)

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]

    def calibrated(self, dev, elsewhere=False):
        model = capi.Model(blob=self.blob)
        if elsewhere:
            bits, scalars = synth.random_boards(self.game, 64, seed=103)
            return capi.calibrate_int8(model, dev, bits, scalars, headroom=2.0)
        return capi.calibrate_int8(model, dev, self.bits, self.scalars_in, headroom=1.0)


def measure(dev, name, elsewhere=False):
    """(int8 max, int8 rms, f16 max, f16 rms, rms ratio, the int8 engine, its outputs) on the network's boards."""
    r = Ref.get(name)
    model = r.calibrated(dev, elsewhere)
    eng = capi.Engine(model, dev, MAX_BATCH, INT8)
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    s16, p16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    worst, rms = max_and_rms(s, p, r.s, r.p)
    worst16, rms16 = max_and_rms(s16, p16, r.s, r.p)
    print(f"[int8 / f16] {name}{' (calibrated elsewhere, headroom 2)' if elsewhere else ''}: int8 max {worst:.3e} rms {rms:.3e}; "
          f"f16 max {worst16:.3e} rms {rms16:.3e}; rms ratio {rms / rms16:.2f}")
    return worst, rms, worst16, rms16, rms / rms16, model, eng, s, p


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n[0] for n in NETS])
def test_parity_with_the_oracle(dev, name):
    r = Ref.get(name)
    worst, rms, _, _, ratio, model, eng, s, p = measure(dev, name)
    assert eng.tower_path == PATH
    assert eng.launch_geometry(BATCH) == ((BATCH + r.per - 1) // r.per, r.per)
    assert np.isfinite(s).all() and np.isfinite(p).all()
    assert worst <= INT8_REL, f"{name}: max |delta| / scale = {worst:.3e} > {INT8_REL}"
    assert rms <= INT8_RMS, f"{name}: rms |delta| / scale = {rms:.3e} > {INT8_RMS}"
    own_rel, own_rms = own_bounds(MEASURED, name)
    assert worst <= own_rel and rms <= own_rms, f"{name}: max {worst:.3e} (own bound {own_rel:.3e}), rms {rms:.3e} (own bound {own_rms:.3e})"
    assert RATIO_MIN <= ratio <= min(RATIO_MAX, 4 * MEASURED[name][4]), f"{name}: int8 rms / f16 rms = {ratio:.2f}"
    s_pre, p_pre = eng.eval_packed(r.bits[:PREFIX], r.scalars_in[:PREFIX])
    assert np.array_equal(s_pre, s[:PREFIX]) and np.array_equal(p_pre, p[:PREFIX])
    if r.wide:
        max_batch, boards, per = r.wide
        wide = capi.Engine(model, dev, max_batch, INT8)
        assert wide.tower_path == PATH
        assert wide.launch_geometry(boards) == ((boards + per - 1) // per, per)
        pick = np.arange(boards) % BATCH
        s_w, p_w = wide.eval_packed(r.bits[pick], r.scalars_in[pick])
        assert np.array_equal(s_w, s[pick]) and np.array_equal(p_w, p[pick])


# ---- 2. calibration from elsewhere ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n[0] for n in NETS])
def test_calibrated_on_a_disjoint_sample(dev, name):
    worst, rms, _, _, _, _, eng, s, p = measure(dev, name, elsewhere=True)
    assert eng.tower_path == PATH
    assert np.isfinite(s).all() and np.isfinite(p).all()
    assert worst <= ELSEWHERE_REL, f"{name}: max |delta| / scale = {worst:.3e} > {ELSEWHERE_REL}"
    assert rms <= ELSEWHERE_RMS, f"{name}: rms |delta| / scale = {rms:.3e} > {ELSEWHERE_RMS}"
    own_rel, own_rms = own_bounds(MEASURED_ELSEWHERE, name)
    assert worst <= own_rel and rms <= own_rms, f"{name}: max {worst:.3e} (own bound {own_rel:.3e}), rms {rms:.3e} (own bound {own_rms:.3e})"


# ---- 3. engine surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "chesshist2x256"])
def test_decoded_entries_on_all_slots(dev, name):
    """submit_packed_decoded on the four slots, then the four waits, against the oracle's decode_output of the oracle's
    logits.  A logit off by d moves a softmax's probability, and tanh, by at most exp(2 d) - 1; d is this network's own bound,
    1.5 x its MEASURED max times the scale."""
    r = Ref.get(name)
    eng = capi.Engine(r.calibrated(dev), dev, MAX_BATCH, INT8)
    assert eng.tower_path == PATH
    rng = np.random.default_rng(21)
    valid = np.arange(r.policy_len)
    jobs = []
    for slot in range(4):
        lo, n = 5 * slot, 7 + 5 * slot  # overlapping slices of the boards, a different batch per slot
        moves = [rng.permutation(valid)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=n)]
        jobs.append((slot, lo, n, moves, eng.submit_packed_decoded(slot, r.bits[lo:lo + n], r.scalars_in[lo:lo + n], moves)))
    got = [eng.wait_decoded(slot, offsets) for slot, _, _, _, offsets in jobs]
    for (slot, lo, n, moves, _), (values, probs) in zip(jobs, got):
        v_ref, p_ref = O.decode_output(r.s[lo:lo + n], r.p[lo:lo + n], moves)
        d = 1.5 * MEASURED[name][0] * max(1.0, float(np.abs(r.p[lo:lo + n]).max()), float(np.abs(r.s[lo:lo + n]).max()))
        bound = float(np.expm1(2 * d))
        assert np.abs(values[:, :4] - v_ref[:, :4]).max() <= bound, slot
        assert np.abs(values[:, 4] - v_ref[:, 4]).max() <= d, slot
        assert all(a.shape == b.shape for a, b in zip(probs, p_ref))
        assert max(float(np.abs(a - b).max()) for a, b in zip(probs, p_ref)) <= bound, slot


class CalibratedCase(Case):
    """tests/test_gpu_symmetry.py's Case on an int8 engine: the same network, calibrated on boards of its own."""

    def __init__(self, dev, game, depth, channels, head, max_batch, seed=5):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed)
        self.game, self.hw, self.n_bool, self.n_scalar, self.policy_len = game, g["size"] ** 2, g["n_bool"], g["n_scalar"], g["policy_len"]
        bits, scalars = synth.random_boards(game, 32, seed=9)
        self.eng = capi.Engine(capi.calibrate_int8(capi.Model(blob=self.blob), dev, bits, scalars, headroom=2.0), dev, max_batch, INT8)
        assert self.eng.tower_path == PATH
        self.square_src, self.policy_map = ataxx_tables(g["size"])
        self.n_sym = len(self.square_src)
        self.valid = np.flatnonzero(self.policy_map[0] >= 0)
        self.eng.set_symmetries(self.square_src, self.policy_map)


def test_sym_entry_with_mixed_ids(dev):
    case = CalibratedCase(dev, "ataxx-7", 2, 128, "ataxx_conv", MAX_BATCH)
    for slot, (batch, seed) in enumerate([(BATCH, 1), (9, 2)]):
        case.check(batch, seed, slot=slot)


def test_audit_against_exact_f32(dev):
    r = Ref.get("ataxx7x128")
    eng = capi.Engine(r.calibrated(dev), dev, MAX_BATCH, INT8)
    with pytest.raises(capi.KzError, match="dtype must be"):  # (int8 is no yardstick)
        eng.set_audit(INT8, 1, 16)
    eng.set_audit(SPLIT16, 1, 16)  # (either exact sibling is accepted)
    eng.set_audit(F32, 1, 16)
    rng = np.random.default_rng(4)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    values, _ = eng.wait_decoded(0, eng.submit_packed_decoded(0, r.bits, r.scalars_in, moves))
    stats = eng.audit_stats()
    print(f"[audit] {stats!r}")
    assert stats.batches == 1 and stats.boards == 16 and stats.skipped == 0
    assert stats.moves == sum(len(m) for m in moves[:16])
    assert np.isfinite(stats.max_abs_prob) and np.isfinite(stats.max_abs_value).all()
    assert stats.max_abs_prob > 0 and stats.max_abs_value.max() > 0  # int8 against exact f32: the audit saw the difference


# ---- 4. range ---------------------------------------------------------------------------------------------------------------
def test_range_beyond_f16_is_reported_and_falls_back(dev):
    r = Ref.get("chess256")
    blob = scaled_stream(r.blob)
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, r.bits, r.scalars_in)  # (the profile is exact f32: finite maxima)
    rng = np.random.default_rng(9)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    f16 = capi.Engine(model, dev, MAX_BATCH, F16)
    _, _, status16 = f16.eval_packed_decoded_status(r.bits, r.scalars_in, moves)
    assert ((status16 & capi.KZ_BOARD_NONFINITE) != 0).all(), status16
    eng = capi.Engine(model, dev, MAX_BATCH, INT8)
    assert eng.tower_path == PATH
    _, _, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, moves)
    assert ((status & capi.KZ_BOARD_NONFINITE) != 0).all(), status
    eng.set_range_fallback(F32)
    values, probs, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, moves)
    assert ((status & capi.KZ_BOARD_FELL_BACK) != 0).all(), status
    v32, p32, _ = capi.Engine(model, dev, MAX_BATCH, F32).eval_packed_decoded_status(r.bits, r.scalars_in, moves)
    assert np.array_equal(values, v32) and all(np.array_equal(a, b) for a, b in zip(probs, p32))


# ---- 5. coexistence ---------------------------------------------------------------------------------------------------------
def test_f16_and_int8_engines_of_one_model_coexist(dev):
    r = Ref.get("chess128")
    model = r.calibrated(dev)
    alone16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    alone8 = capi.Engine(model, dev, MAX_BATCH, INT8).eval_packed(r.bits, r.scalars_in)
    a, b = capi.Engine(model, dev, MAX_BATCH, F16), capi.Engine(model, dev, MAX_BATCH, INT8)
    assert a.tower_path != b.tower_path == PATH
    for _ in range(2):
        got8, got16 = b.eval_packed(r.bits, r.scalars_in), a.eval_packed(r.bits, r.scalars_in)
        assert all(np.array_equal(x, y) for x, y in zip(got16, alone16))
        assert all(np.array_equal(x, y) for x, y in zip(got8, alone8))
    assert not np.array_equal(alone8[1], alone16[1])
    # the calibrated model's f16 engine is the source's
    src16 = capi.Engine(capi.Model(blob=r.blob), dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    assert all(np.array_equal(x, y) for x, y in zip(src16, alone16))
