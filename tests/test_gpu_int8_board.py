"""KZ_DTYPE_INT8_ANY's per-layer plan ("board_conv_i8") on the GPU, on ordinary networks: random-init Go 19x19 2x128 and 2x256,
Go 9x9 2x256 and Ataxx 7x7 2x384, calibrated on the evaluated boards, against the exact-f32 engine of the same model.
tests/test_gpu_int8_board_exact.py holds the arithmetic to the bit; this file is the contract on values that round everywhere.

The bound is not taken from the GPU.  It is the quantisation error the contract itself has on this network and these boards:
tests/int8_nets.int8_reference (float64, quantising where the contract quantises) against the unquantised float64 reference
(exact_nets.reference), as max and rms of the difference over the output scale max(1, max |ref|) (tests/test_gpu_bf16.py:
max_and_rms), times 1.5 for what the reference does not model — the f16 head kernels behind the tower and the f32 summation
order of the stem, which can move a value across a rounding boundary of its int8 step.  The test prints both pairs.

The networks are exact_nets' containers (identity BatchNorms, so that the fold is exact and the reference and the engines see
the same f32 weights) with every convolution and linear layer drawn from a normal distribution of variance 2 / fan_in (the
stem's weights rounded to f16, the boards in halves: the stem's operands are f16 values, as the reference requires).

Then the engine surface on that plan: the non-finite status and the range fallback on boards pushed beyond +-65504, one batch of
mixed symmetry ids against the same boards transformed on the host, and capi.calibrate_int8 on a Go-size board."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E
from tests import int8_board_nets as B
from tests import int8_nets as N
from tests.test_gpu_bf16 import max_and_rms
from tests.test_gpu_symmetry import Case, ataxx_tables

pytestmark = pytest.mark.gpu

ANY, F16, F32 = capi.KZ_DTYPE_INT8_ANY, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32
PATH = "board_conv_i8"
MAX_BATCH = 64
MARGIN = 1.5
# (id, game, channels, head, boards): 2 bpw + 1 boards or more, so that a ragged workgroup and idle ones occur
NETS = [("go19x128", "go-19", 128, "conv", 5), ("go19x256", "go-19", 256, "conv", 3), ("go9x256", "go-9", 256, "conv", 9),
        ("ataxx7x384", "ataxx-7", 384, "ataxx_conv", 13)]
NET = {n[0]: n for n in NETS}


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def random_init(game, depth, channels, head, seed, stem_bias=0.0):
    """(meta, tensors): exact_nets' container with normal weights of variance 2 / fan_in in every layer."""
    meta, t = E._draw(game, depth, channels, head, None, seed, 1.0, {})
    rng = np.random.default_rng([seed, 424243])
    for p in E.layer_names(t):
        w = t[p + ".weight"]
        fan = int(np.prod(w.shape[1:]))
        w = rng.normal(0.0, np.sqrt(2.0 / fan), size=w.shape)
        if p == "common.tower.0":
            w = w.astype(np.float16)
            t[p + ".bias"] = (t[p + ".bias"].astype(np.float64) + stem_bias).astype(np.float32)
        t[p + ".weight"] = w.astype(np.float32)
    return meta, t


class Ref:
    """A network, its boards, the two float64 references and the bound they give: computed once, never written to."""
    _cache = {}

    def __init__(self, name):
        _, self.game, channels, head, boards = NET[name]
        self.meta, self.t = random_init(self.game, 2, channels, head, seed=5)
        self.bits, self.scalars_in = E.exact_boards(self.game, boards, 3)
        x = E.encode(self.meta, self.bits, self.scalars_in)
        s, p, rep = E.reference(self.t, self.meta, x, exact=False, rounding=(frozenset(), None))
        depth = self.meta["tower_depth"]
        names = ["tower.0"] + [n for i in range(1, depth + 1) for n in (f"tower.{i}.mid", f"tower.{i}")]
        names[-1] = f"tower.{depth + 1}"
        self.site_max = np.array([np.abs(rep.values[n]).max() for n in names], np.float32)  # headroom 1, the evaluated boards
        exps = [N.i8_exponent(m) for m in self.site_max]
        s8, p8, _, _ = N.int8_reference(self.t, self.meta, x, exps, exact=False)
        self.s, self.p = s.astype(np.float32), p.astype(np.float32)
        self.ref_max, self.ref_rms = max_and_rms(s8.astype(np.float32), p8.astype(np.float32), self.s, self.p)
        self.exps = exps
        self.blob = E.write_model(self.meta, self.t)
        for a in (self.bits, self.scalars_in, self.s, self.p):
            a.setflags(write=False)

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]


@pytest.mark.parametrize("name", [n[0] for n in NETS])
def test_within_the_contracts_own_quantisation_error_of_exact_f32(dev, name):
    r = Ref.get(name)
    model = capi.Model(blob=r.blob).quantize_int8(r.site_max)
    assert list(model.int8_site_exponents()) == r.exps[:-1]
    eng = capi.Engine(model, dev, MAX_BATCH, ANY)
    assert eng.tower_path == PATH
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    s32, p32 = capi.Engine(model, dev, MAX_BATCH, F32).eval_packed(r.bits, r.scalars_in)
    s16, p16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    worst, rms = max_and_rms(s, p, s32, p32)
    worst16, rms16 = max_and_rms(s16, p16, s32, p32)
    f32_max, f32_rms = max_and_rms(s32, p32, r.s, r.p)
    print(f"[int8 per layer] {name}: reference int8 vs float64 max {r.ref_max:.3e} rms {r.ref_rms:.3e} (bound x {MARGIN}); "
          f"engine int8 vs f32 max {worst:.3e} rms {rms:.3e}; f16 vs f32 max {worst16:.3e} rms {rms16:.3e}; "
          f"f32 engine vs float64 max {f32_max:.3e} rms {f32_rms:.3e}")
    assert np.isfinite(s).all() and np.isfinite(p).all()
    assert f32_max <= 1e-4  # the yardstick is the reference's network
    assert worst <= MARGIN * r.ref_max, f"{name}: max |delta| / scale = {worst:.3e} > {MARGIN} x {r.ref_max:.3e}"
    assert rms <= MARGIN * r.ref_rms, f"{name}: rms |delta| / scale = {rms:.3e} > {MARGIN} x {r.ref_rms:.3e}"
    assert rms >= 2 * rms16  # something is being quantised
    n = len(r.bits) // 2 + 1  # a prefix batch: the same boards, the same bits
    s_pre, p_pre = eng.eval_packed(r.bits[:n], r.scalars_in[:n])
    assert np.array_equal(s_pre, s[:n]) and np.array_equal(p_pre, p[:n])


def test_range_beyond_f16_is_reported_and_falls_back(dev):
    """2^17 added to the stem's bias: the f16 stream overflows on every board, the calibration (from the float64 reference)
    and the exact-f32 engine do not."""
    game, boards = "go-9", 5
    meta, t = random_init(game, 2, 256, "conv", seed=5, stem_bias=2.0 ** 17)
    bits, scalars = E.exact_boards(game, boards, 3)
    x = E.encode(meta, bits, scalars)
    _, _, rep = E.reference(t, meta, x, exact=False, rounding=(frozenset(), None))
    names = ["tower.0", "tower.1.mid", "tower.1", "tower.2.mid", "tower.3"]
    site_max = np.array([np.abs(rep.values[n]).max() for n in names], np.float32)
    assert site_max[0] > 65504 and np.isfinite(site_max).all()
    model = capi.Model(blob=E.write_model(meta, t)).quantize_int8(site_max)
    policy_len = synth.game_spec(game)["policy_len"]
    rng = np.random.default_rng(9)
    moves = [rng.permutation(policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=boards)]
    _, _, status16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed_decoded_status(bits, scalars, moves)
    assert ((status16 & capi.KZ_BOARD_NONFINITE) != 0).all(), status16
    eng = capi.Engine(model, dev, MAX_BATCH, ANY)
    assert eng.tower_path == PATH
    _, _, status = eng.eval_packed_decoded_status(bits, scalars, moves)
    assert ((status & capi.KZ_BOARD_NONFINITE) != 0).all(), status
    eng.set_range_fallback(F32)
    values, probs, status = eng.eval_packed_decoded_status(bits, scalars, moves)
    assert ((status & capi.KZ_BOARD_FELL_BACK) != 0).all(), status
    v32, p32, _ = capi.Engine(model, dev, MAX_BATCH, F32).eval_packed_decoded_status(bits, scalars, moves)
    assert np.array_equal(values, v32) and all(np.array_equal(a, b) for a, b in zip(probs, p32))


class CalibratedCase(Case):
    """tests/test_gpu_symmetry.py's Case on a dtype-8 engine of the per-layer plan, calibrated on boards of its own."""

    def __init__(self, dev, game, depth, channels, head, max_batch, seed=5):
        g = synth.game_spec(game)
        self.blob = synth.random_model(game, depth, channels, head, seed=seed)
        self.game, self.hw, self.n_bool, self.n_scalar, self.policy_len = game, g["size"] ** 2, g["n_bool"], g["n_scalar"], g["policy_len"]
        bits, scalars = synth.random_boards(game, 32, seed=9)
        self.eng = capi.Engine(capi.calibrate_int8(capi.Model(blob=self.blob), dev, bits, scalars, headroom=2.0), dev, max_batch, ANY)
        assert self.eng.tower_path == PATH
        self.square_src, self.policy_map = ataxx_tables(g["size"])
        self.n_sym = len(self.square_src)
        self.valid = np.flatnonzero(self.policy_map[0] >= 0)
        self.eng.set_symmetries(self.square_src, self.policy_map)


def test_sym_entry_with_mixed_ids(dev):
    CalibratedCase(dev, "ataxx-7", 2, 384, "ataxx_conv", MAX_BATCH).check(13, 1, slot=1)


def test_calibrate_int8_on_a_go_size_board(dev):
    model = capi.Model(blob=synth.random_model("go-19", 2, 128, "conv", seed=5))
    bits, scalars = synth.random_boards("go-19", 3, seed=3)
    site_max, _ = model.range_profile(dev, bits, scalars)
    quant = capi.calibrate_int8(model, dev, bits, scalars, headroom=2.0)
    assert list(quant.int8_site_exponents()) == [N.i8_exponent(2.0 * float(m)) for m in site_max[:-1]]
    eng = capi.Engine(quant, dev, 8, ANY)
    assert eng.tower_path == PATH and eng.launch_geometry(3) == (B.workgroups(3, 19, 19, 128), 0)
    s, p = eng.eval_packed(bits, scalars)
    assert np.isfinite(s).all() and np.isfinite(p).all()
