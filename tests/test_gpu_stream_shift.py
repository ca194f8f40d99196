"""kz_model_stream_shift on the GPU: the same function with a residual stream 2^-k times as large, through every arithmetic.

1. The identity at zero tolerance.  scaled_stream(blob) (tests/test_gpu_bf16.py's recipe: the stream times 2^12, the same
   function) shifted by k = 12 has the original's folded weights bit for bit — the fold is f64 and every factor a power of two —
   so in F16, SPLIT16, F32 and BF16 the engine of the shifted model takes the original's path, returns the original's bits and
   reports status 0 on every board; the scaled model without the shift still flags every board in F16 and SPLIT16.
2. A negative shift: shift(Model(blob), -12) in F32 returns the bits of Model(scaled_stream(blob)) in F32.
3. Exact networks (tests/exact_nets.py), k = 3: every non-zero stored value times 2^-3 stays a normal f16 number (asserted on the
   CPU from the oracle's trace), so one engine of each addressing family returns the bits of the float64 reference.
4. In-range random networks, k = 4: F16 against the oracle inside F16_REL / F16_RMS of tests/test_gpu_parity.py, SPLIT16 within
   1e-4, the deviation printed with and without the shift.
5. End to end: profile the scaled network, k = shift_for(max, 2): the F16 engine of the shifted model has status 0 on every
   board and — the chess network; see the note at (5) for the Ataxx one — is inside the f16 contract against the oracle.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E
from tests import oracle_lib as O
from tests.test_gpu_exact import ENGINES, make_engine, mismatch
from tests.test_gpu_parity import F32_ATOL, assert_f16
from tests.test_gpu_range_profile import scaled_stream

pytestmark = pytest.mark.gpu

F16, F32, SPLIT16, BF16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16
BATCH, MAX_BATCH = 37, 64

# (id, game, channels, head, synth keywords): block_gain 64 lets the stream grow by tens per block, so that the 2^12 of
# scaled_stream takes it past 65504 on every board (asserted on the CPU below)
GAIN_NETS = [("chess256", "chess", 256, "attention", {"block_gain": 64.0}),
             ("ataxx7x128", "ataxx-7", 128, "ataxx_conv", {"block_gain": 64.0})]
PATHS = {
    "chess256": {F16: "tower_resident_f16+heads", SPLIT16: "tower_resident_split16+heads", F32: "tower_resident_f32", BF16: "tower_resident_bf16g"},
    "ataxx7x128": {F16: "tower_resident_f16g+heads", SPLIT16: "tower_resident_split16+heads", F32: "tower_resident_f32+heads",
                   BF16: "tower_resident_bf16g+heads"},
}


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its boards, move lists and the oracle's outputs and trace: computed once per module, never written to."""
    _cache = {}

    def __init__(self, game, channels, head, kw):
        self.blob = synth.random_model(game, 2, channels, head, seed=5, **kw)
        self.bits, self.scalars_in = synth.random_boards(game, BATCH, seed=3)
        net = O.OracleNet(self.blob)
        self.x = O.encode_input_full(self.bits, self.scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        self.s, self.p, acts = net.forward_trace(self.x)
        # the stream tensors every f16 kernel stores: the stem's output and block 1's
        self.stream_per_board = np.maximum(np.abs(acts["tower.0"]).reshape(BATCH, -1).max(axis=1),
                                           np.abs(acts["tower.1"]).reshape(BATCH, -1).max(axis=1))
        rng = np.random.default_rng(9)
        self.moves = [rng.permutation(net.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
        for a in (self.bits, self.scalars_in, self.x, self.s, self.p):
            a.setflags(write=False)

    @classmethod
    def get(cls, game, channels, head, kw):
        key = (game, channels, head, tuple(sorted(kw.items())))
        if key not in cls._cache:
            cls._cache[key] = cls(game, channels, head, kw)
        return cls._cache[key]


# ---- 1. the identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,game,channels,head,kw", GAIN_NETS, ids=[n[0] for n in GAIN_NETS])
def test_shifting_the_scaled_network_back_returns_the_original_bits(dev, name, game, channels, head, kw):
    r = Ref.get(game, channels, head, kw)
    assert (r.stream_per_board * 4096.0).min() > 65504.0  # the scaled stream leaves f16 on every board
    original = capi.Model(blob=r.blob)
    scaled = capi.Model(blob=scaled_stream(r.blob))
    shifted = scaled.stream_shift(12)
    for dtype in (F16, SPLIT16, F32, BF16):
        want = capi.Engine(original, dev, MAX_BATCH, dtype)
        eng = capi.Engine(shifted, dev, MAX_BATCH, dtype)
        assert eng.tower_path == want.tower_path == PATHS[name][dtype]
        s_want, p_want = want.eval_packed(r.bits, r.scalars_in)
        s, p = eng.eval_packed(r.bits, r.scalars_in)
        assert np.array_equal(s, s_want), f"dtype {dtype}, scalars: {mismatch(s, s_want, 5)}"
        assert np.array_equal(p, p_want), f"dtype {dtype}, policy: {mismatch(p, p_want, 64)}"
        values, probs, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, r.moves)
        assert (status == 0).all(), (dtype, status)
        v_want, probs_want, _ = want.eval_packed_decoded_status(r.bits, r.scalars_in, r.moves)
        assert np.array_equal(values, v_want) and all(np.array_equal(a, b) for a, b in zip(probs, probs_want))
    # without the shift the scaled model is out of range on every board, in both f16-storage arithmetics
    for dtype in (F16, SPLIT16):
        eng = capi.Engine(scaled, dev, MAX_BATCH, dtype)
        assert eng.tower_path == PATHS[name][dtype]
        _, _, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, r.moves)
        assert ((status & capi.KZ_BOARD_NONFINITE) != 0).all(), (dtype, status)


# ---- 2. a negative shift --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,game,channels,head,kw", GAIN_NETS, ids=[n[0] for n in GAIN_NETS])
def test_a_negative_shift_is_the_scaled_network(dev, name, game, channels, head, kw):
    r = Ref.get(game, channels, head, kw)
    enlarged = capi.Engine(capi.Model(blob=r.blob).stream_shift(-12), dev, MAX_BATCH, F32)
    scaled = capi.Engine(capi.Model(blob=scaled_stream(r.blob)), dev, MAX_BATCH, F32)
    assert enlarged.tower_path == scaled.tower_path == PATHS[name][F32]
    s, p = enlarged.eval_packed(r.bits, r.scalars_in)
    s_want, p_want = scaled.eval_packed(r.bits, r.scalars_in)
    assert np.array_equal(s, s_want), mismatch(s, s_want, 5)
    assert np.array_equal(p, p_want), mismatch(p, p_want, 64)
    assert np.abs(s - r.s).max() <= F32_ATOL * max(1.0, np.abs(r.s).max())  # (and it is still the function)


# ---- 3. exact networks ----------------------------------------------------------------------------------------------------
K_EXACT = 3
# one engine of each addressing family (tests/test_gpu_exact.py lists them all): the chess f16 launch at one and two boards per
# workgroup, the generic one-launch tower in plain f16 and in split arithmetic with the heads inside, the exact-f32 launch, the
# board-tile kernel at 64 channels in both arithmetics, the implicit GEMM
EXACT_IDS = ("chess256-f16-nb2", "chess256-f16-nb1", "ataxx7x128-f16g-2", "ataxx7x128-split16", "chess256-f32",
             "go19x64-board-f16", "go19x64-board-split16", "chess256x1-igemm-f16", "chess256x1-igemm-f32")
EXACT_ENGINES = [e for e in ENGINES if e[0] in EXACT_IDS]
assert len(EXACT_ENGINES) == len(EXACT_IDS)


@pytest.mark.parametrize("engine", EXACT_ENGINES, ids=[e[0] for e in EXACT_ENGINES])
def test_exact_networks_shifted_return_the_float64_bits(dev, engine):
    name, net_name, dtype, max_batch, switches, path, per, batch = engine
    b = E.build(net_name, None)
    # on the CPU, from the oracle's trace: no stored value of the shifted stream falls below f16's smallest normal number
    net = O.OracleNet(b.blob)
    x = O.encode_input_full(b.bits, b.scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
    _, _, acts = net.forward_trace(x)
    model = capi.Model(blob=b.blob)
    shifted_sites = model.range_sites()[:-1]
    for site in shifted_sites:
        v = np.abs(acts[site].astype(np.float64))
        assert v.max() > 0 and (v[v != 0] * 2.0 ** -K_EXACT).min() >= 2.0 ** -14, site
        assert (v * 2.0 ** -K_EXACT).max() <= 65504.0
    eng = make_engine(model.stream_shift(K_EXACT), dev, max_batch, dtype, switches)
    assert eng.tower_path == path
    if per is not None:
        assert eng.launch_geometry(batch) == ((batch + per - 1) // per, per)
    hw = b.meta["board_h"] * b.meta["board_w"]
    for idx in (np.arange(3, 3 + batch) % E.BOARDS, np.array([E.BOARDS - 1])):
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        assert np.array_equal(s, b.ref_scalars[idx]), "scalars: " + mismatch(s, b.ref_scalars[idx], 5)
        assert np.array_equal(p, b.ref_policy[idx]), "policy: " + mismatch(p, b.ref_policy[idx], hw)


# ---- 4. in-range random networks ------------------------------------------------------------------------------------------
K_RANDOM = 4
# (id, game, channels, head, engine max_batch, f16 path, split16 path): the chess launch, the generic one-launch tower, the
# board-tile kernel
RANDOM_NETS = [
    ("chess256", "chess", 256, "attention", 64, "tower_resident_f16+heads", "tower_resident_split16+heads"),
    ("ataxx7x128", "ataxx-7", 128, "ataxx_conv", 64, "tower_resident_f16g+heads", "tower_resident_split16+heads"),
    ("go19x64", "go-19", 64, "conv", 256, "board_conv_f16", "board_conv_split16"),
]


def deviation(out, ref):
    scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    d = (out - ref) / scale
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d ** 2)))


@pytest.mark.parametrize("name,game,channels,head,max_batch,path16,path_split", RANDOM_NETS, ids=[n[0] for n in RANDOM_NETS])
def test_in_range_networks_keep_their_contract_when_shifted(dev, name, game, channels, head, max_batch, path16, path_split):
    r = Ref.get(game, channels, head, {})
    model = capi.Model(blob=r.blob)
    shifted = model.stream_shift(K_RANDOM)
    plain16, shift16 = capi.Engine(model, dev, max_batch, F16), capi.Engine(shifted, dev, max_batch, F16)
    assert plain16.tower_path == shift16.tower_path == path16
    s0, p0 = plain16.eval_packed(r.bits, r.scalars_in)
    s, p = shift16.eval_packed(r.bits, r.scalars_in)
    for what, out, out0, ref in (("scalars", s, s0, r.s), ("policy", p, p0, r.p)):
        print(f"[shift] {name} f16 {what}: max / rms against the oracle {deviation(out, ref)[0]:.3e} / {deviation(out, ref)[1]:.3e} "
              f"shifted by 2^-{K_RANDOM}, {deviation(out0, ref)[0]:.3e} / {deviation(out0, ref)[1]:.3e} unshifted")
    assert_f16(s, r.s, f"{name} shifted, scalars")
    assert_f16(p, r.p, f"{name} shifted, policy")
    plain_split, shift_split = capi.Engine(model, dev, max_batch, SPLIT16), capi.Engine(shifted, dev, max_batch, SPLIT16)
    assert plain_split.tower_path == shift_split.tower_path == path_split
    s0, p0 = plain_split.eval_packed(r.bits, r.scalars_in)
    s, p = shift_split.eval_packed(r.bits, r.scalars_in)
    err = max(float(np.abs(s - r.s).max()), float(np.abs(p - r.p).max()))
    err0 = max(float(np.abs(s0 - r.s).max()), float(np.abs(p0 - r.p).max()))
    print(f"[shift] {name} split16: max |delta| against the oracle {err:.3e} shifted by 2^-{K_RANDOM}, {err0:.3e} unshifted")
    assert err <= 1e-4, f"{name} split16 shifted: max |delta| = {err:.3e} > 1e-4"


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
# The f16 contract against the oracle is asserted on the chess network, the scaled network of tests/test_gpu_bf16.py, whose plain
# f16 engine is inside it before any scaling (2.19e-3 / 3.97e-4 there).  The Ataxx gain network of (1) is not: unscaled and
# unshifted its f16 engine is at rms 7.05e-4 on the scalars (measured; F16_RMS is 6e-4), and a power-of-two shift neither adds
# to that nor takes from it (7.06e-4 scaled by 2^12 and shifted back by 2^-4).  There the test holds the shifted engine to the
# range — status 0 on every board, finite outputs — and prints its deviation from the oracle and from the unscaled network's own
# f16 engine (the same arithmetic on a stream 2^(12 - k) times as large; measured 7.06e-4 against 7.05e-4).
@pytest.mark.parametrize("name,game,channels,head,kw", GAIN_NETS, ids=[n[0] for n in GAIN_NETS])
def test_profile_then_shift_puts_the_scaled_network_back_in_range(dev, name, game, channels, head, kw):
    r = Ref.get(game, channels, head, kw)
    scaled = capi.Model(blob=scaled_stream(r.blob))
    site_max, board_max = scaled.range_profile(dev, r.bits, r.scalars_in)
    assert (board_max > 65504.0).all() and board_max.max() == site_max[:-1].max()
    k = capi.shift_for(float(board_max.max()), 2)
    print(f"[shift] {name}: stream max {board_max.max():.0f} = {board_max.max() / 65504.0:.1f} x 65504 -> k = {k}")
    assert 65504.0 / 8 < 2.0 ** -k * float(board_max.max()) <= 65504.0 / 4 and k >= 3  # two bits of headroom, not more
    eng = capi.Engine(scaled.stream_shift(k), dev, MAX_BATCH, F16)
    assert eng.tower_path == PATHS[name][F16]
    _, _, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, r.moves)
    assert (status == 0).all(), status
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    for what, out, ref in (("scalars", s, r.s), ("policy", p, r.p)):
        print(f"[shift] {name} scaled and shifted by 2^-{k}, {what}: max / rms against the oracle {deviation(out, ref)[0]:.3e} / {deviation(out, ref)[1]:.3e}")
    if name == "chess256":
        assert_f16(s, r.s, f"{name} scaled and shifted by 2^-{k}, scalars")
        assert_f16(p, r.p, f"{name} scaled and shifted by 2^-{k}, policy")
    # against the f16 engine of the unscaled network: the same arithmetic on a stream 2^(12 - k) times as large
    s0, p0 = capi.Engine(capi.Model(blob=r.blob), dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    for what, out, ref, oracle in (("scalars", s, s0, r.s), ("policy", p, p0, r.p)):
        print(f"[shift] {name} {what}: the unscaled network's f16 engine against the oracle {deviation(ref, oracle)[0]:.3e} / {deviation(ref, oracle)[1]:.3e}, "
              f"the shifted engine against it {deviation(out, ref)[0]:.3e} / {deviation(out, ref)[1]:.3e}")
        assert np.isfinite(out).all()
