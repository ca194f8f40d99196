"""KZ_DTYPE_BF16 on the GPU: the one-launch ResTower on bf16 elements (kz_tower_bf16g.hip) behind f32 tensors.

1. Parity with the CPU oracle through eval_packed on one network per branch of the kernel template, depth 2, batch 37 on an
   engine of 64; a prefix batch and (where the family has wide tiles) the wide launch reproduce the same boards bit for bit.
   Tolerance, per board and per output tensor like the f16 contract of tests/test_gpu_parity.py:
       max |delta| <= BF16_REL * max(1, max |ref|),  rms |delta| <= BF16_RMS * max(1, max |ref|)
   = 1.5 x the largest value measured on these networks (the rule the f16 constants follow; figures below).  On top of it the
   bf16 rms divided by the f16 engine's rms on the same network and boards lies in [2, 32]: the unit roundoffs differ by 2^3,
   a factor of 4 either way is margin; below 2 the kernel is not storing bf16 (or the test shows nothing), above 32 something
   rounds twice.
2. Exact networks (tests/exact_nets.py, float64 reference): networks whose tower tensors and tower weights stay within 128
   steps — half of what bf16's 8 bits hold — come back with the reference's bits, heads inside and heads outside.
3. Range: the chess 2x256 network of (1) with its residual stream scaled by 2^12 (the same function: the oracle returns the
   same bits) leaves the f16 range on every board; the f16 and split16 engines report KZ_BOARD_NONFINITE on every board, the
   bf16 engine status 0 and (1)'s bound.
4. Engine surface: the decoded entries on all four slots, `_sym`, the shadow audit against exact f32.

Measured (MI355X): MEASURED below — max |delta| / scale and rms / scale against the oracle, scalars and policy together, the f16
engine's two figures on the same boards, and the ratio of the two rms.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from kzero_amd.model_file import read_model, write_model
from tests import exact_nets as E
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, SPLIT16 = capi.KZ_DTYPE_BF16, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
HEADS_IN, HEADS_OUT = "tower_resident_bf16g+heads", "tower_resident_bf16g"

# name: (bf16 max, bf16 rms, f16 max, f16 rms, bf16 rms / f16 rms).  chess256 is the worst of both columns: its blocks amplify
# (block_gain 64: logits of several hundred) — the f16 engine is at 2.2e-3 / 4.0e-4 there, where the f16 constants of
# tests/test_gpu_parity.py come from (2.3e-3 / 4.1e-4); the six plain networks are a factor of ten below it in either arithmetic.
MEASURED = {
    "ataxx7x128": (1.760e-3, 3.447e-4, 2.740e-4, 4.870e-5, 7.08),
    "go9x128": (1.103e-3, 2.944e-4, 1.557e-4, 3.049e-5, 9.66),
    "chess64": (7.161e-4, 1.173e-4, 1.107e-4, 2.289e-5, 5.13),
    "chess192": (6.372e-4, 1.006e-4, 1.218e-4, 2.357e-5, 4.27),
    "chess256": (1.574e-2, 3.940e-3, 2.190e-3, 3.973e-4, 9.92),
    "chess320": (6.071e-4, 1.197e-4, 1.200e-4, 2.512e-5, 4.76),
    "chesshist2x256": (5.750e-4, 1.099e-4, 1.197e-4, 2.319e-5, 4.74),
}
# 1.5 x the worst of MEASURED
BF16_REL = 2.4e-2  # 1.5 x 1.574e-2
BF16_RMS = 5.9e-3  # 1.5 x 3.940e-3
RATIO_MIN, RATIO_MAX = 2.0, 32.0

BATCH, MAX_BATCH, PREFIX = 37, 64, 11

# (id, game, channels, head, synth keywords, path, boards per workgroup at batch 37,
#  wide launch: (engine max_batch, boards, boards per workgroup) or None)
# chess256: block_gain 64 lets the stream grow by tens per block, so that test_range's 2^12 takes it past 65504 on every board.
NETS = [
    ("ataxx7x128", "ataxx-7", 128, "ataxx_conv", {}, HEADS_IN, 2, (512, 509, 4)),  # +heads, two-plane images
    ("go9x128", "go-9", 128, "conv", {}, HEADS_IN, 1, (2048, 1534, 3)),            # +heads with the pass move; three boards in sixteen tiles
    ("chess64", "chess", 64, "attention", {}, HEADS_OUT, 1, None),                 # the deepest ring
    ("chess192", "chess", 192, "attention", {}, HEADS_OUT, 1, (256, 255, 2)),
    ("chess256", "chess", 256, "attention", {"block_gain": 64.0}, HEADS_OUT, 1, None),  # one-plane image, attention head outside
    ("chess320", "chess", 320, "attention", {}, HEADS_OUT, 1, None),
    ("chesshist2x256", "chess-hist-2", 256, "attention", {}, HEADS_OUT, 1, None),  # two stem chunks
]
NET = {n[0]: n for n in NETS}


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its boards and the oracle's outputs: computed once per module, never written to."""
    _cache = {}

    def __init__(self, name):
        _, self.game, channels, head, kw, self.path, self.per, self.wide = NET[name]
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


def deviation(out, ref):
    """(max |delta| / scale, sum of squares of delta / scale, count): scale = max(1, max |ref|) per board and tensor."""
    scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    d = (out.astype(np.float64) - ref) / scale
    return float(np.abs(d).max()), float((d ** 2).sum()), d.size


def max_and_rms(s, p, ref_s, ref_p):
    (ms, qs, ns), (mp, qp, n_p) = deviation(s, ref_s), deviation(p, ref_p)
    return max(ms, mp), float(np.sqrt((qs + qp) / (ns + n_p)))


def assert_bf16(s, p, ref_s, ref_p, what):
    worst, rms = max_and_rms(s, p, ref_s, ref_p)
    print(f"[bf16] {what}: max |delta| / scale = {worst:.3e}, rms = {rms:.3e}")
    assert np.isfinite(s).all() and np.isfinite(p).all()
    assert worst <= BF16_REL, f"{what}: max |delta| / scale = {worst:.3e} > {BF16_REL}"
    assert rms <= BF16_RMS, f"{what}: rms |delta| / scale = {rms:.3e} > {BF16_RMS}"
    return worst, rms


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n[0] for n in NETS])
def test_parity_with_the_oracle(dev, name):
    r = Ref.get(name)
    model = capi.Model(blob=r.blob)
    eng = capi.Engine(model, dev, MAX_BATCH, BF16)
    assert eng.tower_path == r.path
    assert eng.launch_geometry(BATCH) == ((BATCH + r.per - 1) // r.per, r.per)
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    # the f16 engine of the same network on the same boards: the ratio of the two rms deviations
    s16, p16 = capi.Engine(model, dev, MAX_BATCH, F16).eval_packed(r.bits, r.scalars_in)
    worst16, rms16 = max_and_rms(s16, p16, r.s, r.p)
    worst, rms = max_and_rms(s, p, r.s, r.p)
    print(f"[bf16 / f16] {name}: bf16 max {worst:.3e} rms {rms:.3e}; f16 max {worst16:.3e} rms {rms16:.3e}; rms ratio {rms / rms16:.2f}")
    assert_bf16(s, p, r.s, r.p, name)
    assert RATIO_MIN <= rms / rms16 <= RATIO_MAX, f"{name}: bf16 rms / f16 rms = {rms / rms16:.2f}"
    # a prefix batch: the same boards, another grid and a ragged last workgroup
    s_pre, p_pre = eng.eval_packed(r.bits[:PREFIX], r.scalars_in[:PREFIX])
    assert np.array_equal(s_pre, s[:PREFIX]) and np.array_equal(p_pre, p[:PREFIX])
    if r.wide:
        # the wide tiles: an engine and a batch that fill the chip with workgroups of more boards; the same boards, repeated
        max_batch, boards, per = r.wide
        wide = capi.Engine(model, dev, max_batch, BF16)
        assert wide.tower_path == r.path
        assert wide.launch_geometry(boards) == ((boards + per - 1) // per, per)
        pick = np.arange(boards) % BATCH
        s_w, p_w = wide.eval_packed(r.bits[pick], r.scalars_in[pick])
        assert np.array_equal(s_w, s[pick]) and np.array_equal(p_w, p[pick])


# ---- 2. exact networks ----------------------------------------------------------------------------------------------------
BF16_STEPS = 128  # half of what bf16's 8 significant bits hold


def within_bf16(report, tensors):
    """Every tensor the launch stores as bf16 (the input planes, the stream, the mid activations, the tower output, with the
    heads inside the policy head's hidden layer) and every weight of its stream within BF16_STEPS steps."""
    stored = {k: v for k, (v, _) in report.stored.items() if k == "input" or k.startswith("tower.") or k == "policy_head.hidden"}
    weights = {k: float(np.abs(v).max() / E.step_of(v)) for k, v in tensors.items()
               if k.endswith(".weight") and v.ndim == 4 and (k.startswith("common.tower.") or k == "policy_head.seq.0.weight")}
    assert stored and weights
    return max(stored.values()) <= BF16_STEPS and max(weights.values()) <= BF16_STEPS, stored, weights


# The committed generator at depth 2, its own boards and seed: without a dense layer, and with the dense layer at every position
# that keeps the condition (checked on the CPU; the test asserts it again).  A dense 3x3 layer inside the tower sums 1152 or
# 2304 non-zero terms and leaves 360 .. 920 steps behind it — more than bf16 holds — so those positions stay with the f16 /
# f32 / split16 engines of tests/test_gpu_exact.py; the sparse tower layers here still put two weights per row at random
# (channel, tap) positions of every layer's bf16 stream.  Dense: the chess stem (0), the scalar head's 1x1 convolution, which
# reads every channel of the bf16 tower output (5; with the heads inside that is the in-launch f32 tail), its Linears (7),
# the policy head's last layers (8, 9).
EXACT = [(game, channels, head, path, per, dense_at)
         for game, channels, head, path, per, positions in [("ataxx-7", 128, "ataxx_conv", HEADS_IN, 2, (None, 5, 7, 9)),
                                                            ("chess", 256, "attention", HEADS_OUT, 1, (None, 0, 5, 8))]
         for dense_at in positions]


@pytest.mark.parametrize("game,channels,head,path,per,dense_at", EXACT, ids=[f"{e[0]}x{e[1]}-dense-{e[5]}" for e in EXACT])
def test_exact_networks_return_the_float64_bits(dev, game, channels, head, path, per, dense_at):
    boards = E.exact_boards(game, E.BOARDS, E.SEED)
    meta, tensors, _, (ref_s, ref_p, report) = E.draw_exact(game, 2, channels, head, dense_at, E.SEED, boards=boards)
    ok, stored, weights = within_bf16(report, tensors)
    assert ok, (stored, weights)
    ref_s, ref_p = ref_s.astype(np.float32), ref_p.astype(np.float32)
    eng = capi.Engine(capi.Model(blob=write_model(meta, tensors)), dev, MAX_BATCH, BF16)
    assert eng.tower_path == path
    for n in (E.BOARDS, 1, per + 1):  # ragged: the last workgroup holds fewer boards than the others
        s, p = eng.eval_packed(boards[0][:n], boards[1][:n])
        assert np.array_equal(s, ref_s[:n]), f"scalars, {n} boards: max |d| {np.abs(s - ref_s[:n]).max():g}"
        assert np.array_equal(p, ref_p[:n]), f"policy, {n} boards: {int((p != ref_p[:n]).sum())} of {p.size} differ, max |d| {np.abs(p - ref_p[:n]).max():g}"


# ---- 3. range -------------------------------------------------------------------------------------------------------------
S = 2.0 ** 12


def scaled_stream(blob):
    """The same function with the residual stream S times as large: the stem's weights and bias times S, every block's
    (folded) bias times S, the final BN's running mean times S and its variance times S^2.  bn_eps is one number for the whole
    network, so it goes up by S^2 with the final BN's variance — and every block BatchNorm takes the scaling that keeps its
    fold (conv bias - mean) * k + beta, k = gamma / sqrt(var + eps), the same function of an S times larger input: conv bias,
    mean and beta times S (the folded bias times S), var times S^2 and gamma times S (k unchanged).  Powers of two throughout:
    the oracle returns the unscaled network's bits."""
    meta, t = read_model(blob)
    t = {k: v.copy() for k, v in t.items()}
    depth, s1, s2 = meta["tower_depth"], np.float32(S), np.float32(S * S)
    t["common.tower.0.weight"] *= s1
    t["common.tower.0.bias"] *= s1
    for i in range(1, depth + 1):
        for conv, bn in ((0, 1), (3, 4)):
            t[f"common.tower.{i}.seq.{conv}.bias"] *= s1
            for n in ("weight", "bias", "running_mean"):
                t[f"common.tower.{i}.seq.{bn}.{n}"] *= s1
            t[f"common.tower.{i}.seq.{bn}.running_var"] *= s2
    t[f"common.tower.{depth + 1}.running_mean"] *= s1
    t[f"common.tower.{depth + 1}.running_var"] *= s2
    meta = dict(meta)
    meta["bn_eps"] = float(np.float32(meta["bn_eps"]) * s2)
    return write_model(meta, t)


def test_range_beyond_f16(dev):
    r = Ref.get("chess256")
    blob = scaled_stream(r.blob)
    # on the CPU: the same outputs (the oracle's own 2e-5), and a stream — stem output and block 1's output are the two
    # stream tensors every f16 kernel stores — past 65504 on every board
    s_ref, p_ref, acts = O.OracleNet(blob).forward_trace(r.x)
    assert np.abs(s_ref - r.s).max() <= 2e-5 and np.abs(p_ref - r.p).max() <= 2e-5
    per_board = np.maximum(np.abs(acts["tower.0"]).reshape(BATCH, -1).max(axis=1), np.abs(acts["tower.1"]).reshape(BATCH, -1).max(axis=1))
    print(f"[range] stored stream, max per board: {per_board.min():.0f} .. {per_board.max():.0f}")
    assert per_board.min() > 65504.0
    rng = np.random.default_rng(9)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    model = capi.Model(blob=blob)
    for dtype, path in ((F16, "tower_resident_f16+heads"), (SPLIT16, "tower_resident_split16+heads")):
        eng = capi.Engine(model, dev, MAX_BATCH, dtype)
        assert eng.tower_path == path
        _, _, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, moves)
        assert ((status & capi.KZ_BOARD_NONFINITE) != 0).all(), (path, status)
    eng = capi.Engine(model, dev, MAX_BATCH, BF16)
    assert eng.tower_path == HEADS_OUT
    _, _, status = eng.eval_packed_decoded_status(r.bits, r.scalars_in, moves)
    assert (status == 0).all(), status
    s, p = eng.eval_packed(r.bits, r.scalars_in)
    assert_bf16(s, p, r.s, r.p, "scaled chess256")


# ---- 4. engine surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "chess192"])
def test_decoded_entries_on_all_slots(dev, name):
    """submit_packed_decoded on the four slots, then the four waits: the decode inside the launch (+heads) and the stand-alone
    decode behind the f32 head kernels against the host decode of the engine's own scalars and logits."""
    r = Ref.get(name)
    eng = capi.Engine(capi.Model(blob=r.blob), dev, MAX_BATCH, BF16)
    assert eng.tower_path == r.path
    rng = np.random.default_rng(21)
    valid = np.arange(r.policy_len)
    jobs = []
    for slot in range(4):
        lo, n = 5 * slot, 7 + 5 * slot  # overlapping slices of the boards, a different batch per slot
        moves = [rng.permutation(valid)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=n)]
        jobs.append((slot, lo, n, moves, eng.submit_packed_decoded(slot, r.bits[lo:lo + n], r.scalars_in[lo:lo + n], moves)))
    got = [eng.wait_decoded(slot, offsets) for slot, _, _, _, offsets in jobs]
    for (slot, lo, n, moves, _), (values, probs) in zip(jobs, got):
        s, p = eng.eval_packed(r.bits[lo:lo + n], r.scalars_in[lo:lo + n])
        v_ref, p_ref = O.decode_output(s, p, moves)
        assert np.abs(values[:, :4] - v_ref[:, :4]).max() <= 1e-5, slot
        assert np.abs(values[:, 4] - v_ref[:, 4]).max() <= 1e-5 * max(1.0, float(np.abs(v_ref[:, 4]).max())), slot
        assert all(a.shape == b.shape for a, b in zip(probs, p_ref))
        assert max(float(np.abs(a - b).max()) for a, b in zip(probs, p_ref)) <= 1e-5, slot


def test_sym_entry_is_the_host_side_wrapper(dev):
    from tests.test_gpu_symmetry import Case
    case = Case(dev, "ataxx-7", 2, 128, "ataxx_conv", BF16, HEADS_IN, MAX_BATCH, tables="ataxx")
    for slot, (batch, seed) in enumerate([(BATCH, 1), (9, 2)]):
        case.check(batch, seed, slot=slot)


def test_audit_against_exact_f32(dev):
    r = Ref.get("ataxx7x128")
    eng = capi.Engine(capi.Model(blob=r.blob), dev, MAX_BATCH, BF16)
    with pytest.raises(capi.KzError, match="dtype must be"):  # (bf16 is no yardstick: not for itself either)
        eng.set_audit(BF16, 1, 16)
    eng.set_audit(SPLIT16, 1, 16)  # (either exact sibling is accepted)
    eng.set_audit(F32, 1, 16)
    eng.set_range_fallback(F32)  # keeps working: accepted, and with nothing to catch it changes nothing
    rng = np.random.default_rng(4)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=BATCH)]
    values, _ = eng.wait_decoded(0, eng.submit_packed_decoded(0, r.bits, r.scalars_in, moves))
    stats = eng.audit_stats()
    print(f"[audit] {stats!r}")
    assert stats.batches == 1 and stats.boards == 16 and stats.skipped == 0
    assert stats.moves == sum(len(m) for m in moves[:16])
    assert stats.max_abs_prob <= BF16_REL  # (a probability's scale is 1)
    scale = np.maximum(1.0, np.abs(values[:16]).max(axis=0))
    assert (stats.max_abs_value <= BF16_REL * scale).all(), (stats.max_abs_value, scale)
    assert stats.max_abs_prob > 0 and stats.max_abs_value.max() > 0  # bf16 against exact f32: the audit saw the difference
