"""The shadow audit on the GPU (include/kz_hip.h: kz_engine_set_audit, kz_engine_audit_stats).

Every case builds three engines of one model with max_batch 32: A, the engine under audit; B, the same dtype without the audit;
C, the audit's dtype without the audit.  The batches are ragged (21 boards, some of them finished games) and the audit samples
8.  What A must have accumulated is computed here from B's and C's outputs on the first 8 boards of every audited batch, in the
order the header fixes — per compared board the five values, then the probabilities in the caller's move order; d = |b - c| in
f32, a running f32 maximum, a running f64 sum of (double)d * (double)d, one term after the other (a plain loop: np.sum adds
pairwise) — and every field is compared with ==.  No tolerance appears: the engines are deterministic and the order is specified.
A's own results are compared with np.array_equal to B's: the audit changes nothing."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E
from tests.test_gpu_symmetry import ataxx_tables, move_lists

pytestmark = pytest.mark.gpu

F16, F32, SPLIT16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16
OK, BAD_DECODE, NONFINITE, FELL_BACK = capi.KZ_BOARD_OK, capi.KZ_BOARD_BAD_DECODE, capi.KZ_BOARD_NONFINITE, capi.KZ_BOARD_FELL_BACK
MAX_BATCH, BATCH, BOARDS = 32, 21, 8
FINISHED = (3, 10, 20)  # finished games: no moves (one of them among the sampled boards)
SOFTMAX_MSG = "Softmax input sum must be strictly positive"


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Expect:
    """The statistics, accumulated the way the header says."""

    def __init__(self):
        self.batches = self.boards = self.moves = self.skipped = 0
        self.max_abs_value = np.zeros(5, np.float32)
        self.max_abs_prob = np.float32(0)
        self.sum_sq_value = [0.0] * 5
        self.sum_sq_prob = 0.0

    def add(self, b, c, k):
        """One audited batch that was returned: b = B's (values, probs, status) on the batch, c = C's on its first k boards."""
        (vb, pb, sb), (vc, pc, sc) = b, c
        assert len(sc) == k and vb.dtype == np.float32 and vc.dtype == np.float32
        self.batches += 1
        for i in range(k):
            if sb[i] != OK or sc[i] != OK:
                self.skipped += 1
                continue
            self.boards += 1
            for col in range(5):
                d = np.abs(vb[i, col] - vc[i, col])
                assert d.dtype == np.float32
                self.max_abs_value[col] = max(self.max_abs_value[col], d)
                self.sum_sq_value[col] += float(d) * float(d)
            assert pb[i].dtype == np.float32 and pb[i].shape == pc[i].shape
            for j in range(len(pb[i])):
                d = np.abs(pb[i][j] - pc[i][j])
                self.max_abs_prob = max(self.max_abs_prob, d)
                self.sum_sq_prob += float(d) * float(d)
            self.moves += len(pb[i])

    def check(self, got):
        print(f"[audit] expected batches {self.batches} boards {self.boards} moves {self.moves} skipped {self.skipped} "
              f"max|dv| {self.max_abs_value.tolist()} max|dp| {float(self.max_abs_prob)} sum_sq_prob {self.sum_sq_prob}; got {got}")
        assert (got.batches, got.boards, got.moves, got.skipped) == (self.batches, self.boards, self.moves, self.skipped)
        for col in range(5):
            assert got.max_abs_value[col] == self.max_abs_value[col], col
            assert got.sum_sq_value[col] == self.sum_sq_value[col], col
        assert got.max_abs_prob == self.max_abs_prob
        assert got.sum_sq_prob == self.sum_sq_prob


def assert_zero(stats):
    assert (stats.batches, stats.boards, stats.moves, stats.skipped) == (0, 0, 0, 0)
    assert not stats.max_abs_value.any() and not stats.sum_sq_value.any() and stats.max_abs_prob == 0 and stats.sum_sq_prob == 0


class Case:
    """A model, its three engines, and 21 boards with their move lists."""

    def __init__(self, dev, blob, game, dtype, against, path, seed=5, valid=None):
        g = synth.game_spec(game)
        self.policy_len = g["policy_len"]
        self.model = capi.Model(blob=blob)
        assert self.model.plan(MAX_BATCH, dtype)[0] == path
        self.a = capi.Engine(self.model, dev, MAX_BATCH, dtype)
        self.b = capi.Engine(self.model, dev, MAX_BATCH, dtype)
        self.c = capi.Engine(self.model, dev, MAX_BATCH, against)  # (the sibling's max_batch: min(64, 32))
        assert self.a.tower_path == path and self.b.tower_path == path
        self.against = against
        rng = np.random.default_rng(seed + 100)
        self.bits, self.scalars = synth.random_boards(game, BATCH, seed=seed + 1)
        self.moves = move_lists(rng, np.arange(self.policy_len) if valid is None else valid, BATCH, finished=FINISHED[0])
        for f in FINISHED[1:]:
            self.moves[f] = np.zeros(0, np.int32)

    def batch(self, shift=0, n=BATCH):
        """n boards of the 21, starting at board `shift` (cyclically): (bits, scalars, moves)."""
        idx = (np.arange(n) + shift) % BATCH
        return self.bits[idx], self.scalars[idx], [self.moves[i] for i in idx]

    @staticmethod
    def run(eng, slot, batch, k=None, sym=None):
        """The first k boards of a batch through the plain / _sym entry with the status wait."""
        bits, scalars, moves = batch
        k = len(moves) if k is None else k
        off = eng.submit_packed_decoded(slot, bits[:k], scalars[:k], moves[:k], sym=None if sym is None else sym[:k])
        return eng.wait_decoded_status(slot, off)


def same(x, y):
    """(values, probs[, status]) of two engines, bit for bit."""
    return (np.array_equal(x[0], y[0]) and len(x[1]) == len(y[1]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1])) and
            (len(x) < 3 or np.array_equal(x[2], y[2])))


def random_net(game, depth, channels, head, **kw):
    return synth.random_model(game, depth, channels, head, seed=5, **kw)


ATAXX = ("ataxx-7", 3, 128, "ataxx_conv", {})
CASES = [
    (("chess", 2, 256, "attention", {}), F16, F32, "tower_resident_f16+heads"),
    (("chess", 2, 256, "attention", {}), F16, SPLIT16, "tower_resident_f16+heads"),
    (ATAXX, F16, F32, "tower_resident_f16g+heads"),
    (ATAXX, SPLIT16, F32, "tower_resident_split16+heads"),
    (("go-19", 2, 64, "conv", {}), F16, F32, "conv_igemm_f16"),  # one launch per layer, the stand-alone kz_decode_output
    (("chess", 2, 128, "dense", {"attention": (8, 16, 16, 128)}), F16, F32, "attention_tower_f16"),
]
IDS = ["chess_f16_vs_f32", "chess_f16_vs_split16", "ataxx_f16_vs_f32", "ataxx_split16_vs_f32", "go19_f16_vs_f32", "attention_tower_f16_vs_f32"]


@pytest.mark.parametrize("net,dtype,against,path", CASES, ids=IDS)
def test_reproduction_and_nothing_changes(dev, net, dtype, against, path):
    """Three batches on slots 0-2, all submitted before any wait, period 1: the statistics are the expectation, and A's results
    and status bytes are B's — through kz_engine_wait_decoded and through kz_engine_wait_decoded_status."""
    game, depth, channels, head, kw = net
    c = Case(dev, random_net(game, depth, channels, head, **kw), game, dtype, against, path)
    if not c.model.supports_dtype(SPLIT16):  # (the AttentionTower network: no split16 kernels to audit against)
        with pytest.raises(capi.KzError, match="kz_engine_set_audit: this model has no KZ_DTYPE_F32_SPLIT16 kernels"):
            c.a.set_audit(SPLIT16, 1, BOARDS)
        with pytest.raises(capi.KzError, match="the audit is off"):
            c.a.audit_stats()
    c.a.set_audit(against, 1, BOARDS)
    assert_zero(c.a.audit_stats())
    batches = [c.batch(shift) for shift in (0, 5, 11)]
    offs = {}
    for eng in (c.a, c.b):
        for slot, (bits, scalars, moves) in enumerate(batches):
            offs[eng, slot] = eng.submit_packed_decoded(slot, bits, scalars, moves)
    with pytest.raises(capi.KzError, match="an audited batch is in flight"):
        c.a.audit_stats()
    order = (1, 0, 2)  # the order the batches are returned in is the order they accumulate in
    out_b = {}
    for slot in order:
        if slot == 1:
            got, out_b[slot] = c.a.wait_decoded_status(slot, offs[c.a, slot]), c.b.wait_decoded_status(slot, offs[c.b, slot])
            assert not got[2].any()
        else:
            got = c.a.wait_decoded(slot, offs[c.a, slot])
            out_b[slot] = c.b.wait_decoded(slot, offs[c.b, slot]) + (np.zeros(BATCH, np.uint8),)
        assert same(got, out_b[slot][:len(got)]), f"slot {slot}: the audit changed a result"
    expect = Expect()
    for slot in order:
        expect.add(out_b[slot], Case.run(c.c, 0, batches[slot], BOARDS), BOARDS)
    stats = c.a.audit_stats()
    expect.check(stats)
    assert stats.batches == 3 and stats.boards == 3 * BOARDS and stats.skipped == 0
    if dtype == F16:
        assert stats.max_abs_prob > 0, "f16 against a <= 1e-4 arithmetic: the audit compared nothing?"
    assert stats.rms_prob == float(np.sqrt(expect.sum_sq_prob / expect.moves))


def test_period_counts_decoded_submits_with_boards(dev):
    """Period 3 over 7 submits: submits 1, 4 and 7 are audited; a batch == 0 submit in between does not count.  The synchronous
    form goes through the same count."""
    c = Case(dev, random_net(*ATAXX[:4]), "ataxx-7", F16, F32, "tower_resident_f16g+heads")
    c.a.set_audit(F32, 3, BOARDS)
    sizes = [21, 5, 21, 3, 21, 21, 9]
    expect = Expect()
    for n, size in enumerate(sizes):
        batch = c.batch(n, size)
        if n == 2:  # an empty submit between number 2 and number 3
            v, p, st = c.a.wait_decoded_status(1, c.a.submit_packed_decoded(1, c.bits[:0], c.scalars[:0], []))
            assert v.shape == (0, 5) and p == [] and st.shape == (0,)
        ref = Case.run(c.b, 0, batch)
        if n % 2:
            got = c.a.eval_packed_decoded(*batch)  # kz_engine_eval_packed_decoded
            assert same(got, ref[:2])
        else:
            assert same(Case.run(c.a, n % capi.KZ_ENGINE_SLOTS, batch), ref)
        if n % 3 == 0:
            k = min(BOARDS, size)
            expect.add(ref, Case.run(c.c, 0, batch, k), k)
    stats = c.a.audit_stats()
    assert stats.batches == 3 and stats.boards == 8 + 3 + 8
    expect.check(stats)


def test_sym_and_avg_entries(dev):
    """Ataxx D4 (n_sym 8): a `_sym` batch is audited with the same ids, an averaged batch through the averaged entry —
    min(8, batch, 32 // 8) = 4 boards of it.  The tables reach the sibling both ways: set before the audit, and after."""
    square_src, policy_map = ataxx_tables(7)
    valid = np.flatnonzero((policy_map >= 0).all(axis=0))
    c = Case(dev, random_net(*ATAXX[:4]), "ataxx-7", F16, F32, "tower_resident_f16g+heads", valid=valid)
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 8, size=BATCH).astype(np.uint8)
    c.a.set_symmetries(square_src, policy_map)  # handed to the sibling by set_audit
    c.a.set_audit(F32, 1, BOARDS)
    for eng in (c.b, c.c):
        eng.set_symmetries(square_src, policy_map)
    expect = Expect()
    batch = c.batch(2)
    ref = Case.run(c.b, 0, batch, sym=ids)
    assert same(Case.run(c.a, 2, batch, sym=ids), ref)
    expect.add(ref, Case.run(c.c, 0, batch, BOARDS, sym=ids), BOARDS)
    expect.check(c.a.audit_stats())
    assert expect.max_abs_prob > 0

    c.a.set_symmetries(square_src, policy_map)  # ... and through kz_engine_set_symmetries afterwards

    def avg(eng, slot, b, k):
        off = eng.submit_packed_decoded_avg(slot, b[0][:k], b[1][:k], b[2][:k])
        return eng.wait_decoded_status(slot, off)

    for shift, size in ((0, 4), (7, 3)):  # (an engine of 32 takes 32 // 8 = 4 boards per averaged call)
        batch = c.batch(shift, size)
        ref = avg(c.b, 1, batch, size)
        assert same(avg(c.a, 3, batch, size), ref)
        expect.add(ref, avg(c.c, 1, batch, size), size)
    got = c.a.eval_packed_decoded_avg(*c.batch(3, 4))  # the synchronous averaged form counts too
    ref = avg(c.b, 1, c.batch(3, 4), 4)
    assert same(got, ref[:2])
    expect.add(ref, avg(c.c, 1, c.batch(3, 4), 4), 4)
    stats = c.a.audit_stats()
    assert stats.batches == 4 and stats.boards == 8 + 4 + 3 + 4
    expect.check(stats)


@pytest.mark.parametrize("net,game,path", [("chess_2x256_att", "chess", "tower_resident_f16+heads"),
                                           ("ataxx7_1x128", "ataxx-7", "tower_resident_f16g+heads")], ids=["chess", "ataxx"])
def test_exact_network_has_zero_deviation(dev, net, game, path):
    """A network on which no arithmetic rounds (tests/exact_nets.py): f16 audited against exact f32 deviates by exactly 0."""
    b = E.build(net, None)
    model = capi.Model(blob=b.blob)
    eng = capi.Engine(model, dev, MAX_BATCH, F16)
    assert eng.tower_path == path
    eng.set_audit(F32, 1, BOARDS)
    rng = np.random.default_rng(3)
    idx = np.arange(3, 3 + BATCH) % E.BOARDS
    moves = move_lists(rng, np.arange(synth.game_spec(game)["policy_len"]), BATCH, finished=FINISHED[0])
    v, p, st = eng.wait_decoded_status(0, eng.submit_packed_decoded(0, b.bits[idx], b.scalars_in[idx], moves))
    assert not st.any()
    stats = eng.audit_stats()
    print(f"[audit] exact {net}: {stats}")
    assert stats.batches == 1 and stats.boards == BOARDS and stats.boards > 0 and stats.moves > 0 and stats.skipped == 0
    assert all(float(x) == 0.0 for x in stats.max_abs_value) and all(float(x) == 0.0 for x in stats.sum_sq_value)
    assert float(stats.max_abs_prob) == 0.0 and stats.sum_sq_prob == 0.0


def test_skipped_boards(dev):
    c = Case(dev, random_net(*ATAXX[:4]), "ataxx-7", F16, F32, "tower_resident_f16g+heads")
    c.a.set_audit(F32, 1, BOARDS)
    # a move index outside the policy on board 2: skipped, the other seven compared, and the call fails as it does without the audit
    bits, scalars, moves = c.batch()
    moves = [m.copy() for m in moves]
    moves[2][0] = c.policy_len
    messages = []
    for eng in (c.a, c.b):
        with pytest.raises(capi.KzError, match=SOFTMAX_MSG) as err:
            eng.wait_decoded(0, eng.submit_packed_decoded(0, bits, scalars, moves))
        messages.append(str(err.value))
    assert messages[0] == messages[1]
    ref = Case.run(c.b, 0, (bits, scalars, moves))
    assert ref[2][2] == BAD_DECODE and np.flatnonzero(ref[2]).tolist() == [2]
    expect = Expect()
    expect.add(ref, Case.run(c.c, 0, (bits, scalars, moves), BOARDS), BOARDS)
    stats = c.a.audit_stats(reset=True)
    assert stats.skipped == 1 and stats.boards == BOARDS - 1 and stats.batches == 1
    expect.check(stats)
    assert_zero(c.a.audit_stats())
    # the range fallback beside the audit: board 1 leaves the f16 range (finite in f32), comes back fell-back, and is skipped
    c.a.set_range_fallback(F32)
    bits, scalars, moves = c.batch()
    scalars = scalars.copy()
    scalars[1, 0] = 3e5
    got = Case.run(c.a, 1, (bits, scalars, moves))
    assert got[2][1] == FELL_BACK and np.flatnonzero(got[2]).tolist() == [1]
    v, p = c.a.wait_decoded(2, c.a.submit_packed_decoded(2, bits, scalars, moves))  # the batch succeeds
    assert same((v, p), got[:2])
    ref = Case.run(c.b, 0, (bits, scalars, moves))
    assert ref[2][1] & NONFINITE and np.flatnonzero(ref[2]).tolist() == [1]
    assert all(np.array_equal(got[0][i], ref[0][i]) and np.array_equal(got[1][i], ref[1][i]) for i in range(BATCH) if i != 1)
    ref32 = Case.run(c.c, 0, (bits, scalars, moves), BOARDS)
    assert not ref32[2].any()
    expect = Expect()
    expect.add(ref, ref32, BOARDS)
    expect.add(ref, ref32, BOARDS)
    stats = c.a.audit_stats()
    assert stats.skipped == 2 and stats.boards == 2 * (BOARDS - 1)
    expect.check(stats)


def test_refusals_and_lifecycle(dev):
    c = Case(dev, random_net(*ATAXX[:4]), "ataxx-7", F16, F32, "tower_resident_f16g+heads")
    a = c.a
    batch = c.batch()
    with pytest.raises(capi.KzError, match="kz_engine_audit_stats: the audit is off"):
        a.audit_stats()
    refusals = {}

    def refused(key, eng, *args):
        with pytest.raises(capi.KzError, match="kz_engine_set_audit: ") as err:
            eng.set_audit(*args)
        refusals[key] = str(err.value)

    split = capi.Engine(c.model, dev, MAX_BATCH, SPLIT16)
    refused("own", split, SPLIT16, 1, BOARDS)
    refused("own f32", c.c, F32, 1, BOARDS)
    refused("f16", a, F16, 1, BOARDS)
    refused("other", a, 7, 1, BOARDS)
    refused("period", a, F32, 0, BOARDS)
    refused("boards 0", a, F32, 1, 0)
    refused("boards 33", a, F32, 1, MAX_BATCH + 1)
    off = a.submit_packed_decoded(3, *batch)
    refused("in flight", a, F32, 1, BOARDS)
    refused("in flight, off", a, -1, 0, 0)
    a.wait_decoded(3, off)
    print("\n".join(f"[audit] {k}: {v}" for k, v in refusals.items()))
    assert "evaluates in that dtype already" in refusals["own"] and refusals["own"] == refusals["own f32"]
    assert "dtype must be" in refusals["f16"] and "got 1" in refusals["f16"] and "got 7" in refusals["other"]
    assert "period 0 must be at least 1" in refusals["period"]
    assert "boards 0 must be in 1..32" in refusals["boards 0"] and "boards 33 must be in 1..32" in refusals["boards 33"]
    assert "a batch is in flight" in refusals["in flight"] and refusals["in flight"] == refusals["in flight, off"]
    # one message per cause
    assert len({refusals[k].split(", got")[0] for k in ("own", "f16", "period", "boards 0", "in flight")}) == 5
    with pytest.raises(capi.KzError, match="the audit is off"):  # none of the refused calls turned it on
        a.audit_stats()
    assert same(Case.run(a, 0, batch), Case.run(c.b, 0, batch))

    a.set_audit(F32, 1, MAX_BATCH)  # boards = the sibling's max_batch: the whole batch of 21
    assert capi.load().kz_engine_audit_stats(a._h, None, 0) != 0
    assert capi.load().kz_last_error().decode() == "kz_engine_audit_stats: null output"
    Case.run(a, 0, batch)
    stats = a.audit_stats()
    assert stats.batches == 1 and stats.boards == BATCH
    assert a.audit_stats(reset=True).boards == BATCH  # reset hands out the totals, then zeroes them
    assert_zero(a.audit_stats())
    Case.run(a, 1, batch)
    assert a.audit_stats().batches == 1
    a.set_audit(F32, 2, BOARDS)  # on twice: new settings, zeroed statistics, the count starts over
    assert_zero(a.audit_stats())
    Case.run(a, 0, batch)
    Case.run(a, 0, batch)
    stats = a.audit_stats()
    assert stats.batches == 1 and stats.boards == BOARDS
    a.set_audit(SPLIT16, 1, BOARDS)  # another arithmetic: another sibling
    assert_zero(a.audit_stats())
    ref = Case.run(c.b, 0, batch)
    assert same(Case.run(a, 0, batch), ref)
    expect = Expect()
    expect.add(ref, Case.run(split, 0, batch, BOARDS), BOARDS)
    expect.check(a.audit_stats())
    a.set_audit(-1, 0, 0)  # off: period and boards are ignored, and A is B again
    with pytest.raises(capi.KzError, match="the audit is off"):
        a.audit_stats()
    assert same(Case.run(a, 0, batch), ref)
    a.set_audit(-1, 1, 1)  # (off twice is off)
