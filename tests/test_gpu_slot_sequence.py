"""What a slot has in flight, across kinds: the four host-pointer submits (raw, decoded, decoded with symmetry ids, averaged)
share one body and one in-flight record per slot (kz_engine.hip: submit, InFlight), and every call that returns a batch reads
that record.  This file runs the kinds side by side and one after the other on the same slots, so that nothing of the batch a
slot held before — its kind, where its range words lie, whether it was averaged — may leak into the next.

An invariance check between entries, not a parity test: every result is compared bit for bit (np.array_equal) with the same
boards through the blocking `eval_*` entry of the matching kind on a FRESH engine of the same model.  Parity with the oracle
stays with tests/test_gpu_parity.py, tests/test_gpu_symmetry*.py and tests/test_gpu_board_status.py.

Two networks, the smallest the averaged-symmetry tests build (synth seed 5), both at max_batch 16 with the 8 Ataxx symmetries
(an averaged batch is at most 2 boards):
  Ataxx 7x7 2x128 f16  tower_resident_f16g+heads  one launch with the heads and the decode inside, zero copy, two streams
  Ataxx 7x7 2x64  f16  tower_resident_f16g        heads and kz_decode_output as launches of their own, one stream, staged copies
The out-of-range board is tests/test_gpu_board_status.py's: scalars_in[b, 0] = 3e5, finite in f32 and inf as f16."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests.test_gpu_symmetry import ataxx_tables, move_lists

pytestmark = pytest.mark.gpu

F16, F32 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32
MAX_BATCH = 16
KINDS = ["raw", "decoded", "ids", "avg"]
SIZES = {"raw": 4, "decoded": 3, "ids": 5, "avg": 2}
# the ids of the two rounds cover 0..7 between them
IDS = [np.array([0, 3, 5, 7, 2], np.uint8), np.array([1, 4, 6, 7, 0], np.uint8)]
BAD_BOARD = 1  # of the decoded batch, in the fallback round


class World:
    """An engine under test, a fresh engine for the blocking references, and one fixed input per kind."""

    def __init__(self, dev, channels, path):
        self.model = capi.Model(blob=synth.random_model("ataxx-7", 2, channels, "ataxx_conv", seed=5))
        self.tables = ataxx_tables(7)
        self.dev = dev
        self.eng = self.engine(F16)
        assert self.eng.tower_path == path
        self.fresh = self.engine(F16)
        valid = np.flatnonzero((self.tables[1] >= 0).all(axis=0))  # moves with an image under every symmetry
        self.inputs, self.refs = {}, {}
        for i, kind in enumerate(KINDS):
            n = SIZES[kind]
            rng = np.random.default_rng(200 + i)
            bits, scalars = synth.random_boards("ataxx-7", n, seed=71 + i)
            self.inputs[kind] = (bits, scalars, move_lists(rng, valid, n, finished=n - 1))

    def engine(self, dtype):
        eng = capi.Engine(self.model, self.dev, MAX_BATCH, dtype)
        eng.set_symmetries(*self.tables)
        return eng

    def submit(self, slot, kind, ids=IDS[0], scalars=None, eng=None):
        eng = eng or self.eng
        bits, s, moves = self.inputs[kind]
        s = s if scalars is None else scalars
        if kind == "raw":
            return eng.submit_packed(slot, bits, s)
        if kind == "avg":
            return eng.submit_packed_decoded_avg(slot, bits, s, moves)
        return eng.submit_packed_decoded(slot, bits, s, moves, sym=ids if kind == "ids" else None)

    def wait(self, slot, kind, token):
        """(values or scalars, probs or policy, status or None)"""
        if kind == "raw":
            return self.eng.wait(slot, token) + (None,)
        return self.eng.wait_decoded_status(slot, token)

    def ref(self, kind, ids=IDS[0]):
        """The blocking entry of the matching kind on the fresh engine; computed once per (kind, ids)."""
        key = (kind, ids.tobytes() if kind == "ids" else None)
        if key not in self.refs:
            bits, s, moves = self.inputs[kind]
            if kind == "raw":
                self.refs[key] = self.fresh.eval_packed(bits, s)
            elif kind == "avg":
                self.refs[key] = self.fresh.eval_packed_decoded_avg(bits, s, moves)
            else:
                self.refs[key] = self.fresh.eval_packed_decoded(bits, s, moves, sym=ids if kind == "ids" else None)
        return self.refs[key]


def same(kind, got, ref, skip=()):
    if kind == "raw":
        return np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    boards = [b for b in range(len(ref[0])) if b not in skip]
    return len(got[1]) == len(ref[1]) and all(np.array_equal(got[0][b], ref[0][b]) and np.array_equal(got[1][b], ref[1][b]) for b in boards)


@pytest.fixture(scope="module", params=[(128, "tower_resident_f16g+heads"), (64, "tower_resident_f16g")], ids=["one_launch", "staged"])
def world(request):
    assert capi.device_count() >= 1
    return World(0, *request.param)


def test_four_kinds_in_flight_then_rotated(world):
    w = world
    # round 1: slot k carries KINDS[k]; nobody waits until all four are submitted; waited in another order
    tokens = [w.submit(k, KINDS[k]) for k in range(4)]
    got = {k: w.wait(k, KINDS[k], tokens[k]) for k in (2, 0, 3, 1)}
    for k in range(4):
        assert same(KINDS[k], got[k], w.ref(KINDS[k])), KINDS[k]
        assert got[k][2] is None or (got[k][2].shape == (SIZES[KINDS[k]],) and not got[k][2].any()), KINDS[k]
    # slot 3 has just returned an averaged batch: an empty batch of a decoded kind directly behind it
    bits, scalars, _ = w.inputs["ids"]
    v, p, st = w.eng.wait_decoded_status(3, w.eng.submit_packed_decoded(3, bits[:0], scalars[:0], [], sym=IDS[1][:0]))
    assert v.shape == (0, 5) and p == [] and st.shape == (0,)
    # round 2: the kinds rotated by one slot (slot k carries what slot k - 1 did), other ids; status 0 on every board
    rotated = [KINDS[(k - 1) % 4] for k in range(4)]
    assert rotated[3] == "ids" and all(a != b for a, b in zip(rotated, KINDS))
    tokens = [w.submit(k, rotated[k], ids=IDS[1]) for k in range(4)]
    got = {k: w.wait(k, rotated[k], tokens[k]) for k in (1, 3, 0, 2)}
    for k in range(4):
        assert same(rotated[k], got[k], w.ref(rotated[k], IDS[1])), rotated[k]
        assert got[k][2] is None or (got[k][2].shape == (SIZES[rotated[k]],) and not got[k][2].any()), rotated[k]


def test_range_fallback_names_one_board_of_one_slot(world):
    w = world
    bits, scalars, moves = w.inputs["decoded"]
    bad = scalars.copy()
    bad[BAD_BOARD, 0] = 3e5
    w.eng.set_range_fallback(F32)
    try:
        tokens = [w.submit(k, KINDS[k], scalars=bad if KINDS[k] == "decoded" else None) for k in range(4)]
        got = {k: w.wait(k, KINDS[k], tokens[k]) for k in (3, 1, 0, 2)}
    finally:
        w.eng.set_range_fallback(-1)
    k_dec = KINDS.index("decoded")
    assert got[k_dec][2].tolist() == [capi.KZ_BOARD_FELL_BACK if b == BAD_BOARD else 0 for b in range(SIZES["decoded"])]
    assert same("decoded", got[k_dec], w.ref("decoded"), skip=(BAD_BOARD,))
    # the board that fell back is the exact-f32 engine's
    v32, p32 = w.engine(F32).eval_packed_decoded(bits[BAD_BOARD:BAD_BOARD + 1], bad[BAD_BOARD:BAD_BOARD + 1], [moves[BAD_BOARD]])
    assert np.array_equal(got[k_dec][0][BAD_BOARD], v32[0]) and np.array_equal(got[k_dec][1][BAD_BOARD], p32[0])
    for k in range(4):
        if k != k_dec:
            assert same(KINDS[k], got[k], w.ref(KINDS[k])), KINDS[k]
            assert got[k][2] is None or not got[k][2].any(), KINDS[k]


def test_failed_submit_leaves_the_slot_free(world):
    w = world
    eng, slot = w.eng, 3
    # the slot's last batch was an averaged one
    assert same("avg", w.wait(slot, "avg", w.submit(slot, "avg")), w.ref("avg"))
    bits, scalars, moves = w.inputs["decoded"]
    offsets, idx = capi.Engine._csr(moves)
    wrong = offsets.copy()
    wrong[0] = 1
    with pytest.raises(capi.KzError, match=r"move_offsets\[0\] must be 0"):
        capi.check(capi.load().kz_engine_submit_packed_decoded(eng._h, slot, bits.ctypes.data, bits.shape[1], scalars.ctypes.data,
                                                               len(bits), wrong.ctypes.data, idx.ctypes.data))
    with pytest.raises(capi.KzError, match="nothing submitted with a move list"):  # nothing is in flight on it
        eng.wait_decoded(slot, offsets)
    got = w.wait(slot, "decoded", w.submit(slot, "decoded"))  # no "slot still in flight"
    assert same("decoded", got, w.ref("decoded")) and not got[2].any()
