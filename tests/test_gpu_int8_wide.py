"""The engine surface of a dtype-5 engine ("tower_resident_i8+heads") at the three-board level on Go 9x9: three boards in sixteen
tiles of 16 rows, 342 workgroups and more — the launch geometry of the reference's own loop (Go 9x9 x 128 at batch 2048).
tests/test_gpu_int8_wide_exact.py holds the level's arithmetic to the bit; this file is the contract beside it, on the
networks of tests/test_gpu_int8_heads.py (synth.random_model, depth 2) with the batch tiled from their boards.

1. One launch: N decoded batches are exactly N launches, all named kz_tower_resident_i8, at (342 workgroups, 3 boards).
2. The decoded entries on all four slots, on the exact network go9_3x128 (known logits): ragged lists — all moves, none, and
   lists with repeated indices longer than a wave's staging (a quarter of the X image: 256 rows x 272 B / 16 = 4,352 floats) —
   against the float64 decode within tests/decode_cases.py's derived bounds, status 0 everywhere, every slot the bits of the
   synchronous entry; a board in the MIDDLE of its workgroup with a move index outside the policy gets KZ_BOARD_BAD_DECODE alone.
3. `_sym` with mixed ids: the bits of a narrow dtype-5 engine (max_batch 64, one board per workgroup) on the same boards and ids.
4. Range: the 2^12-scaled stream of an amplifying Go network: the boards the launch flags KZ_BOARD_NONFINITE are exactly the
   boards a narrow engine flags, workgroup mates or not; with the range fallback on they come back KZ_BOARD_FELL_BACK with the
   exact-f32 engine's results.
5. Parity with the CPU oracle within tests/test_gpu_int8.py's own_bounds(MEASURED) of go9x128 — figures measured on dtype 4 on
   the narrow tiles: the wide launch returns the narrow engine's bits (asserted), so no new bound is needed."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import decode_cases as D
from tests import exact_nets as E
from tests import int8_nets as N
from tests.test_gpu_bf16 import max_and_rms, scaled_stream
from tests.test_gpu_int8 import BATCH, MEASURED, Ref, own_bounds
from tests.test_gpu_int8_exact import same_bits
from tests.test_gpu_symmetry import go_tables, move_lists

pytestmark = pytest.mark.gpu

HEADS, INT8, F16, F32 = capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32
PATH = "tower_resident_i8+heads"
WGS = 342               # workgroups the sixteen-tile level must fill (kz_tower_i8.hip, measured: Go 9x9 at batch 1024)
WIDE = 3 * WGS          # a max_batch that fills it with whole workgroups of three boards
RAGGED = WIDE - 2       # ... and the last workgroup holds one board
NARROW = 64
STAGING = 256 * 272 // 16  # floats of a wave's share of the decode's staging at sixteen tiles


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def wide_engine(model, dev, dtype=HEADS):
    eng = capi.Engine(model, dev, WIDE, dtype)
    assert eng.tower_path == (PATH if dtype == HEADS else eng.tower_path)
    per = 3 if dtype == HEADS else 2  # (the tower alone: two boards in eleven tiles, sixteen exist with the heads inside only)
    assert eng.launch_geometry(WIDE) == ((WIDE + per - 1) // per, per) and eng.launch_geometry(RAGGED) == ((RAGGED + per - 1) // per, per)
    return eng


# ---- 1. one launch ----------------------------------------------------------------------------------------------------------
def test_a_decoded_batch_of_three_board_workgroups_is_one_launch(dev):
    r = Ref.get("go9x128")
    model = r.calibrated(dev)
    idx = np.arange(WIDE) % BATCH
    rng = np.random.default_rng(2)
    moves = [rng.permutation(r.policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=WIDE)]
    eng = wide_engine(model, dev)
    eng.eval_packed_decoded(r.bits[idx], r.scalars_in[idx], moves)  # (first use)
    eng.set_profiling(True)
    before, before_tower = eng.kernel_time("")[1], eng.kernel_time("kz_tower_resident_i8")[1]
    for _ in range(3):
        eng.eval_packed_decoded(r.bits[idx], r.scalars_in[idx], moves)
    counts = (eng.kernel_time("")[1] - before, eng.kernel_time("kz_tower_resident_i8")[1] - before_tower)
    eng.set_profiling(False)
    assert counts == (3, 3), counts
    assert model.plan(WIDE, HEADS) == (PATH, 1)


# ---- 2. decode on all slots -------------------------------------------------------------------------------------------------
def test_decoded_entries_on_all_slots_with_lists_longer_than_the_staging(dev):
    b = N.build_exact("go9_3x128", None)
    eng = wide_engine(capi.Model(blob=b.blob).quantize_int8(b.site_max), dev)
    policy_len = b.ref_policy.shape[1]
    rng = np.random.default_rng(3)
    n_long = STAGING + 130
    jobs = []
    for slot in range(capi.KZ_ENGINE_SLOTS):
        n = (WIDE, RAGGED, WIDE - 1, WIDE)[slot]
        idx = (np.arange(n) + 5 * slot) % N.BOARDS
        lists = []
        for board in range(n):
            kind = (board + 1) % 3 if board < 30 + slot else 3  # (a board in the middle of its workgroup has a long list)
            if kind == 0:
                lists.append(np.arange(policy_len, dtype=np.int32))                              # all moves
            elif kind == 1:
                lists.append(np.zeros(0, np.int32))                                               # a finished board
            elif kind == 2:
                lists.append(np.resize(rng.permutation(policy_len), n_long).astype(np.int32))     # longer than the staging
            else:
                lists.append(rng.permutation(policy_len)[:int(rng.integers(1, 61))].astype(np.int32))
        assert any(len(m) > STAGING for m in lists) and any(len(m) == 0 for m in lists)
        jobs.append((slot, idx, lists, eng.submit_packed_decoded(slot, b.bits[idx], b.scalars_in[idx], lists)))
    got = [eng.wait_decoded_status(slot, offsets) for slot, _, _, offsets in jobs]
    for (slot, idx, lists, _), (values, probs, status) in zip(jobs, got):
        assert (status == 0).all(), (slot, np.flatnonzero(status))
        ref_values, ref_probs = E.decode_ref(b.ref_scalars[idx], b.ref_policy[idx], lists)
        worst = D.Worst()
        why = D.values_errors(values, ref_values, b.ref_scalars[idx][:, 4], worst)
        for board, (out, ref) in enumerate(zip(probs, ref_probs)):
            assert out.shape == ref.shape
            if len(ref):
                why += [f"board {board}: {x}" for x in D.probs_errors(out, ref, worst)]
        print(f"[int8+heads wide decode] slot {slot}: {worst}")
        assert not why, why[:5]
    slot, idx, lists, _ = jobs[1]
    values, probs, _ = got[1]
    v_one, p_one, status = eng.eval_packed_decoded_status(b.bits[idx], b.scalars_in[idx], lists)
    assert (status == 0).all() and np.array_equal(v_one, values) and all(np.array_equal(a, c) for a, c in zip(p_one, probs))
    # one index outside the policy on one board in the middle of its workgroup: that board alone, the decode's bit alone
    victim = 3 * 7 + 1
    assert victim % 3 == 1 and len(lists[victim]) > 5
    bad = [m.copy() for m in lists]
    bad[victim][5] = policy_len
    _, probs_bad, status = eng.eval_packed_decoded_status(b.bits[idx], b.scalars_in[idx], bad)
    assert status[victim] == capi.KZ_BOARD_BAD_DECODE and (np.delete(status, victim) == 0).all(), np.flatnonzero(status)
    assert all(np.array_equal(a, c) for i, (a, c) in enumerate(zip(probs_bad, probs)) if i != victim)
    # the raw entry at the same level: the reference's bits
    s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
    same_bits(b, s, p, idx, "go9_3x128, raw, three boards per workgroup")


# ---- 3. symmetries ----------------------------------------------------------------------------------------------------------
def test_sym_entry_with_mixed_ids_is_the_narrow_engine_bit_for_bit(dev):
    g = synth.game_spec("go-9")
    blob = synth.random_model("go-9", 2, 128, "conv", seed=5)
    cal_bits, cal_scalars = synth.random_boards("go-9", 32, seed=9)
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, cal_bits, cal_scalars, headroom=2.0)
    wide, narrow = wide_engine(model, dev), capi.Engine(model, dev, NARROW, HEADS)
    assert narrow.tower_path == PATH and narrow.launch_geometry(NARROW) == (NARROW, 1)
    square_src, policy_map = go_tables(g["size"])
    for eng in (wide, narrow):
        eng.set_symmetries(square_src, policy_map)
    rng = np.random.default_rng(17)
    bits, scalars = synth.random_boards("go-9", RAGGED, seed=17)
    ids = rng.integers(0, len(square_src), size=RAGGED).astype(np.uint8)
    assert len(set(ids[:9].tolist())) > 1  # (mixed within the first workgroups)
    moves = move_lists(rng, np.arange(g["policy_len"]), RAGGED, finished=4)
    v, p = wide.wait_decoded(2, wide.submit_packed_decoded(2, bits, scalars, moves, sym=ids))
    v0, _ = wide.eval_packed_decoded(bits[:NARROW], scalars[:NARROW], moves[:NARROW])
    assert not np.array_equal(v0, v[:NARROW])  # (the symmetries do something)
    for lo in (0, 3 * 110 + 1, RAGGED - NARROW):  # slices that start at the first, the second and the third board of a workgroup
        hi = lo + NARROW
        v_n, p_n = narrow.eval_packed_decoded(bits[lo:hi], scalars[lo:hi], moves[lo:hi], sym=ids[lo:hi])
        assert np.array_equal(v_n, v[lo:hi]), lo
        assert all(np.array_equal(a, c) for a, c in zip(p_n, p[lo:hi])), lo


# ---- 4. range ---------------------------------------------------------------------------------------------------------------
def test_nonfinite_boards_are_reported_per_board_and_fall_back(dev):
    n = RAGGED
    blob = scaled_stream(synth.random_model("go-9", 2, 128, "conv", seed=5, block_gain=64.0))
    bits, scalars = synth.random_boards("go-9", n, seed=3)
    policy_len = synth.game_spec("go-9")["policy_len"]
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, bits[:BATCH], scalars[:BATCH])  # (the profile is exact f32: finite maxima)
    rng = np.random.default_rng(9)
    moves = [rng.permutation(policy_len)[:int(k)].astype(np.int32) for k in rng.integers(1, 61, size=n)]
    wide, narrow = wide_engine(model, dev), capi.Engine(model, dev, NARROW, HEADS)
    _, _, status = wide.eval_packed_decoded_status(bits, scalars, moves)
    flagged = (status & capi.KZ_BOARD_NONFINITE) != 0
    assert flagged.any(), "the scaled network leaves the f16 range on no board: the test shows nothing"
    for lo in (0, 3 * 110 + 1, n - NARROW):  # exactly the boards the narrow engine (a board per workgroup) flags
        _, _, s_n = narrow.eval_packed_decoded_status(bits[lo:lo + NARROW], scalars[lo:lo + NARROW], moves[lo:lo + NARROW])
        assert np.array_equal((s_n & capi.KZ_BOARD_NONFINITE) != 0, flagged[lo:lo + NARROW]), lo
    wide.set_range_fallback(F32)
    values, probs, status = wide.eval_packed_decoded_status(bits, scalars, moves)
    assert np.array_equal((status & capi.KZ_BOARD_FELL_BACK) != 0, flagged), np.flatnonzero(((status & capi.KZ_BOARD_FELL_BACK) != 0) != flagged)
    v32, p32, _ = capi.Engine(model, dev, WIDE, F32).eval_packed_decoded_status(bits, scalars, moves)
    for board in np.flatnonzero(flagged):
        assert np.array_equal(values[board], v32[board]) and np.array_equal(probs[board], p32[board]), board


# ---- 5. parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [INT8, HEADS], ids=["dtype4", "dtype5"])
def test_parity_with_the_oracle_at_three_boards_per_workgroup(dev, dtype):
    r = Ref.get("go9x128")
    model = r.calibrated(dev)
    eng = wide_engine(model, dev, dtype)
    idx = np.arange(RAGGED) % BATCH
    s, p = eng.eval_packed(r.bits[idx], r.scalars_in[idx])
    assert np.isfinite(s).all() and np.isfinite(p).all()
    s_n, p_n = capi.Engine(model, dev, NARROW, dtype).eval_packed(r.bits, r.scalars_in)
    assert np.array_equal(s, s_n[idx]) and np.array_equal(p, p_n[idx])  # the narrow engine's bits on every copy of a board
    worst, rms = max_and_rms(s, p, r.s[idx], r.p[idx])
    own_rel, own_rms = own_bounds(MEASURED, "go9x128")
    print(f"[int8 wide] go9x128 dtype {dtype}: max {worst:.3e} (bound {own_rel:.3e}) rms {rms:.3e} (bound {own_rms:.3e})")
    assert worst <= own_rel and rms <= own_rms
