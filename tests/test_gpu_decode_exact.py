"""The decode of every shipping launch — tanh, the wdl softmax, the gather and softmax over the listed moves
(kz_decode_dev.hpp: decode_board_wave) — held to a float64 softmax of logits that are known exactly, in every instantiation
and every way boards map to waves.  The networks are the scaled family of tests/exact_nets.py (`build_scaled`): each case
first returns the reference's raw scalars and logits to the bit (without that nothing below means anything), then decodes the
lists of tests/decode_cases.py through eval_packed_decoded_status and must stay inside the derived bounds stated there,
with status 0 on every board.  Wide variant: the logits span more than 104, every list holds the maximum at a chosen
position among entries at least 100 below it — a maximum the wave's reductions miss overflows expf —, lengths around 64,
the wave's staging `cap` and beyond it (the re-read tail; cap per instance in decode_cases.CASES).  Moderate variant: every
probability a normal f32 inside the relative bound, s0 of a few thousandths for tanh's ulp bound.

tests/test_decode_nets.py holds, without a GPU, that the references meet the conditions that make this a test (class shares,
the oracle inside the bounds, decodes with a fault outside them).

Largest errors observed on an MI355X, per decode site, over both variants (bounds: probabilities (m + 18) u ref with
m = ceil(n / 64), wdl 19 u ref, tanh 5 ulp):
  kz_tower.hip (chess f16, one and two boards per workgroup; cap 8448)   probs 24.9 u ref, 23 % of a list's bound; wdl 0.60 u ref; tanh 0.33 ulp
  kz_tower_pairs.hpp, chess split16 (wave 0; cap 8448)                   probs 24.9 u ref, 23 %; wdl 0.60 u ref; tanh 0.33 ulp
  kz_decode_output (f32 and f16g chess, generic dense, Go 19x19; 1024)   probs 6.5 u ref, 28 %; wdl 1.50 u ref; tanh 0.48 ulp
  conv_heads_tail (Ataxx 7x7 and 5x5, Go 9x9; f16, split16, f32; caps 864 to 3696)   probs 19.7 u ref, 31 %; wdl 2.11 u ref; tanh 0.34 ulp
  underflow class: largest output 7.3e-31 (2^-99 = 1.6e-30); every saturated tanh exactly +-1.
The probability maxima are on the longest lists (m = 135 at 8578 moves); relative to a list's own bound no case uses a third.
"""
import numpy as np
import pytest

from kzero_amd import capi
from tests import decode_cases as D
from tests.test_gpu_exact import make_engine, mismatch
from tests.test_gpu_symmetry import go_tables, map_bits, map_moves, synthetic_tables

pytestmark = pytest.mark.gpu

CASES = [(c, v) for c in D.CASES for v in D.VARIANTS]
IDS = [f"{c[0]}-{v}" for c, v in CASES]
SYM_CASES = [c for c in D.CASES if c[0] in ("chess256-f16-nb2", "go9x128-f16g-2")]  # the chess launch, one conv-head launch


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine_of(dev, case, b):
    name, net, dtype, max_batch, switches, path, per, batch, (cap, _), what = case
    eng = make_engine(capi.Model(blob=b.blob), dev, max_batch, dtype, switches)
    assert eng.tower_path == path
    geometry = eng.launch_geometry(batch)
    if per is not None:
        assert geometry == ((batch + per - 1) // per, per)
        assert batch % per == 1 or per == 1, "ragged: the last workgroup holds one board"
    else:
        assert batch % 4 == 1, "ragged: kz_decode_output's last workgroup holds one board"
    return eng, geometry


def batch_lists(r, boards, pick):
    return [r.lists(int(d))[l].moves if l >= 0 else np.zeros(0, np.int32) for d, l in zip(boards, pick)]


@pytest.mark.parametrize("case,variant", CASES, ids=IDS)
def test_decode_meets_the_float64_reference(dev, case, variant):
    name, net, dtype, max_batch, switches, path, per, batch, (cap, where), what = case
    r = D.reference(net, cap, variant)
    b = r.b
    eng, geometry = engine_of(dev, case, b)
    n_lists = len(r.lists(3))
    boards, rounds = D.schedule(batch, n_lists)
    bits, scalars_in = b.bits[boards], b.scalars_in[boards]
    # the raw outputs are the reference's bits: what is decoded below is known exactly
    s, p = eng.eval_packed(bits, scalars_in)
    assert np.array_equal(s, b.ref_scalars[boards]), "scalars: " + mismatch(s, b.ref_scalars[boards], 5)
    assert np.array_equal(p, b.ref_policy[boards]), "policy: " + mismatch(p, b.ref_policy[boards], b.meta["board_h"] * b.meta["board_w"])
    worst, why, longest = D.Worst(), [], 0
    for rnd, pick in enumerate(rounds):
        moves = batch_lists(r, boards, pick)
        values, probs, status = eng.eval_packed_decoded_status(bits, scalars_in, moves)
        assert not status.any(), f"round {rnd}: status {status[status != 0][:8]} on boards {np.flatnonzero(status)[:8]}"
        why += [f"round {rnd}: {x}" for x in D.values_errors(values, r.values[boards], b.ref_scalars[boards, 4], worst)]
        for i, (d, l) in enumerate(zip(boards, pick)):
            if l < 0:
                assert probs[i].size == 0
                continue
            ml = r.lists(int(d))[l]
            assert probs[i].shape == ml.moves.shape
            longest = max(longest, len(ml.moves))
            why += [f"round {rnd} slot {i} board {d} {ml.label}: {x}" for x in D.probs_errors(probs[i], r.probs(int(d), l), worst)]
            # the same index gives the same bits wherever it stands: staged value or re-read tail
            _, first, inverse = np.unique(ml.moves, return_index=True, return_inverse=True)
            if not np.array_equal(bits_of(probs[i]), bits_of(probs[i])[first][inverse]):
                why.append(f"round {rnd} slot {i} board {d} {ml.label}: one index, two probabilities")
            if ml.same:
                assert ml.same[0] < cap <= ml.same[1] and bits_of(probs[i])[ml.same[0]] == bits_of(probs[i])[ml.same[1]]
    print(f"[decode exact] {name} {variant} k={b.k}: {path}, {batch} boards in {geometry[0]} workgroups of {geometry[1]}; {what}, cap {cap} "
          f"({where}); {len(rounds)} rounds of {n_lists} lists, longest {longest}: {worst}")
    assert longest > cap, "no list reaches the re-read tail"
    assert not why, f"{len(why)} outside the bounds, first: {why[:4]}"


@pytest.mark.parametrize("case", SYM_CASES, ids=[c[0] for c in SYM_CASES])
def test_the_lists_again_with_symmetry_ids(dev, case):
    """The `_sym` entry on the original boards and lists against the host route (planes permuted and re-packed, move indices
    mapped, tests/test_gpu_symmetry.py) through the plain entry: the same bits in values, probabilities and status, the lists
    longer than the staging included.  (A mapped board is another position: its logits are not the reference's, a list may
    overflow on it — in both routes alike.)"""
    name, net, dtype, max_batch, switches, path, per, batch, (cap, _), what = case
    r = D.reference(net, cap, "wide")
    b = r.b
    eng, _ = engine_of(dev, case, b)
    hw, policy_len = b.meta["board_h"] * b.meta["board_w"], b.ref_policy.shape[1]
    square_src, policy_map = go_tables(b.meta["board_h"]) if net.startswith("go") else synthetic_tables(hw, policy_len, 3, seed=77)
    assert policy_map.shape[1] == policy_len and (policy_map >= 0).all()
    eng.set_symmetries(square_src, policy_map)
    n_sym, n_bool = len(square_src), b.meta["input_bool_channels"]
    boards, rounds = D.schedule(batch, len(r.lists(3)))
    bits, scalars_in = b.bits[boards], b.scalars_in[boards]
    longest = differs = 0
    for rnd, pick in enumerate(rounds):
        moves = batch_lists(r, boards, pick)
        ids = ((np.arange(batch) + rnd) % n_sym).astype(np.uint8)
        v_ref, p_ref, st_ref = eng.eval_packed_decoded_status(map_bits(bits, n_bool, hw, square_src, ids), scalars_in, map_moves(moves, policy_map, ids))
        v, p, st = eng.eval_packed_decoded_status(bits, scalars_in, moves, sym=ids)
        assert np.array_equal(bits_of(v), bits_of(v_ref)) and np.array_equal(st, st_ref), f"round {rnd}"
        for i, (a, ref) in enumerate(zip(p, p_ref)):
            assert a.shape == moves[i].shape and np.array_equal(bits_of(a), bits_of(ref)), f"round {rnd} slot {i}"
        longest = max(longest, max(len(m) for m in moves))
        v0, _, _ = eng.eval_packed_decoded_status(bits, scalars_in, moves) if rnd == 0 else (v, None, None)
        differs += int(not np.array_equal(v0, v))
    assert longest > cap and differs, "the symmetries do something, on lists that reach the re-read tail"
