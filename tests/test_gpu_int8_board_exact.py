"""KZ_DTYPE_INT8_ANY on the GPU, to the bit (tests/int8_board_nets.py): the per-layer int8 kernel ("board_conv_i8") must return
the bits of the float64 reference that quantises where the contract quantises.  Integer sums are exact and every scale is a
power of two, so there is no tolerance: a difference is an indexing, packing, lane-map, rounding or clamping error.

Every network of the table in the exact family (the first three also with the first conv A and the last conv B dense) and in
the rounding family, and one network per chunk count with weights that round.  Board counts 1, bpw + 1 and 2 bpw + 1 (bpw: boards
per workgroup of the board-tile geometry): odd group counts under the grid's rounding to eight groups, so idle workgroups occur
and the last workgroup is ragged.  Through the packed entry, through kz_engine_eval_dense, and through submit_packed_decoded on
all four slots (the decode held to tests/decode_cases.py's bounds on the reference's logits, and to the synchronous entry's
bits).  And on a shape both plans run, dtype 8 is dtype 5's plan and returns its bits."""
import numpy as np
import pytest

from kzero_amd import capi
from tests import decode_cases as D
from tests import exact_nets as E
from tests import int8_board_nets as B
from tests import int8_nets as N
from tests.test_gpu_exact import mismatch

pytestmark = pytest.mark.gpu

ANY = capi.KZ_DTYPE_INT8_ANY
MAX_BATCH = 64
CASES = ([(net, "exact", d) for net in B.NETS for d in B.dense_positions(net)] + [(net, "round", None) for net in B.NETS] +
         [(net, "weights", None) for net in B.WEIGHT_NETS])
IDS = [f"{net}-{fam}-{d}" for net, fam, d in CASES]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def same_bits(b, s, p, idx, what):
    hw = b.meta["board_h"] * b.meta["board_w"]
    assert np.array_equal(s, b.ref_scalars[idx]), f"{what}, scalars: " + mismatch(s, b.ref_scalars[idx], 5)
    assert np.array_equal(p, b.ref_policy[idx]), f"{what}, policy: " + mismatch(p, b.ref_policy[idx], hw)


@pytest.mark.parametrize("net,family,dense_at", CASES, ids=IDS)
def test_board_conv_i8_returns_the_reference_bits(dev, net, family, dense_at):
    b = B.build_exact(net, dense_at) if family == "exact" else B.build_round(net, dense_at, "round" if family == "weights" else None)
    depth, channels = b.meta["tower_depth"], b.meta["tower_channels"]
    h, w = b.meta["board_h"], b.meta["board_w"]
    assert all(b.report.exact.values()) and N.head_conditions(b.heads, depth)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    assert list(model.int8_site_exponents()) == b.exps[:2 * depth]
    eng = capi.Engine(model, dev, MAX_BATCH, ANY)
    assert eng.tower_path == "board_conv_i8"
    bpw = B.geometry(h, w)[1]
    assert eng.launch_geometry(B.BOARDS) == (B.workgroups(B.BOARDS, h, w, channels), 0)
    assert 2 * bpw + 1 <= MAX_BATCH
    counts = list(dict.fromkeys((1, bpw + 1, 2 * bpw + 1)))
    for n in counts:
        idx = np.arange(n) % B.BOARDS
        what = f"{net} {family} {dense_at}, {n} boards"
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        same_bits(b, s, p, idx, what)
        s, p = eng.eval_dense(b.x[idx])
        same_bits(b, s, p, idx, what + ", eval_dense")
    # the decoded entry, four slots in flight
    policy_len = b.ref_policy.shape[1]
    rng = np.random.default_rng(7)
    jobs = []
    for slot in range(4):
        n = counts[slot % len(counts)]
        idx = (np.arange(n) + slot) % B.BOARDS
        moves = [rng.permutation(policy_len)[:int(k)].astype(np.int32) for k in rng.integers(0, min(policy_len, 60) + 1, size=n)]
        jobs.append((slot, idx, moves, eng.submit_packed_decoded(slot, b.bits[idx], b.scalars_in[idx], moves)))
    got = [eng.wait_decoded(slot, off) for slot, _, _, off in jobs]
    for (slot, idx, moves, _), (values, probs) in zip(jobs, got):
        ref_values, ref_probs = E.decode_ref(b.ref_scalars[idx], b.ref_policy[idx], moves)
        why = D.values_errors(values, ref_values, b.ref_scalars[idx][:, 4])
        for board, (out, ref) in enumerate(zip(probs, ref_probs)):
            assert out.shape == ref.shape
            if len(ref):
                why += [f"board {board}: {x}" for x in D.probs_errors(out, ref)]
        assert not why, (slot, why)
        v_one, p_one = eng.eval_packed_decoded(b.bits[idx], b.scalars_in[idx], moves)
        assert np.array_equal(v_one, values) and all(np.array_equal(a, c) for a, c in zip(p_one, probs)), slot


@pytest.mark.parametrize("family", ["exact", "round"])
def test_dtype_8_is_dtype_5_where_the_one_launch_tower_runs(dev, family):
    b = N.build_exact(B.BOTH_PLANS) if family == "exact" else N.build_round(B.BOTH_PLANS, None)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    e8, e5 = capi.Engine(model, dev, MAX_BATCH, ANY), capi.Engine(model, dev, MAX_BATCH, capi.KZ_DTYPE_INT8_HEADS)
    assert e8.tower_path == e5.tower_path and e8.tower_path.startswith("tower_resident_i8")
    assert e8.launch_geometry(N.BOARDS) == e5.launch_geometry(N.BOARDS)
    s8, p8 = e8.eval_packed(b.bits, b.scalars_in)
    s5, p5 = e5.eval_packed(b.bits, b.scalars_in)
    assert np.array_equal(s8, s5) and np.array_equal(p8, p5)
