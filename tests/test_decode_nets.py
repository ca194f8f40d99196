"""The scaled family of tests/exact_nets.py and the decode cases of tests/decode_cases.py, without a GPU: the family is exact
(the conditions of the exact networks, outputs 2^k times the base network's bit for bit, l - max exact in f32), the lists
of every (network, staging size) the GPU test uses put enough entries into either error class, the oracle's f32 restatement
of decode_output — which every other decode test leans on — stays inside the bounds against the float64 reference, and
decodes with a fault leave them: what tests/test_gpu_decode_exact.py asserts can fail."""
import numpy as np
import pytest

from tests import decode_cases as D
from tests import exact_nets as E
from tests import oracle_lib as O

NETS = sorted(D.K_WIDE)
CASES = [(net, cap, variant) for net, cap in D.NET_CAPS for variant in D.VARIANTS]
IDS = [f"{net}-cap{cap}-{variant}" for net, cap, variant in CASES]


def test_every_gpu_case_has_its_exponents_and_a_list_longer_than_its_staging():
    assert {c[1] for c in D.CASES} == set(D.K_WIDE)
    assert len({c[0] for c in D.CASES}) == len(D.CASES)
    for name, net, *_rest, (cap, where), _what in D.CASES:
        n = D.lengths(E.build(net, None).ref_policy.shape[1], cap)
        assert {cap - 1, cap, cap + 1, cap + 130} <= set(n) and n[-1] > cap, name
        assert any(at >= cap for at in D.positions(cap + 130, cap)) and cap - 1 in D.positions(cap + 1, cap), name
        assert ":" in where


def test_the_staging_sizes_are_where_the_case_table_says():
    """Every `cap` cites the line it is read from: that line still sizes the staging (the arithmetic beside it in the table)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kzero_amd", "csrc")
    want = {"kz_kernels.hip": "DECODE_STAGE = 1024", "kz_tower.hip": "stage, 64 * RS / 4,", "kz_tower_pairs.hpp": "L::IMG / 4,",
            "kz_conv_heads.hpp": "cap = stage_bytes / 16"}
    for name, *_rest, (cap, where), _what in D.CASES:
        file, line = re.match(r"(\w+\.\w+):(\d+)", where).groups()
        assert want[file] in open(os.path.join(csrc, file)).read().split("\n")[int(line) - 1], f"{name}: {where}"
    src = open(os.path.join(csrc, "kz_tower.hip")).read()
    assert "constexpr int C = 256;" in src and "constexpr int RS = C * 2 + 16;" in src and D.CHESS_F16[0] == 64 * (256 * 2 + 16) // 4
    src = open(os.path.join(csrc, "kz_tower_pairs.hpp")).read()
    assert "static constexpr int RS = TWO ? C + 16 : C * 2 + 16;" in src and "static constexpr int IMG = ROWS * RS;" in src
    assert "conv_heads_tail<C, NT>(a, lds, L::LDS_BYTES, board0, boards, rows_valid, small_conv, XH, L::IMG);" in src
    src = open(os.path.join(csrc, "kz_conv_heads.hpp")).read()
    assert "constexpr int G = C / 16, RS = C * 4 + 16;" in src and "small_conv, xin, rows_img * RS);" in src


@pytest.mark.parametrize("variant", D.VARIANTS)
@pytest.mark.parametrize("net", NETS)
def test_scaled_network_is_exact_and_a_power_of_two_times_the_base(net, variant):
    b = D.scaled(net, variant)
    kp, kv, kw = b.k
    assert E.conditions_hold(b.report)
    s, p, _ = E.reference(b.tensors, b.meta, b.x)  # (asserts that both outputs are exact in f32)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s) and np.array_equal(p.astype(np.float32).astype(np.float64), p)
    assert np.array_equal(s.astype(np.float32), b.ref_scalars) and np.array_equal(p.astype(np.float32), b.ref_policy)
    base = b.base
    f = np.array([2.0 ** kv] + 3 * [2.0 ** kw] + [1.0], np.float32)
    assert np.array_equal((base.ref_scalars * f).view(np.uint32), b.ref_scalars.view(np.uint32))
    fp = np.full(base.ref_policy.shape[1], 2.0 ** (kp[0] if isinstance(kp, tuple) else kp), np.float32)
    if isinstance(kp, tuple):  # (Go: the squares, then the pass move, the last index)
        assert b.meta["policy_kind"] == "conv" and len(kp) == 2
        fp[-1] = 2.0 ** kp[1]
    assert np.array_equal((base.ref_policy * fp).view(np.uint32), b.ref_policy.view(np.uint32))
    assert np.isfinite(b.ref_policy).all() and np.isfinite(b.ref_scalars).all()
    # every difference the decode forms is exact in f32: the float64 reference starts from the same l - max
    for v in (b.ref_policy, b.ref_scalars[:, 1:4]):
        d32 = v - v.max(axis=1, keepdims=True)
        assert d32.dtype == np.float32
        assert np.array_equal(d32.astype(np.float64), v.astype(np.float64) - v.astype(np.float64).max(axis=1, keepdims=True))
    spread = b.ref_policy.max(axis=1) - b.ref_policy.min(axis=1)
    wdl = b.ref_scalars[:, 1:4].max(axis=1) - b.ref_scalars[:, 1:4].min(axis=1)
    print(f"[decode nets] {net} {variant} k={b.k}: spread {spread.min():g} to {spread.max():g}, wdl {wdl.min():g} to {wdl.max():g}, "
          f"|s0| {np.abs(b.ref_scalars[:, 0]).min():g} to {np.abs(b.ref_scalars[:, 0]).max():g}")
    if variant == "wide":
        assert spread.min() > 104 and (wdl >= 88).any()
        t = np.sort(b.ref_scalars[:, 1:4].astype(np.float64), axis=1)
        assert (t[:, 2] - t[:, 1] >= 89).any(), "no board whose largest wdl logit overflows expf when the maximum misses it"
        assert (np.abs(np.tanh(b.ref_scalars[:, 0].astype(np.float64)).astype(np.float32)) == 1.0).any(), "no board saturates tanh"
    else:
        assert spread.max() < 55 and np.abs(b.ref_scalars[:, 0]).max() < 2.0 ** -6
    assert b.ref_scalars[:, 0].any()


@pytest.mark.parametrize("net,cap,variant", CASES, ids=IDS)
def test_classes_oracle_and_mutants(net, cap, variant):
    r = D.reference(net, cap, variant)
    b, wide = r.b, variant == "wide"
    n_rel = n_under = 0
    lists = [r.lists(d) for d in range(E.BOARDS)]
    n_lists = len(lists[0])
    assert all(len(ls) == n_lists and [x.label for x in ls] == [x.label for x in lists[0]] for ls in lists)
    for d in range(E.BOARDS):
        deep = False
        for l, ml in enumerate(lists[d]):
            p = r.probs(d, l)
            assert len(p) == len(ml.moves) and abs(float(p.sum()) - 1.0) < 1e-12
            n_rel += int((p >= D.REL_MIN).sum())
            n_under += int((p < D.REL_MIN).sum())
            lg = r.logits[d][ml.moves]
            deep = deep or bool((lg - lg.max() < -104).any())
            if ml.at is not None:
                assert ml.moves[ml.at] == np.argmax(r.logits[d]) and (np.delete(lg, ml.at) < lg[ml.at]).all()
            if ml.label.startswith("far") and wide:
                assert (np.delete(lg, ml.at) <= lg[ml.at] - D.FAR).all()
            if ml.same:
                i, j = ml.same
                assert i < cap <= j and ml.moves[i] == ml.moves[j]
        assert deep or not wide, f"board {d}: no list reaches 104 below its maximum"
    share = n_rel / (n_rel + n_under)
    print(f"[decode nets] {net} cap {cap} {variant}: {n_lists} lists per board, {n_rel + n_under} entries, {share:.1%} in the relative class")
    if wide:
        assert 0.10 <= share <= 0.90
        wdl = r.values[:, 1:4]
        assert (wdl < D.REL_MIN).any() and (wdl >= D.REL_MIN).any()
    else:
        assert n_under == 0 and (r.values[:, 1:4] >= D.REL_MIN).all()
    # every schedule the GPU cases of this (network, cap) run covers every list of every board they hold
    for c in D.CASES:
        if (c[1], c[8][0]) == (net, cap):
            boards, rounds = D.schedule(c[7], n_lists)
            got = {(int(d), int(l)) for pick in rounds for d, l in zip(boards, pick) if l >= 0}
            assert got == {(int(d), l) for d in set(boards.tolist()) for l in range(n_lists)}
            assert all((pick < 0).sum() == 1 for pick in rounds)

    def decoded(fn):
        """fn(list per board) -> (values, probs), over all lists: {(board, l): probs}, values."""
        out, values = {}, None
        for l in range(n_lists):
            values, probs = fn([lists[d][l].moves for d in range(E.BOARDS)])
            out.update({(d, l): probs[d] for d in range(E.BOARDS)})
        return values, out

    def errors(values, probs, worst=None):
        why = D.values_errors(values, r.values, b.ref_scalars[:, 4], worst)
        for (d, l), p in probs.items():
            why += [f"board {d} {lists[d][l].label}: {x}" for x in D.probs_errors(p, r.probs(d, l), worst)]
        return why
    # the oracle's restatement and the plain f32 model are inside the bounds ...
    for name, fn in (("oracle", lambda m: O.decode_output(b.ref_scalars, b.ref_policy, m)),
                     ("f32 model", lambda m: D.decode_f32(b.ref_scalars, b.ref_policy, m, cap))):
        worst = D.Worst()
        why = errors(*decoded(fn), worst)
        print(f"[decode nets] {net} cap {cap} {variant} {name}: {worst}")
        assert not why, f"{name}: {len(why)} outside the bounds, first: {why[:3]}"
    # ... and every fault is outside them (wide: each on this very case)
    for fault in D.FAULTS if wide else ():
        why = errors(*decoded(lambda m: D.decode_f32(b.ref_scalars, b.ref_policy, m, cap, fault)))
        print(f"[decode nets] {net} cap {cap} {variant} fault {fault}: {len(why)} outside the bounds, first: {why[:1]}")
        assert why, f"the bounds do not see the fault {fault}"
    # the wdl maximum over two of the three: the fault that leaves out this network's largest logit overflows
    seen = [f for f in D.WDL_FAULTS if D.values_errors(D.decode_f32(b.ref_scalars, b.ref_policy, [[]] * E.BOARDS, cap, f)[0], r.values, b.ref_scalars[:, 4])]
    print(f"[decode nets] {net} cap {cap} {variant} wdl faults seen: {seen}")
    assert seen or not wide
    if wide:
        top = int(np.argmax(b.ref_scalars[0, 1:4]))
        assert D.WDL_FAULTS[top] in seen


def test_the_networks_together_see_every_choice_of_two_wdl_logits():
    """Which of s1..s3 is the largest is a property of the network; over the cases' networks each of the three is, by 89 or more."""
    tops = set()
    for net in NETS:
        t = D.scaled(net, "wide").ref_scalars[:, 1:4].astype(np.float64)
        order = np.argsort(t, axis=1)
        gap = np.take_along_axis(t, order[:, 2:], 1) - np.take_along_axis(t, order[:, 1:2], 1)
        tops |= set(order[:, 2][gap[:, 0] >= 89].tolist())
    assert tops == {0, 1, 2}
