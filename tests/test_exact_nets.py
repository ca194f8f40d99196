"""The exactly representable networks of tests/exact_nets.py, without a GPU: the conditions that make zero tolerance
follow hold for every committed (network, dense position) with no seed redraw, the oracle returns the bits of the
independent float64 reference, and a single flipped weight — an error the f16 bounds of tests/test_gpu_parity.py cannot
see — changes the reference's output.  The wide family (lo halves that are not zero) likewise: its three conditions, its
coverage of every layer's input and weight fragments, the oracle's bits, and the gap it closes — a missing lo fragment,
which the 1e-4 of the split16 paths cannot see, changes its outputs on every board."""
import os

import numpy as np
import pytest

from kzero_amd import synth
from kzero_amd.model_file import read_model, write_model
from tests import exact_nets as E
from tests import oracle_lib as O

F16_REL, F16_RMS = 3.5e-3, 6e-4  # tests/test_gpu_parity.py's assert_f16 (a GPU module: restated, test_bounds_restated holds them equal)

CASES = [(net, pos) for net in E.NETS for pos in E.positions(net)]
IDS = [f"{net}-{'none' if pos is None else pos}" for net, pos in CASES]


def test_bounds_restated():
    from tests import test_gpu_parity as P
    assert (F16_REL, F16_RMS) == (P.F16_REL, P.F16_RMS)
    assert F32_ATOL == P.F32_ATOL


def test_step_of():
    assert E.step_of([3.0, 6.0, -12.0]) == 1.0 and E.step_of([0.75, 0.0, 2.5]) == 0.25 and E.step_of([0.0]) == 1.0
    assert E.step_of([48.0, -16.0]) == 16.0


@pytest.mark.parametrize("net,pos", CASES, ids=IDS)
def test_conditions_and_oracle(net, pos):
    b = E.build(net, pos)
    stored, sums = b.report.worst()
    print(f"[exact] {net} dense_at={pos} ({b.layers[pos] if pos is not None else '-'}): max |v| / step = {stored:.0f}, "
          f"max sum |a b| / step = {sums:.0f}")
    assert b.seed == E.SEED, "the committed list needs no redraw"
    for name, (v, roundtrips) in b.report.stored.items():
        assert roundtrips and v <= E.STORED_MAX, f"{name}: {v} steps, f16 round trip {roundtrips}"
    for name, v in b.report.sums.items():
        assert v <= E.SUM_MAX, f"{name}: sum |a b| / step = {v}"
    # the generator's promises
    for i, p in enumerate(b.layers):
        w, bias = b.tensors[p + ".weight"], b.tensors[p + ".bias"]
        assert bias.any(), f"{p}: an all-zero bias hides a bias indexing error"
        if i == pos and pos not in E.NETS[net][5]:
            assert np.count_nonzero(w) == w.size, f"{p}: the dense layer has a zero weight"
    if b.meta["policy_kind"] == "attention":
        assert np.array_equal(b.tensors["policy_head.FLAT_TO_ATT"], synth.chess_flat_to_att())
    # the oracle returns the same bits (five boards: the oracle is the slow side)
    n = 5
    oracle = O.OracleNet(b.blob)
    x32 = b.x[:n].astype(np.float32)
    assert np.array_equal(x32, O.encode_input_full(b.bits[:n], b.scalars_in[:n], oracle.n_scalar, oracle.n_bool, oracle.h, oracle.w))
    s, p = oracle.forward(x32, threads=4)
    assert np.array_equal(s, b.ref_scalars[:n]), "scalars"
    assert np.array_equal(p, b.ref_policy[:n]), "policy"


@pytest.mark.parametrize("net", ["chess_2x256_att", "go9_1x128", "arimaa_1x96"])
def test_oracle_trace_equals_reference(net):
    """forward_trace's tower and scalar-head tensors, with the dense layer in the tower's last convolution."""
    b = E.build(net, 2 * b_depth(net))
    oracle = O.OracleNet(b.blob)
    _, _, acts = oracle.forward_trace(b.x[:2].astype(np.float32))
    ref = b.report.acts
    names = [k for k in acts if k.startswith("tower.") or k.startswith("scalar_head.")]
    assert len(names) == 2 + 2 * b_depth(net) + 2
    for k in names:
        assert np.array_equal(acts[k], ref[k][:2].reshape(2, -1).astype(np.float32)), k


def b_depth(net):
    return E.NETS[net][1]


def _flips(shape, n=16):
    """Twenty single weights of an OIHW convolution: corner and edge taps, the last input channel, the last output channel,
    and sixteen drawn ones.  Fixed before any was tried."""
    co, ci = shape[0], shape[1]
    fixed = [(0, ci - 1, 0, 0), (co - 1, ci - 1, 2, 2), (17, 0, 0, 2), (co // 2, ci - 1, 1, 1)]
    rng = np.random.default_rng(2024)
    return fixed + [(int(rng.integers(co)), int(rng.integers(ci)), int(rng.integers(3)), int(rng.integers(3))) for _ in range(n)]


def test_one_flipped_weight_shows_in_the_reference_and_not_in_the_f16_bounds():
    """The gap this file closes.  One weight's sign in a 256-channel 3x3 convolution changes the exact network's outputs
    (so an engine that reads one wrong weight, or one wrong input channel on one tap, fails array_equal), while the
    same flip in a random-weight chess 2x256 moves the oracle's outputs by a small fraction of the f16 bounds."""
    b = E.build("chess_2x256_att", 2)
    layer = b.layers[2]
    n = 3  # (boards of the random network; the exact network keeps all of its own: a channel may live on one of them only)
    x = b.x
    s0, p0, _ = E.reference(b.tensors, b.meta, x)
    rmeta, rt = read_model(synth.random_model("chess", 2, 256, "attention", seed=3))
    rbits, rscalars = synth.random_boards("chess", n, seed=4)
    net0 = O.OracleNet(write_model(rmeta, rt))
    xr = O.encode_input_full(rbits, rscalars, net0.n_scalar, net0.n_bool, net0.h, net0.w)
    rs0, rp0 = net0.forward(xr, threads=4)
    inside = 0
    flips = _flips(b.tensors[layer + ".weight"].shape)
    for f in flips:
        t = dict(b.tensors)
        w = t[layer + ".weight"].copy()
        w[f] = -w[f]
        t[layer + ".weight"] = w
        s1, p1, _ = E.reference(t, b.meta, x)
        changed = int(np.count_nonzero(s1 != s0) + np.count_nonzero(p1 != p0))
        assert changed > 0, f"flip {f}: the exact network does not see it"
        rt1 = dict(rt)
        w = rt1[layer + ".weight"].copy()
        w[f] = -w[f]
        rt1[layer + ".weight"] = w
        rs1, rp1 = O.OracleNet(write_model(rmeta, rt1)).forward(xr, threads=4)
        worst = 0.0
        ok = True
        for a, ref in ((rs1, rs0), (rp1, rp0)):
            scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
            rel = float((np.abs(a - ref) / scale).max())
            rms = float(np.sqrt(np.mean(((a - ref) / scale) ** 2)))
            worst = max(worst, rel / F16_REL, rms / F16_RMS)
            ok = ok and rel <= F16_REL and rms <= F16_RMS
        inside += ok
        print(f"[flip] {layer}{list(f)}: exact network: {changed} outputs differ; random network: {worst:.3f} of the f16 bounds")
    print(f"[flip] {inside} of {len(flips)} flips stay inside the f16 bounds on the random network")
    assert inside == len(flips)


# ---- the wide family: lo halves that are not zero ----

WIDE_CASES = [(net, wide) for net in E.WIDE_NETS for wide in E.wide_positions(net)]
WIDE_IDS = [f"{net}-{E.wide_id(wide)}" for net, wide in WIDE_CASES]
F32_ATOL = 1e-4  # tests/test_gpu_parity.py's bound on the exact-f32 and split16 paths (test_bounds_restated)


@pytest.mark.parametrize("net,wide", WIDE_CASES, ids=WIDE_IDS)
def test_wide_conditions_and_oracle(net, wide):
    """split-stored, no lo.lo and sums on every committed wide network, and the oracle (f32: exact by the sums) returns
    the reference's bits."""
    b = E.build(net, None, wide)
    rep = b.report
    print(f"[wide] {net} {E.wide_id(wide)}: max sum |a b| / step = {max(rep.sums.values()):.0f}, "
          f"{sum(1 for k in rep.split if not k.endswith('.weight'))} stored tensors, {len(rep.lolo)} products")
    assert b.seed == E.SEED, "the committed list needs no redraw"
    assert set(rep.split) == set(rep.stored) | {p + ".weight" for p in b.layers}
    for name, (exact, normal) in rep.split.items():
        assert exact, f"{name}: v != hi + lo for an f16 neighbour as hi, or |v| > {E.SPLIT_MAX}"
        assert normal, f"{name}: a lo half below 2^-14"
    assert set(rep.lolo) == set(b.layers) | ({"policy_head.bmm"} if b.meta["policy_kind"] == "attention" else set())
    for name, (one_narrow, three_terms) in rep.lolo.items():
        assert one_narrow, f"{name}: both operands carry lo halves"
        assert three_terms, f"{name}: hi*hi + hi*lo + lo*hi is not the product"
    for name, v in rep.sums.items():
        assert v <= E.SUM_MAX, f"{name}: sum |a b| / step = {v}"
    # it is wide where it says
    at = wide[0]
    if at == "input":
        assert rep.lo_in["common.tower.0"][0] >= E.LIVE_SHARE and not any(m.any() for m in rep.lo_w.values())
    else:
        assert rep.lo_w[b.layers[at]].any() and not any(m.any() for p, m in rep.lo_w.items() if p != b.layers[at])
        assert not any(share for p, (share, _) in rep.lo_in.items() if b.layers.index(p) <= at), "everything in front of the wide layer is narrow"
    for p in b.layers:
        assert b.tensors[p + ".bias"].any(), f"{p}: an all-zero bias hides a bias indexing error"
    n = 5
    oracle = O.OracleNet(b.blob)
    x32 = b.x[:n].astype(np.float32)
    assert np.array_equal(x32, O.encode_input_full(b.bits[:n], b.scalars_in[:n], oracle.n_scalar, oracle.n_bool, oracle.h, oracle.w))
    s, p = oracle.forward(x32, threads=4)
    assert np.array_equal(s, b.ref_scalars[:n]), "scalars"
    assert np.array_equal(p, b.ref_policy[:n]), "policy"


@pytest.mark.parametrize("net", E.WIDE_NETS)
def test_wide_coverage(net):
    """Every layer position meets lo halves from both sides in some wide variant of its network: a variant whose input to
    the layer has a lo half in every 32-channel chunk and on LIVE_SHARE of its (board, square, channel) entries, and a
    variant in which every weight fragment (16 output rows, tap, 32 input channels) of the layer holds one.  conv_bulk
    makes up both operands of q_from . q_to, of which one stays narrow: its fragments are covered by two variants together."""
    cover = E.coverage(net)
    layers = E.build(net, None, E.wide_positions(net)[0]).layers
    for p in layers:
        shares = {E.wide_id(w): lo_in[p][0] for w, (lo_in, _) in cover.items() if lo_in[p][1]}
        best = max(shares, key=shares.get) if shares else None
        print(f"[wide] {net} {p}: input lo on {shares.get(best, 0.0):.3f} of the entries ({best})")
        assert shares and shares[best] >= E.LIVE_SHARE, f"{p}: no variant feeds it lo halves in every chunk and on {E.LIVE_SHARE} of the entries"
        maps = [lo_w[p] for _, lo_w in cover.values()]
        if p == "policy_head.conv_bulk":
            assert np.logical_or.reduce(maps).all() and max(m.mean() for m in maps) == 0.5
        else:
            assert any(m.all() for m in maps), f"{p}: no variant has a lo half in every weight fragment"


def test_split_exact():
    """The measuring stick itself: either neighbour as hi, the subnormal rule, the range."""
    ok = [E.WIDE, -0.25 * E.WIDE, 1.5 * E.WIDE, 1023.0 + 2.0 ** -12, 3.0, 0.0, E.SPLIT_MAX]
    assert E.split_exact(np.array(ok)) == (True, True) and E.split_exact(np.array([3.0, 0.5])) == (True, False)
    assert not E.split_exact(np.array([1.0 + 2.0 ** -23]))[0], "lo needs more than f16 holds"
    assert not E.split_exact(np.array([1.0 + 2.0 ** -15]))[0], "a subnormal lo"
    assert not E.split_exact(np.array([E.SPLIT_MAX + 16.0]))[0], "beyond half of f16's range"
    below, above = E.f16_neighbours(np.array([E.WIDE, 2.0]))
    assert below.tolist() == [1.0, 2.0] and above.tolist() == [1.0 + 2.0 ** -10, 2.0]


# (network, wide variant, spoiled layer, its fragments): the stem wide, so the first block's convolution reads lo halves; its own weights wide
GAP_NET = "chess_2x256_att"
GAP_ACT = ((0, "from"), "common.tower.1.seq.0", [(0, 0), (1, 2), (2, 1)])
GAP_WEIGHT = ((1, "from"), "common.tower.1.seq.0", [(0, (0, 0), 0), (5, (1, 1), 3), (15, (2, 2), 7), (9, (0, 2), 4)])


def _random_twin():
    rmeta, rt = read_model(synth.random_model("chess", 2, 256, "attention", seed=3))
    rbits, rscalars = synth.random_boards("chess", E.BOARDS, seed=4)
    return rmeta, rt, E.encode(rmeta, rbits, rscalars)


def _gap(wide, layer, spoils):
    """(outputs changed per board on the wide exact network, max |delta| / 1e-4 on the random-weight network) per spoil."""
    b = E.build(GAP_NET, None, wide)
    s0, p0, _ = E.reference(b.tensors, b.meta, b.x)
    assert np.array_equal(s0.astype(np.float32), b.ref_scalars) and np.array_equal(p0.astype(np.float32), b.ref_policy)
    rmeta, rt, xr = _random_twin()
    rs0, rp0, _ = E.reference(rt, rmeta, xr, exact=False)
    out = []
    for spoil in spoils:
        s1, p1, _ = E.reference(b.tensors, b.meta, b.x, spoil=dict(layer=layer, **spoil), exact=False)
        changed = (s1 != s0).sum(axis=1) + (p1 != p0).sum(axis=1)
        rs1, rp1, _ = E.reference(rt, rmeta, xr, spoil=dict(layer=layer, **spoil), exact=False)
        out.append((changed, max(np.abs(rs1 - rs0).max(), np.abs(rp1 - rp0).max()) / F32_ATOL))
    return out


def test_a_wrong_lo_address_shows_on_a_wide_network_and_not_in_the_1e_4_bound():
    """The gap the wide family closes.  What a wrong lo address does — the lo halves of one layer's input missing on one
    tap at the edge squares, or the lo halves of one weight fragment missing — changes a wide exact network's outputs on
    every board (so a split16 engine that reads one wrong lo fragment fails array_equal), while the same fault in a
    random-weight chess 2x256, evaluated by the same float64 reference, stays under the 1e-4 that holds the split16 paths."""
    wide, layer, taps = GAP_ACT
    for tap, (changed, share) in zip(taps, _gap(wide, layer, [dict(tap=t) for t in taps])):
        print(f"[gap] {layer} input lo missing on tap {tap} at the edge squares: wide network: {changed.sum()} outputs differ "
              f"({changed.min()} on the least affected board); random network: {share:.4f} of the 1e-4 bound")
        assert changed.all(), f"tap {tap}: a board's outputs do not see it"
        assert share < 1.0
    wide, layer, frags = GAP_WEIGHT
    for frag, (changed, share) in zip(frags, _gap(wide, layer, [dict(fragment=f) for f in frags])):
        print(f"[gap] {layer} weight fragment {frag} without lo: wide network: {changed.sum()} outputs differ "
              f"({changed.min()} on the least affected board); random network: {share:.4f} of the 1e-4 bound")
        assert changed.all(), f"fragment {frag}: a board's outputs do not see it"
        assert share < 1.0


def test_the_narrow_family_is_blind_to_a_wrong_lo_address():
    """The same two faults on a network of the narrow family: nothing changes, every lo half being zero."""
    b = E.build(GAP_NET, 2)
    s0, p0, _ = E.reference(b.tensors, b.meta, b.x)
    for spoil in (dict(tap=GAP_ACT[2][0]), dict(fragment=GAP_WEIGHT[2][0])):
        s1, p1, _ = E.reference(b.tensors, b.meta, b.x, spoil=dict(layer=GAP_ACT[1], **spoil), exact=False)
        assert np.array_equal(s1, s0) and np.array_equal(p1, p0)


def test_gpu_cases_name_the_paths_the_selector_plans():
    """tests/test_gpu_exact.py's engine list against kz_model_plan (host logic, no GPU; tests/test_path_table.py holds it to
    tests/golden/path_table.json): every case runs the kernel it is listed for."""
    from kzero_amd import capi
    from tests import test_gpu_exact as G
    assert {e[1] for e in G.ENGINES} == set(E.NETS), "a network without an engine, or an engine without its network"
    models = {}
    for name, net, dtype, max_batch, switches, path, _, batch in G.ENGINES:
        if net not in models:
            models[net] = capi.Model(blob=E.build(net, None).blob)
        saved = {k: os.environ.get(k) for k in switches}
        os.environ.update(switches)
        try:
            planned = models[net].plan(max_batch, dtype)[0]
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        assert planned == path, name
        assert batch <= max_batch
