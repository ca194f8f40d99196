"""The exactly representable networks of tests/exact_nets.py, without a GPU: the conditions that make zero tolerance
follow hold for every committed (network, dense position) with no seed redraw, the oracle returns the bits of the
independent float64 reference, and a single flipped weight — an error the f16 bounds of tests/test_gpu_parity.py cannot
see — changes the reference's output."""
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
