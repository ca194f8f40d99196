"""The networks of tests/board_nets.py hold what they promise, on the CPU: the conditions of tests/exact_nets.py that make zero
tolerance follow, narrow and wide, with no redraw the table does not record; the wide family's coverage of every tower layer;
the geometry, workgroup counts and planned paths each network is there for; the oracle's bits; and the three mutant references
— faults of a kernel that stages 64 input channels at a time, writes 64 output channels per workgroup and rotates three
activation buffers — change the outputs of every case of the networks named for them, and cannot even be written down on the
three networks the board engines of tests/test_gpu_exact.py run.  tests/test_gpu_board_exact.py holds the f16 and split16
board-tile engines to the same references' bits."""
import os

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import board_nets as B
from tests import exact_nets as E
from tests import oracle_lib as O

CASES = [(net, d, None) for net in B.NETS for d in B.dense_positions(net)] + [(net, None, w) for net in B.NETS for w in B.wide_positions(net)]
CASES.sort(key=lambda c: list(B.NETS).index(c[0]))
IDS = [f"{net}-{E.wide_id(w) if w else 'none' if d is None else d}" for net, d, w in CASES]

# network -> ((tiles per board, boards per workgroup, skew16), boards of the three launches, their workgroups)
GEOMETRY = {
    "go19_1x256": ((23, 1, 11), [9, 2, 1], [36, 8, 4]),
    "go19_1x192": ((23, 1, 11), [9, 2, 1], [27, 6, 3]),
    "go13_2x128": ((11, 2, 11), [17, 3, 1], [18, 4, 2]),
    "go9_1x256": ((6, 4, 0), [33, 5, 1], [36, 8, 4]),
    "ataxx7_1x384": ((4, 6, 0), [49, 7, 1], [54, 12, 6]),
    "chess_1x320_att": ((4, 5, 0), [41, 6, 1], [45, 10, 5]),
    "ataxx5_1x128": ((2, 11, 0), [89, 12, 1], [18, 4, 2]),
    "ataxx6_1x128": ((3, 8, 0), [65, 9, 1], [18, 4, 2]),
    "ataxx4_1x128": ((1, 16, 0), [129, 17, 1], [18, 4, 2]),
    "ataxx5_1x320": ((2, 11, 0), [89, 12, 1], [45, 10, 5]),
    "ataxx6_1x320": ((3, 8, 0), [65, 9, 1], [45, 10, 5]),
    "ataxx4_1x320": ((1, 16, 0), [129, 17, 1], [45, 10, 5]),
    "go13_1x128": ((11, 2, 11), [17, 3, 1], [18, 4, 2]),
}
MT = 24  # tiles of a workgroup


def test_geometry_is_what_the_table_says():
    assert set(GEOMETRY) == set(B.NETS)
    for net, (geo, boards, wgs) in GEOMETRY.items():
        assert B.geometry(net) == geo, net
        assert B.launches(net) == boards and [B.workgroups(net, n) for n in boards] == wgs, net
    tiles = {net: geo[0] * geo[1] for net, (geo, _, _) in GEOMETRY.items()}
    # the padding-tile skip needs exactly one idle tile: 19x19 only; 13x13's two, 8x8's four and 5x5's two are computed
    assert {net for net, n in tiles.items() if n == MT - 1} == {"go19_1x256", "go19_1x192"}
    assert tiles["go13_2x128"] == 22 and tiles["chess_1x320_att"] == 20 and tiles["ataxx5_1x128"] == 22 and tiles["go9_1x256"] == MT
    # boards per workgroup set by the LDS, not by the 24 tiles
    by_lds = ("chess_1x320_att", "ataxx5_1x128", "ataxx4_1x128", "ataxx5_1x320", "ataxx4_1x320")  # five of six, 11 of 12, 16 of 24
    assert all((GEOMETRY[net][0][1] < MT // GEOMETRY[net][0][0]) == (net in by_lds) for net in B.NETS)
    # boards straddle tiles where the squares are no multiple of 16
    assert [B.size(net) ** 2 % 16 == 0 for net in ("chess_1x320_att", "ataxx4_1x128", "go9_1x256")] == [True, True, False]
    # chunks of 64 input channels: one with a chunk that is neither first nor last needs three; quarters past the second likewise
    assert sorted({B.NETS[net][2] // 64 for net in B.CHUNK_NETS}) == [3, 4, 5, 6]
    assert all(E.NETS[net][2] // 64 <= 2 and E.NETS[net][1] == 1 for net in B.BEFORE)


@pytest.mark.parametrize("net", list(B.NETS))
def test_selector_plans_the_board_kernel(net):
    """kz_model_plan, host logic: the f16 engine with the table's max_batch and switches runs "board_conv_f16" (at least 160
    workgroups at max_batch), the split16 engine "board_conv_split16" where the table says so and the one-launch split tower
    where not, and the launch geometry is the table's for every launch."""
    game, depth, channels, head, kw, _, max_batch, switches, split = B.NETS[net]
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        assert model.plan(max_batch, capi.KZ_DTYPE_F16)[0] == "board_conv_f16"
        for n in B.launches(net):
            assert model.launch_geometry(max_batch, capi.KZ_DTYPE_F16, n) == (B.workgroups(net, n), 0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert B.workgroups(net, max_batch) >= 160
    planned = model.plan(max_batch, capi.KZ_DTYPE_F32_SPLIT16)[0]
    if split:
        assert planned == "board_conv_split16"
        for n in B.launches(net):
            assert model.launch_geometry(max_batch, capi.KZ_DTYPE_F32_SPLIT16, n) == (B.workgroups(net, n), 0)
        assert model.plan(max_batch, capi.KZ_DTYPE_F32)[0] == "conv_igemm_f32"  # tests/test_gpu_board_exact.py: F32_PATH
    else:
        assert planned.startswith("tower_resident_split16") and not B.wide_positions(net)
    assert max(B.launches(net)) <= max_batch


def every_mutant_differs(net, b, label):
    s0, p0 = b.ref_scalars.astype(np.float64), b.ref_policy.astype(np.float64)
    for name, spoil in B.mutants(net).items():
        s1, p1, _ = E.reference(b.tensors, b.meta, b.x, spoil=spoil, exact=False)
        changed = int((s1 != s0).sum() + (p1 != p0).sum())
        print(f"[mutant] {net} {label} {name}: {changed} output entries differ")
        assert changed > 0, f"{net} {label}: the reference does not see {name}"


@pytest.mark.parametrize("net,dense_at,wide", CASES, ids=IDS)
def test_conditions_oracle_and_mutants(net, dense_at, wide):
    b = B.build(net, dense_at, wide)
    rep = b.report
    assert b.seed == B.REDRAWN.get((net, dense_at, wide), B.SEED), "a redraw the table does not record"
    assert E.conditions_hold(rep, wide is not None)
    for name, v in rep.sums.items():
        assert v <= E.SUM_MAX, f"{name}: sum |a b| / step = {v}"
    if wide is None:
        for name, (v, roundtrips) in rep.stored.items():
            assert roundtrips and v <= E.STORED_MAX, f"{name}: {v} steps, f16 round trip {roundtrips}"
        if dense_at is not None:
            w = b.tensors[b.layers[dense_at] + ".weight"]
            assert b.layers[dense_at].startswith("common.tower.")
            density = B.NETS[net][5].get(dense_at, 1.0)
            assert np.count_nonzero(w) == w.size if density == 1.0 else np.count_nonzero(w) >= 0.9 * density * w.size
    else:
        for name, (exact, normal) in rep.split.items():
            assert exact and normal, name
        for name, (one_narrow, three_terms) in rep.lolo.items():
            assert one_narrow and three_terms, name
        at = wide[0]
        if at == "input":
            assert rep.lo_in["common.tower.0"][0] >= E.LIVE_SHARE and not any(m.any() for m in rep.lo_w.values())
        else:
            assert b.layers[at].startswith("common.tower.")
            assert rep.lo_w[b.layers[at]].any() and not any(m.any() for p, m in rep.lo_w.items() if p != b.layers[at])
    for p in b.layers:
        assert b.tensors[p + ".bias"].any(), f"{p}: an all-zero bias hides a bias indexing error"
    # the oracle returns the same bits: the first board, one in the middle, the last
    idx = np.array([0, B.BOARDS // 2, B.BOARDS - 1])
    oracle = O.OracleNet(b.blob)
    x32 = b.x[idx].astype(np.float32)
    assert np.array_equal(x32, O.encode_input_full(b.bits[idx], b.scalars_in[idx], oracle.n_scalar, oracle.n_bool, oracle.h, oracle.w))
    s, p = oracle.forward(x32, threads=4)
    assert np.array_equal(s, b.ref_scalars[idx]), "scalars"
    assert np.array_equal(p, b.ref_policy[idx]), "policy"
    # the mutants this network is there for
    names = set(B.mutants(net))
    assert any(n.startswith("chunk-") for n in names) == (net in B.CHUNK_NETS)
    assert any(n.startswith("quarter-") for n in names) == (net in B.QUARTER_NETS)
    assert ("stale-residual" in names) == (net in B.STALE_NETS)
    every_mutant_differs(net, b, IDS[CASES.index((net, dense_at, wide))])


@pytest.mark.parametrize("net", [n for n in B.NETS if B.wide_positions(n)])
def test_wide_coverage_of_the_tower(net):
    """The two coverage conditions of tests/test_exact_nets.py's test_wide_coverage on every tower layer: some variant feeds it
    lo halves in every 32-channel chunk and on LIVE_SHARE of its entries, some variant has a lo half in every weight fragment."""
    cover = B.coverage(net)
    tower = [p for p in B.build(net, None, B.wide_positions(net)[0]).layers if p.startswith("common.tower.")]
    assert len(tower) == 2 * B.NETS[net][1] + 1
    for p in tower:
        shares = {E.wide_id(w): lo_in[p][0] for w, (lo_in, _) in cover.items() if lo_in[p][1]}
        best = max(shares, key=shares.get) if shares else None
        print(f"[wide] {net} {p}: input lo on {shares.get(best, 0.0):.3f} of the entries ({best})")
        assert shares and shares[best] >= E.LIVE_SHARE, f"{p}: no variant feeds it lo halves in every chunk and on {E.LIVE_SHARE} of the entries"
        assert any(lo_w[p].all() for _, lo_w in cover.values()), f"{p}: no variant has a lo half in every weight fragment"


@pytest.mark.parametrize("net", B.BEFORE)
def test_no_mutant_can_be_expressed_on_the_networks_run_so_far(net):
    """go19_1x64, go19_1x128, go13_1x128: at most two chunks of 64 channels, at most two quarters, one block — the reference
    refuses every chunk, quarter and block one could name."""
    assert net in E.NETS and any(e[1] == net and e[5].startswith("board_conv") for e in _gpu_engines())
    b = E.build(net, None)
    depth, channels = b.meta["tower_depth"], b.meta["tower_channels"]
    assert depth == 1 and channels // 64 <= 2

    def refused(spoil):
        with pytest.raises(ValueError):
            E.reference(b.tensors, b.meta, b.x[:1], spoil=spoil, exact=False)
    for layer in ("common.tower.1.seq.0", "common.tower.1.seq.3"):
        for k in range(8):
            refused(dict(layer=layer, chunk=k))
    for block in range(4):
        for q in range(8):
            refused(dict(block=block, quarter=q))
        refused(dict(block=block, stale=True))
    # ... and the networks named for a mutant are not refused (every_mutant_differs runs them); a quarter below 2 is, anywhere
    big = B.build("go13_2x128", None)
    for spoil in (dict(block=1, stale=True), dict(block=3, stale=True), dict(block=2, quarter=1), dict(layer="common.tower.2.seq.0", chunk=1)):
        with pytest.raises(ValueError):
            E.reference(big.tensors, big.meta, big.x[:1], spoil=spoil, exact=False)


def _gpu_engines():
    from tests import test_gpu_exact as G
    return G.ENGINES
