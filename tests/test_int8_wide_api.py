"""The int8 launch's wide tiles without a GPU: kz_model_launch_geometry — the model-level twin of kz_engine_launch_geometry, host
logic like kz_model_plan — against a Python restatement of the tile rule (include/kz_hip.h):

  narrow tiles     tests/test_int8_heads_api.py's: 64 rows at 256 channels; at 128 channels 112 rows for a board of at most 56
                   squares, else 64, else 96
  wide levels      256 channels, 8x8: 8 tiles (two boards), the tower alone — never with the heads inside.  128 channels: 64
                   squares 8 tiles, 81 squares 11, 49 or 25 squares 13; and with the heads inside 16 tiles (three 9x9, four 8x8
                   boards) in front of the 8 / 11 — the tower alone was measured slower in sixteen tiles than in eleven at every
                   batch, so that level exists with the heads inside only
  thresholds       a level is taken when the launch's batch gives at least T workgroups of it, measured: the tower alone 256
                   (128 for the two boards at 256 channels, as before); with the heads inside 128, and 342 for sixteen tiles.
                   Below the lowest one the narrow tiles.  The engine's max_batch decides whether it is wide at all, each
                   launch's own batch which level it takes
  the tail-fit cap dtype 5 where the narrow tiles carry the heads: a level whose tail does not fit — more than four boards, or
                   the tail's floats beyond min(16 KB, 160 KB - the level's own LDS) — is skipped, not the levels below it

over every network of tests/int8_nets.py and every sweep case that runs in int8, dtypes 4 and 5, max_batch 64 / 256 / 2048 and
batches on both sides of every threshold.  Then the cases the rule is known by, by name; the plans, which do not change; the
refusals, which are kz_model_plan's under the function's own name; and the bindings."""
import json
import os
import re

import pytest

from kzero_amd import capi, synth
from tests import int8_nets
from tests import sweep_cases
from tests.test_int8_heads_api import calibrated, fused, own_lds_bytes, refusal, res_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT8, HEADS = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS
MAX_BATCHES = (64, 256, 2048)
T_PLAIN_128, T_PLAIN_256, T_HEADS, T_HEADS_16 = 256, 128, 128, 342  # workgroups a level must fill


def threshold(cp, nt, heads):
    if heads:
        return T_HEADS_16 if nt == 16 else T_HEADS
    return T_PLAIN_256 if cp == 256 else T_PLAIN_128


def narrow_tiles(cp, hw):
    if cp == 256:
        return 4 if hw <= 64 else 0
    return 7 if 2 * hw <= 112 else 4 if hw <= 64 else 6 if hw <= 96 else 0


def wide_levels(cp, hw, heads):
    """Widest first."""
    if cp == 256:
        return [8] if hw == 64 and not heads else []
    if hw in (64, 81):
        return ([16] if heads else []) + [8 if hw == 64 else 11]
    return [13] if hw in (49, 25) else []


def tail_fits(cp, nt, hw, head, kw):
    """test_int8_heads_api.fused's count for a level of nt tiles: at most four boards, the floats within the scratch."""
    if cp == 256 and nt != 4:
        return False  # (<256, 8> is compiled without the tail)
    nb = nt * 16 // hw
    hc, hs = kw.get("scalar_hidden_channels", 4), kw.get("scalar_hidden_size", 32)
    if nb > 4:
        return False
    floats = nb * hc * hw + nb * hw + nb * hs + 5 * hs + (256 // hs) * nb * hs
    return floats * 4 <= min(16 * 1024, 160 * 1024 - own_lds_bytes(cp, nt))


def levels_of(game, channels, head, kw, dtype):
    """(widened channels, squares, the heads are inside, the levels the plan may take)"""
    hw = synth.game_spec(game)["size"] ** 2
    cp = -(-channels // 64) * 64
    heads = dtype == HEADS and fused(game, channels, head, kw)[0]
    levels = wide_levels(cp, hw, heads)
    if heads:
        levels = [nt for nt in levels if tail_fits(cp, nt, hw, head, kw)]
    return cp, hw, heads, levels


def geometry(game, channels, head, kw, dtype, max_batch, batch):
    """(workgroups, boards per workgroup) by the rule."""
    cp, hw, heads, levels = levels_of(game, channels, head, kw, dtype)

    def fills(nt, n):
        per = nt * 16 // hw
        return -(-n // per) >= threshold(cp, nt, heads)

    nt = narrow_tiles(cp, hw)
    if any(fills(level, max_batch) for level in levels):  # the plan is wide: each launch takes the widest level it fills
        nt = next((level for level in levels if fills(level, batch)), nt)
    per = nt * 16 // hw
    return -(-batch // per), per


def edge_batches(game, channels, head, kw, dtype, max_batch):
    """Both sides of every threshold of every level of the shape under either dtype, and the ends."""
    out = {0, 1, max_batch, max_batch - 1, 37}
    for dt in (INT8, HEADS):
        cp, hw, heads, levels = levels_of(game, channels, head, kw, dt)
        for nt in levels:
            per, t = nt * 16 // hw, threshold(cp, nt, heads)
            first = (t - 1) * per + 1  # the smallest batch of t workgroups
            out |= {first - 1, first, first + 1, t * per, t * per + 1}
    return sorted(b for b in out if 0 <= b <= max_batch)


def check_geometry(name, quant, game, channels, head, kw):
    n = 0
    for dtype in (INT8, HEADS):
        for mb in MAX_BATCHES:
            for batch in edge_batches(game, channels, head, kw, dtype, mb):
                want = geometry(game, channels, head, kw, dtype, mb, batch)
                assert quant.launch_geometry(mb, dtype, batch) == want, (name, dtype, mb, batch, want)
                n += 1
    return n


def int8_model(game, depth, channels, head, kw, seed=1):
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=seed, **kw))
    try:
        quant = calibrated(model)
    except capi.KzError:
        return None
    return quant if quant.supports_dtype(INT8) else None


def test_the_rule_across_the_int8_networks():
    for name, (game, depth, channels, head, kw) in int8_nets.NETS.items():
        quant = int8_model(game, depth, channels, head, kw)
        assert quant is not None, name
        assert check_geometry(name, quant, game, channels, head, kw) >= 30


def test_the_rule_across_the_sweep_shapes():
    ran = wide = 0
    for case in sweep_cases.CASES:
        quant = int8_model(case.game, case.depth, case.channels, case.head, case.kw, seed=11)
        if quant is None:
            continue
        ran += 1
        check_geometry(case.id, quant, case.game, case.channels, case.head, case.kw)
        wide += bool(levels_of(case.game, case.channels, case.head, case.kw, INT8)[3])
    assert ran >= 20 and wide >= 6  # chess, Ataxx 5 / 7 / 8 and Go 9x9 at 128 channels, 8x8 at 256


def test_go9_takes_three_two_and_one_board_by_the_batch():
    game, depth, channels, head, kw = int8_nets.NETS["go9_3x128"]
    quant = int8_model(game, depth, channels, head, kw)
    mb = 2048
    five = lambda batch: quant.launch_geometry(mb, HEADS, batch)
    assert five(2048) == (683, 3)
    assert five(3 * 341 + 1) == (342, 3)   # the smallest batch of 342 workgroups of three: 1024 boards
    assert five(3 * 341) == (512, 2)       # one level below: two boards in eleven tiles
    assert five(255) == (128, 2)
    assert five(254) == (254, 1)           # below the lowest threshold: one board in six tiles
    assert quant.plan(mb, HEADS) == ("tower_resident_i8+heads", 1)
    # an engine that fills the eleven-tile level only never takes sixteen tiles, one that fills none is narrow
    assert quant.launch_geometry(1023, HEADS, 1023) == (512, 2) and quant.launch_geometry(254, HEADS, 254) == (254, 1)
    # the tower alone: two boards from 256 workgroups, never three (sixteen tiles lost to eleven at every measured batch)
    four = lambda batch: quant.launch_geometry(mb, INT8, batch)
    assert four(2048) == (1024, 2) and four(511) == (256, 2) and four(510) == (510, 1)
    assert quant.launch_geometry(8192, INT8, 8192) == (4096, 2)


def test_a_tail_that_does_not_fit_sixteen_tiles_stays_a_level_below():
    # 9,728 B are left behind sixteen tiles: three Go boards with the default scalar head fit (8,956 B), with an 8-channel /
    # 64-hidden one they do not (13,868 B) — but the eleven-tile level, with 16 KB, takes them
    kw = dict(scalar_hidden_channels=8, scalar_hidden_size=64)
    quant = int8_model("go-9", 2, 128, "conv", kw)
    assert quant.plan(2048, HEADS) == ("tower_resident_i8+heads", 1)
    assert tail_fits(128, 11, 81, "conv", kw) and not tail_fits(128, 16, 81, "conv", kw) and tail_fits(128, 16, 81, "conv", {})
    for mb in (2048, 8192):
        for batch in edge_batches("go-9", 128, "conv", kw, HEADS, mb) + [mb]:
            assert quant.launch_geometry(mb, HEADS, batch)[1] in (1, 2), (mb, batch)
    assert quant.launch_geometry(2048, HEADS, 2048) == (1024, 2)
    assert int8_model("go-9", 2, 128, "conv", {}).launch_geometry(2048, HEADS, 2048) == (683, 3)  # (the default head does)
    # four 8x8 boards (10,368 B) do not fit sixteen tiles either: two per workgroup, with the heads inside and without
    eight = int8_model("ataxx-8", 2, 128, "ataxx_conv", {})
    assert eight.plan(2048, HEADS) == ("tower_resident_i8+heads", 1)
    assert eight.launch_geometry(2048, HEADS, 2048) == (1024, 2) and eight.launch_geometry(2048, INT8, 2048) == (1024, 2)
    assert eight.launch_geometry(2048, HEADS, 255) == (128, 2) and eight.launch_geometry(2048, INT8, 255) == (255, 1)


def test_eight_5x5_boards_without_the_heads_four_with_them():
    game, depth, channels, head, kw = int8_nets.NETS["ataxx5_2x128"]
    quant = int8_model(game, depth, channels, head, kw)
    assert quant.launch_geometry(2048, INT8, 2048) == (256, 8)
    assert quant.launch_geometry(2048, INT8, 2040) == (510, 4)  # 255 workgroups of eight: the narrow tiles
    assert quant.plan(2048, HEADS) == ("tower_resident_i8+heads", 1)
    assert quant.launch_geometry(2048, HEADS, 2048) == (512, 4)
    # 7x7: four boards in thirteen tiles — from 128 workgroups with the heads inside, from 256 without
    game, depth, channels, head, kw = int8_nets.NETS["ataxx7_2x128"]
    quant = int8_model(game, depth, channels, head, kw)
    assert quant.launch_geometry(1024, HEADS, 509) == (128, 4) and quant.launch_geometry(1024, HEADS, 508) == (254, 2)
    assert quant.launch_geometry(1024, INT8, 1021) == (256, 4) and quant.launch_geometry(1024, INT8, 1020) == (510, 2)


def test_256_channels_are_as_they_were():
    game, depth, channels, head, kw = int8_nets.NETS["chess_2x256_att"]
    quant = int8_model(game, depth, channels, head, kw)
    for dtype in (INT8, HEADS):  # (an attention head: dtype 5 is dtype 4's plan)
        assert quant.launch_geometry(256, dtype, 255) == (128, 2) and quant.launch_geometry(256, dtype, 254) == (254, 1)
        assert quant.launch_geometry(4096, dtype, 4096) == (2048, 2)
    conv8 = int8_model("ataxx-8", 2, 256, "ataxx_conv", {})
    assert conv8.launch_geometry(2048, INT8, 2048) == (1024, 2) and conv8.launch_geometry(2048, HEADS, 2048) == (2048, 1)


def test_plans_are_the_committed_path_tables():
    tables = {dtype: json.load(open(os.path.join(REPO, "tests", "golden", name)))
              for dtype, name in ((INT8, "path_table_int8.json"), (HEADS, "path_table_int8_heads.json"))}
    n = 0
    for case in sweep_cases.CASES:
        quant = int8_model(case.game, case.depth, case.channels, case.head, case.kw, seed=11)
        if quant is None:
            continue
        for dtype, table in tables.items():
            assert ["%s %d" % quant.plan(mb, dtype) for mb in table["max_batch"]] == table["cases"][case.id], (case.id, dtype)
            n += 1
    assert n >= 40
    for name, (game, depth, channels, head, kw) in int8_nets.NETS.items():  # (not in the tables: the rule of test_int8_heads_api)
        quant = int8_model(game, depth, channels, head, kw)
        want = ("tower_resident_i8+heads", 1) if fused(game, channels, head, kw)[0] else None
        for mb in MAX_BATCHES:
            four, five = quant.plan(mb, INT8), quant.plan(mb, HEADS)
            assert four[0] == "tower_resident_i8" and four == quant.plan(64, INT8) and five == (want or four), (name, mb)


def test_the_engine_function_and_the_model_function_agree_on_other_dtypes():
    # every tower kind through the same helper: where no calibration is needed the model function answers what kz_model_plan
    # plans, for the dtypes it plans, and refuses what it refuses, under its own name
    n = 0
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        for dtype in (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16, INT8, HEADS):
            try:
                model.plan(256, dtype)
            except capi.KzError as e:
                msg = refusal(model.launch_geometry, 256, dtype, 5)
                assert msg == str(e).replace("kz_model_plan: ", "kz_model_launch_geometry: ", 1), (case.id, dtype)
                continue
            wgs, per = model.launch_geometry(256, dtype, 256)
            assert wgs >= 1 and (per == 0 or wgs == -(-256 // per)), (case.id, dtype, wgs, per)
            assert model.launch_geometry(256, dtype, 0)[0] == 0 or per == 0
            n += 1
    assert n >= 100
    model = res_model()
    assert refusal(model.launch_geometry, 0, INT8, 0) == "kz_model_launch_geometry: max_batch must be positive"
    assert refusal(model.launch_geometry, 64, 17, 1) == "kz_model_launch_geometry: unknown dtype"
    assert refusal(model.launch_geometry, 64, capi.KZ_DTYPE_F16, 65) == "kz_model_launch_geometry: batch out of range"
    assert refusal(model.launch_geometry, 64, capi.KZ_DTYPE_F16, -1) == "kz_model_launch_geometry: batch out of range"
    assert refusal(model.launch_geometry, 64, INT8, 1).startswith("kz_model_launch_geometry: unknown dtype 4 for a model that carries no int8 calibration")
    # the f16 family's own wide tiles, through the shared helper
    go = res_model("go-9", 2, 128, "conv")
    assert go.launch_geometry(2048, capi.KZ_DTYPE_F16, 2048) == (683, 3) and go.launch_geometry(2048, capi.KZ_DTYPE_F16, 200) == (200, 1)


def test_header_shim_and_capi_bind_the_function():
    header = open(os.path.join(REPO, "include", "kz_hip.h")).read()
    assert re.search(r"int kz_model_launch_geometry\(const kz_model \*model, int max_batch, int dtype, int batch,\s*int \*workgroups, "
                     r"int \*boards_per_workgroup\);", header)
    shim = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
    assert "fn kz_model_launch_geometry(model: *const c_void, max_batch: c_int, dtype: c_int, batch: c_int, workgroups: *mut c_int, boards_per_workgroup: *mut c_int) -> c_int;" in shim
    assert "pub fn launch_geometry(&self, max_batch: usize, dtype: i32, batch: usize) -> (usize, usize)" in shim
    assert "kz_model_launch_geometry" in capi.SIGNATURES and hasattr(capi.load(), "kz_model_launch_geometry")
