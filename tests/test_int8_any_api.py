"""KZ_DTYPE_INT8_ANY (dtype 8) without a GPU: on a calibrated ResTower model it is exactly dtype 5's plan wherever dtype 5 has
one, and the per-layer plan "board_conv_i8" exactly where the rule of include/kz_hip.h holds — at least one block, a board of
2 .. 32 squares a side that fits a workgroup of the board-tile kernels, at most 512 channels after widening, NO minimum of
workgroups — and a refusal naming "dtype 8" elsewhere.  Then the shapes that must take the per-layer plan (dtype 4 refuses
every one of them), the refusals (dtype 4's, saying "dtype 8"; 6, 7 and 17 stay unknown), the switches (none is read), the
taps and the error profile (refused), the library's strings, the launch geometry and the committed path table of dtype 8."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import int8_board_nets as B
from tests import int8_nets
from tests import sweep_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import gen_path_table  # noqa: E402

INT8, HEADS, ANY = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8_ANY
BATCHES = (1, 8, 64, 256, 2048)
SWITCHES = ("KZ_FORCE_GENERIC", "KZ_KEEP_ACTIVATIONS", "KZ_NO_FUSED_HEADS", "KZ_NO_RESIDENT_F16G", "KZ_NO_BOARD_CONV", "KZ_TOWER_NB")
# (game, depth, channels, head, keywords): dtype 4 refuses every one of them
MUST_TAKE = [("go-19", 2, c, "conv", {}) for c in (64, 128, 192, 256, 320)] + [
    ("go-13", 2, 128, "conv", {}), ("go-9", 2, 256, "conv", {}), ("ataxx-7", 2, 384, "ataxx_conv", {}),
    ("chess", 2, 192, "attention", {})]


def res_model(game="chess", depth=2, channels=128, head="attention", seed=1, **kw):
    return capi.Model(blob=synth.random_model(game, depth, channels, head, seed=seed, **kw))


def calibrated(model):
    return model.quantize_int8([1.0] * len(model.range_sites()))


def refusal(fn, *args):
    with pytest.raises(capi.KzError) as e:
        fn(*args)
    return str(e.value)


def rule(game, depth, channels):
    """The per-layer plan's condition, restated: the tower runs widened to a multiple of 64 where that is at most 512 channels
    (as for every f16 and int8 plan), its int8 images to the next multiple of 128."""
    size = synth.game_spec(game)["size"]
    return depth >= 1 and 2 <= size <= 32 and B.geometry(size, size)[1] >= 1 and B.widened(channels) <= 512


def head_launches_of(model, max_batch):
    """Launches of the f16 engine's head kernels behind a materialised tower output: what the per-layer f16 plan has beyond its
    encode and 1 + 2 depth tower launches (KZ_FORCE_GENERIC: the per-layer f16 path of any ResTower)."""
    os.environ["KZ_FORCE_GENERIC"] = "1"
    try:
        path, launches = model.plan(max_batch, capi.KZ_DTYPE_F16)
    finally:
        del os.environ["KZ_FORCE_GENERIC"]
    assert path in ("conv_igemm_f16", "board_conv_f16"), path
    return launches - (2 + 2 * model.info.tower_depth)


def all_cases():
    for case in sweep_cases.CASES:
        yield case.id, case.game, case.depth, case.channels, case.head, case.kw
    for name, (game, depth, channels, head, kw) in int8_nets.NETS.items():
        yield name, game, depth, channels, head, kw


def test_the_value_in_the_bindings():
    header = open(os.path.join(REPO, "include", "kz_hip.h")).read()
    assert re.search(r"^#define KZ_DTYPE_INT8_ANY 8\b", header, flags=re.M) and ANY == 8
    assert "6 and 7" in header  # the header says the two values in between stay unknown


def test_dtype_8_is_dtype_5_where_it_plans_and_the_per_layer_plan_where_the_rule_holds():
    took, refused = set(), 0
    for name, game, depth, channels, head, kw in all_cases():
        model = res_model(game, depth, channels, head, seed=11, **kw)
        assert not model.supports_dtype(ANY), name
        assert "dtype 8" in refusal(model.plan, 64, ANY), name
        if "attention" in kw or head == "none" or depth < 1:
            refusal(model.quantize_int8, [1.0])
            continue
        quant = calibrated(model)
        if quant.supports_dtype(HEADS):
            assert quant.supports_dtype(ANY), name
            for mb in BATCHES:
                assert quant.plan(mb, ANY) == quant.plan(mb, HEADS), (name, mb)
                assert quant.launch_geometry(mb, ANY, mb) == quant.launch_geometry(mb, HEADS, mb), (name, mb)
        elif rule(game, depth, channels):
            assert quant.supports_dtype(ANY), name
            for mb in BATCHES:  # (no minimum of workgroups: max_batch 1 plans as 2048 does)
                assert quant.plan(mb, ANY) == ("board_conv_i8", 2 + 2 * depth + head_launches_of(model, mb)), (name, mb)
            took.add((game, channels))
        else:
            refused += 1
            assert not quant.supports_dtype(ANY), name
            msg = refusal(quant.plan, 64, ANY)
            assert "dtype 8" in msg and "unknown dtype" not in msg and "KZ_" not in msg, msg
    assert len(took) >= 8 and {g for g, _ in took} >= {"go-19", "go-9"}, took


@pytest.mark.parametrize("game,depth,channels,head,kw", MUST_TAKE, ids=[f"{g}-{d}x{c}-{h}" for g, d, c, h, _ in MUST_TAKE])
def test_shapes_that_must_take_board_conv_i8(game, depth, channels, head, kw):
    model = res_model(game, depth, channels, head, **kw)
    quant = calibrated(model)
    assert not quant.supports_dtype(INT8) and not quant.supports_dtype(HEADS)
    assert "dtype 4" in refusal(quant.plan, 256, INT8)
    assert quant.supports_dtype(ANY)
    size = synth.game_spec(game)["size"]
    for mb in BATCHES:
        path, launches = quant.plan(mb, ANY)
        assert path == "board_conv_i8" and launches == 2 + 2 * depth + head_launches_of(model, mb), (mb, path, launches)
        for batch in (1, mb):
            assert quant.launch_geometry(mb, ANY, batch) == (B.workgroups(batch, size, size, channels), 0)
    # every other dtype of the calibrated model is its source's
    for dtype in (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16):
        assert quant.supports_dtype(dtype) == model.supports_dtype(dtype)
        if model.supports_dtype(dtype):
            assert quant.plan(256, dtype) == model.plan(256, dtype)


def test_launch_geometry_is_board_conv_workgroups_on_the_widened_tower():
    assert B.workgroups(512, 19, 19, 256) == 512 * 4 and B.workgroups(13, 19, 19, 192) == 13 * 4
    assert B.workgroups(2048, 9, 9, 256) == 512 * 4 and B.workgroups(13, 7, 7, 64) == 3 * 2
    quant = calibrated(res_model("go-19", 2, 96, "conv"))  # 96 channels: int8 images of 128
    assert quant.launch_geometry(64, ANY, 13) == (13 * 2, 0)


def test_refusals_say_dtype_8_and_other_values_stay_unknown():
    for model in (res_model(), res_model("ataxx-7", 2, 128, "ataxx_conv"), res_model("go-19", 1, 64, "conv"),
                  res_model("chess", 2, 192, "attention"), res_model("chess", 0, 128, "attention")):
        msg = refusal(model.plan, 64, ANY)
        assert msg.startswith("kz_model_plan: unknown dtype 8 for a model that carries no int8 calibration"), msg
        assert "KZ_" not in msg and "dtype 4" not in msg
        assert msg.replace("dtype 8", "dtype 4") == refusal(model.plan, 64, INT8)  # dtype 4's message otherwise
    att = res_model("chess", 1, 64, "attention", attention=(4, 16, 16, 96))
    dense = res_model("sttt", 1, 64, "none", dense_network=False)
    for model, needle in ((att, "attention-tower"), (dense, "DenseNetwork")):
        msg = refusal(model.plan, 64, ANY)
        assert needle in msg and "(dtype 8)" in msg and msg.replace("dtype 8", "dtype 4") == refusal(model.plan, 64, INT8)
    # calibrated, and no kernel either way: more than 512 channels after widening
    wide = calibrated(res_model("ataxx-7", 1, 576, "ataxx_conv"))
    msg = refusal(wide.plan, 64, ANY)
    assert "unknown dtype" not in msg and "(dtype 8) has no kernel for this shape" in msg and "the model is calibrated" in msg
    assert "board_conv_i8" in msg and not wide.supports_dtype(ANY)
    quant = calibrated(res_model("go-19", 2, 128, "conv"))
    for dtype in (6, 7, 17):
        assert refusal(quant.plan, 64, dtype) == "kz_model_plan: unknown dtype"
        assert not quant.supports_dtype(dtype)
        assert refusal(quant.launch_geometry, 64, dtype, 1) == "kz_model_launch_geometry: unknown dtype"


def test_dtype_8_reads_none_of_the_switches(monkeypatch):
    for game, channels, head in (("go-19", 128, "conv"), ("go-19", 96, "conv"), ("go-9", 256, "conv"), ("ataxx-7", 128, "ataxx_conv"),
                                 ("chess", 192, "attention")):
        quant = calibrated(res_model(game, 2, channels, head))
        plain = [quant.plan(mb, ANY) for mb in BATCHES]
        for name in SWITCHES:
            monkeypatch.setenv(name, "1")
            assert quant.supports_dtype(ANY) and [quant.plan(mb, ANY) for mb in BATCHES] == plain, name
            monkeypatch.delenv(name)


def test_taps_and_the_error_profile_refuse_dtype_8():
    for game, channels, head in (("ataxx-7", 128, "ataxx_conv"), ("go-19", 128, "conv")):
        quant = calibrated(res_model(game, 2, channels, head))
        bits, scalars = synth.random_boards(game, 2, seed=1)
        four = refusal(quant.tower_taps_path, 64, INT8)
        eight = refusal(quant.tower_taps_path, 64, ANY)
        assert "no tap instance" in eight and "dtype 8" in eight and eight.replace("dtype 8", "dtype 4") == four
        assert "dtype 8" in refusal(quant.tower_taps, 0, 64, ANY, bits, scalars)
        assert "dtype 8" in refusal(quant.error_profile, 0, 64, ANY, bits, scalars)


def test_the_library_names_the_path_and_not_the_constant():
    out = subprocess.run(["strings", "-n", "4", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "board_conv_i8" in out and "kz_board_conv_i8" in out
    # no KZ_DTYPE_ identifier beyond the three the older messages have always named (tests/test_abi.py: the documented ones)
    assert set(re.findall(r"KZ_DTYPE_\w+", out)) <= {"KZ_DTYPE_F32", "KZ_DTYPE_F16", "KZ_DTYPE_F32_SPLIT16"}


def test_committed_path_table_is_what_the_selector_chooses():
    committed = json.load(open(gen_path_table.OUT_INT8_ANY))
    fresh = json.loads(json.dumps(gen_path_table.build_int8_any()))
    assert committed == fresh, "regenerate with tools/gen_path_table.py --int8-any"
    five = json.load(open(gen_path_table.OUT_INT8_HEADS))
    assert set(fresh["cases"]) == set(five["cases"]) and fresh["max_batch"] == five["max_batch"]
    assert set(fresh["uncalibrated"].values()) == {"refused"}
    n_board = 0
    for name, row in fresh["cases"].items():
        for got, was in zip(row, five["cases"][name]):
            if was not in ("refused", "no calibration"):
                assert got == was, name  # dtype 5's entry wherever it has one
            else:
                assert got == was or got.startswith("board_conv_i8 "), (name, got, was)
                n_board += got.startswith("board_conv_i8 ")
    assert n_board > 0
    assert json.loads(json.dumps(gen_path_table.build_int8_heads())) == five, "dtype 5's table must not change"
