"""KZ_DTYPE_BF16 without a GPU: the value in the three bindings, which networks the selector gives the one-launch bf16 tower
(`kz_model_supports_dtype`, `kz_model_plan`: the host logic `kz_engine_create` runs), which it refuses and with which message,
and the committed bf16 column of the path table (tests/golden/path_table_bf16.json, tools/gen_path_table.py --bf16)."""
import json
import os
import re
import subprocess
import sys

import pytest

from kzero_amd import capi, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import gen_path_table  # noqa: E402

BF16 = capi.KZ_DTYPE_BF16
HEADS_IN, HEADS_OUT = "tower_resident_bf16g+heads", "tower_resident_bf16g"


def test_the_three_bindings_agree_on_the_value():
    header = open(os.path.join(REPO, "include", "kz_hip.h")).read()
    assert re.search(r"^#define KZ_DTYPE_BF16 3\b", header, flags=re.M)
    assert capi.KZ_DTYPE_BF16 == 3
    hip_rs = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
    assert "pub const KZ_DTYPE_BF16: i32 = 3;" in hip_rs
    assert re.search(r'Ok\("bf16"\) => HipDtype::Bf16', hip_rs) and "HipDtype::Bf16 => KZ_DTYPE_BF16" in hip_rs
    assert re.search(r'Err\(_\) \| Ok\("parity"\)[^\n]*=> HipDtype::Parity', hip_rs), "parity stays the default"
    # the four values are distinct
    assert len({capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, BF16}) == 4


# attention head outside: the tower launch, the scalar head, conv_bulk, conv_under, the gather = 5 launches per batch
@pytest.mark.parametrize("game,channels,head,path,launches", [
    ("ataxx-7", 128, "ataxx_conv", HEADS_IN, 1), ("go-9", 128, "conv", HEADS_IN, 1), ("go-13", 128, "conv", HEADS_IN, 1),
    ("chess", 64, "attention", HEADS_OUT, 5), ("chess", 192, "attention", HEADS_OUT, 5), ("chess", 256, "attention", HEADS_OUT, 5),
    ("chess", 320, "attention", HEADS_OUT, 5), ("chess", 512, "attention", HEADS_OUT, 5),
    ("chess-hist-2", 256, "attention", HEADS_OUT, 5)])
def test_supported_networks_take_the_one_launch_tower(game, channels, head, path, launches):
    model = capi.Model(blob=synth.random_model(game, 2, channels, head, seed=1))
    assert model.supports_dtype(BF16)
    for max_batch in (1, 8, 64, 256, 2048):
        assert model.plan(max_batch, BF16) == (path, launches), max_batch
    # the other arithmetics' plans do not move (tests/test_path_table.py holds all of them)
    assert model.plan(256, capi.KZ_DTYPE_F16)[0].startswith("tower_resident_f16")


def test_no_fused_heads_switch_is_read(monkeypatch):
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=1))
    monkeypatch.setenv("KZ_NO_FUSED_HEADS", "1")
    path, launches = model.plan(64, BF16)
    assert path == HEADS_OUT and launches > 1
    # the one-launch tower is all this arithmetic has: the switches that pick a per-layer path change nothing
    monkeypatch.delenv("KZ_NO_FUSED_HEADS")
    for key in ("KZ_FORCE_GENERIC", "KZ_KEEP_ACTIVATIONS", "KZ_NO_RESIDENT_F16G", "KZ_NO_BOARD_CONV"):
        monkeypatch.setenv(key, "1")
        assert model.plan(64, BF16) == (HEADS_IN, 1), key
        monkeypatch.delenv(key)


def test_a_channel_count_off_the_lattice_is_widened():
    model = capi.Model(blob=synth.random_model("chess", 2, 96, "attention", seed=1))
    assert model.supports_dtype(BF16) and model.plan(64, BF16)[0] == HEADS_OUT


@pytest.mark.parametrize("what,game,depth,channels,head,kw,message", [
    ("go-19", "go-19", 2, 128, "conv", {}, "one-launch tower only"),
    ("per-layer-width", "go-13", 2, 256, "conv", {}, "one-launch tower only"),
    ("attention-tower", "chess", 3, 256, "attention", {"attention": (8, 16, 16, 256)}, "no attention-tower kernel"),
    ("dense-network", "chess", 3, 256, "none", {"dense_network": True}, "no DenseNetwork kernel"),
    ("no-blocks", "chess", 0, 256, "attention", {}, "at least one residual block")])
def test_refused_networks_and_their_messages(what, game, depth, channels, head, kw, message):
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
    assert model.supports_dtype(BF16) is False
    with pytest.raises(capi.KzError, match=message) as err:
        model.plan(64, BF16)
    assert "bf16" in str(err.value) and "dtype 3" in str(err.value)
    assert "KZ_DTYPE_BF16" not in str(err.value)  # (tests/test_abi.py: the library's KZ_ strings are the documented switches)


def test_each_refusal_has_a_message_of_its_own():
    seen = set()
    for game, depth, channels, head, kw in [("go-19", 2, 128, "conv", {}), ("chess", 3, 256, "attention", {"attention": (8, 16, 16, 256)}),
                                            ("chess", 3, 256, "none", {"dense_network": True}), ("chess", 0, 256, "attention", {})]:
        model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
        with pytest.raises(capi.KzError) as err:
            model.plan(64, BF16)
        seen.add(str(err.value))
    assert len(seen) == 4


def test_unknown_dtypes_stay_unknown():
    model = capi.Model(blob=synth.random_model("chess", 2, 64, "attention", seed=1))
    for dtype in (4, -1, 17):
        with pytest.raises(capi.KzError, match="unknown dtype"):
            model.plan(64, dtype)


def test_the_library_names_no_new_identifier():
    out = subprocess.run(["strings", "-n", "4", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "KZ_DTYPE_BF16" not in out
    assert "tower_resident_bf16g+heads" in out


def test_committed_bf16_column_is_what_the_selector_chooses():
    committed = json.load(open(gen_path_table.OUT_BF16))
    fresh = json.loads(json.dumps(gen_path_table.build_bf16()))
    assert committed["max_batch"] == fresh["max_batch"] == [1, 8, 256, 2048]
    assert set(committed["cases"]) == set(fresh["cases"])
    for case_id, row in fresh["cases"].items():
        assert committed["cases"][case_id] == row, f"{case_id}: regenerate with tools/gen_path_table.py --bf16"
    # the column is about something: the three kinds of entry all occur
    flat = [v for row in committed["cases"].values() for v in row]
    assert any(v.startswith(HEADS_IN + " ") for v in flat) and any(v.startswith(HEADS_OUT + " ") for v in flat) and "refused" in flat
