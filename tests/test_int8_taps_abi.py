"""The int8 taps' boundary without a GPU (include/kz_hip.h, "int8 taps and error profile"): the three entries are exported and
bound in capi and in hip.rs, kz_int8_site_error is 120 bytes field for field, every model-level refusal is host logic in front of
any HIP call with a message of its own in the function's name, kz_model_int8_taps_path is kz_model_plan's tower without "+heads"
on every calibrated network of the committed int8 path tables — "tower_resident_i8" or "board_conv_i8", for dtypes 4, 5 and 8 —,
the three older tap entries refuse the int8 dtypes with the messages they had, and tools/int8_error_profile.py parses and prints
on --fake records."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import sweep_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import int8_error_profile as tool  # noqa: E402

INT8, HEADS, ANY = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8_ANY
ENTRIES = ("kz_model_int8_taps_path", "kz_model_int8_taps", "kz_model_int8_error_profile")
PATHS = ("tower_resident_i8", "board_conv_i8")
TABLES = {INT8: "path_table_int8.json", HEADS: "path_table_int8_heads.json", ANY: "path_table_int8_any.json"}
OLD_MESSAGE = ("the int8 tower (dtype %d) has no tap instance: its stored tensors are int8 images at a scale per site, which the taps' "
               "element formats do not hold")


def res_model(game="chess", depth=2, channels=128, head="attention", seed=1, **kw):
    return capi.Model(blob=synth.random_model(game, depth, channels, head, seed=seed, **kw))


def calibrated(model):
    return model.quantize_int8([1.0] * len(model.range_sites()))


def refusal(fn, *args):
    with pytest.raises(capi.KzError) as e:
        fn(*args)
    return str(e.value)


def test_the_three_entries_are_exported_and_bound():
    lib = capi.load()
    hip_rs = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
    externs = re.search(r'extern "C" \{(.*?)\n\}', hip_rs, flags=re.S).group(1)
    header = open(os.path.join(REPO, "include", "kz_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
        assert re.search(rf"\bfn {name}\(", externs), name
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    for method in ("int8_taps_path", "int8_taps", "int8_error_profile"):
        assert callable(getattr(capi.Model, method))
    assert "int8 taps and error profile" in header
    assert "counted per" in header and "site by kz_model_int8_error_profile" in header  # (the sentence about silent saturation)


def test_int8_site_error_is_120_bytes_field_for_field():
    assert C.sizeof(capi.Int8SiteError) == 120 and capi.INT8_SITE_ERROR_DTYPE.itemsize == 120
    names = ["image", "stream", "at_clamp", "ref_beyond", "exponent", "reserved"]
    assert [n for n, _ in capi.Int8SiteError._fields_] == list(capi.INT8_SITE_ERROR_DTYPE.names) == names
    offsets = [getattr(capi.Int8SiteError, n).offset for n in names]
    assert offsets == [capi.INT8_SITE_ERROR_DTYPE.fields[n][1] for n in names] == [0, 48, 96, 104, 112, 116]
    assert capi.INT8_SITE_ERROR_DTYPE["image"] == capi.INT8_SITE_ERROR_DTYPE["stream"] == capi.SITE_ERROR_DTYPE
    assert capi.INT8_SITE_ERROR_DTYPE["at_clamp"] == capi.INT8_SITE_ERROR_DTYPE["ref_beyond"] == np.uint64
    assert capi.INT8_SITE_ERROR_DTYPE["exponent"] == capi.INT8_SITE_ERROR_DTYPE["reserved"] == np.int32
    hip_rs = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\n#\[derive[^\n]*\]\npub struct KzInt8SiteError \{(.*?)\}", hip_rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("image", "KzSiteError"), ("stream", "KzSiteError"), ("at_clamp", "u64"),
                                                        ("ref_beyond", "u64"), ("exponent", "i32"), ("reserved", "i32")]


def _calls(model, max_batch, dtype):
    """The three entries on `model` with well-formed dummy arguments: (name, callable) — a refusal raises KzError."""
    bits = np.zeros((1, max(model.info.bits_bytes, 1)), np.uint8)
    scalars = np.zeros((1, max(model.info.input_scalar_channels, 1)), np.float32)
    return [("kz_model_int8_taps_path", lambda: model.int8_taps_path(max_batch, dtype)),
            ("kz_model_int8_taps", lambda: model.int8_taps(0, max_batch, dtype, bits, scalars, 0, 1)),
            ("kz_model_int8_error_profile", lambda: model.int8_error_profile(0, max_batch, dtype, bits, scalars))]


REFUSALS = {
    # what is refused: (model, max_batch, dtype, a phrase of the message)
    "dtype_f16": (lambda: calibrated(res_model()), 8, capi.KZ_DTYPE_F16, "not an int8 dtype"),
    "dtype_f32": (lambda: calibrated(res_model()), 8, capi.KZ_DTYPE_F32, "not an int8 dtype"),
    "dtype_7": (lambda: calibrated(res_model()), 8, 7, "not an int8 dtype"),
    "uncalibrated": (lambda: res_model(), 8, INT8, "not calibrated"),
    "uncalibrated_go19": (lambda: res_model("go-19", 2, 128, "conv"), 8, ANY, "not calibrated"),
    "attention_tower": (lambda: res_model("chess", 1, 64, "attention", attention=(4, 16, 16, 96)), 8, INT8, "AttentionTower"),
    "dense_network": (lambda: res_model("sttt", 1, 64, "none", dense_network=False), 8, HEADS, "DenseNetwork"),
    "no_blocks": (lambda: res_model("chess", 0, 128, "attention"), 8, ANY, "without blocks"),
    "shape_dtype_4": (lambda: calibrated(res_model("go-19", 2, 128, "conv")), 8, INT8, "does not run in dtype 4"),
    "shape_dtype_5": (lambda: calibrated(res_model("chess", 2, 192, "attention")), 8, HEADS, "does not run in dtype 5"),
    "shape_dtype_8": (lambda: calibrated(res_model("ataxx-7", 1, 576, "ataxx_conv")), 8, ANY, "does not run in dtype 8"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_model_level_refusals_need_no_gpu(case):
    make, max_batch, dtype, phrase = REFUSALS[case]
    model = make()
    for name, call in _calls(model, max_batch, dtype):
        msg = refusal(call)
        assert msg.startswith(name + ": ") and phrase in msg, (name, msg)
        if case.startswith("shape_"):  # ... saying why as plan_path says it
            why = refusal(model.plan, max_batch, dtype)
            assert why.startswith("kz_model_plan: ") and msg.endswith(why[len("kz_model_plan: "):]), (msg, why)


def test_every_refusal_has_a_message_of_its_own():
    messages = {refusal(make().int8_taps_path, max_batch, dtype) for make, max_batch, dtype, _ in REFUSALS.values()}
    assert len(messages) == len(REFUSALS)


def test_null_and_argument_checks_come_before_any_hip_call():
    lib = capi.load()
    model = calibrated(res_model())
    bits = np.zeros((1, model.info.bits_bytes), np.uint8)
    scalars = np.zeros((1, model.info.input_scalar_channels), np.float32)
    image, stream = np.zeros(1 << 16, np.int8), np.zeros(1 << 16, np.float32)
    out = np.zeros(5, capi.INT8_SITE_ERROR_DTYPE)
    buf = C.create_string_buffer(64)
    b, s, st = bits.ctypes.data, scalars.ctypes.data, bits.shape[1]
    nulls = [
        ("kz_model_int8_taps_path", lambda: lib.kz_model_int8_taps_path(None, 8, INT8, buf, len(buf))),
        ("kz_model_int8_taps", lambda: lib.kz_model_int8_taps(None, 0, 8, INT8, b, st, s, 1, 0, 1, image.ctypes.data, stream.ctypes.data)),
        ("kz_model_int8_taps", lambda: lib.kz_model_int8_taps(model._h, 0, 8, INT8, None, st, s, 1, 0, 1, image.ctypes.data, stream.ctypes.data)),
        ("kz_model_int8_taps", lambda: lib.kz_model_int8_taps(model._h, 0, 8, INT8, b, st, None, 1, 0, 1, image.ctypes.data, stream.ctypes.data)),
        ("kz_model_int8_taps", lambda: lib.kz_model_int8_taps(model._h, 0, 8, INT8, b, st, s, 1, 0, 1, None, None)),  # either may be null, not both
        ("kz_model_int8_error_profile", lambda: lib.kz_model_int8_error_profile(None, 0, 8, INT8, b, st, s, 1, out.ctypes.data)),
        ("kz_model_int8_error_profile", lambda: lib.kz_model_int8_error_profile(model._h, 0, 8, INT8, None, st, s, 1, out.ctypes.data)),
        ("kz_model_int8_error_profile", lambda: lib.kz_model_int8_error_profile(model._h, 0, 8, INT8, b, st, None, 1, out.ctypes.data)),
        ("kz_model_int8_error_profile", lambda: lib.kz_model_int8_error_profile(model._h, 0, 8, INT8, b, st, s, 1, None)),
    ]
    for name, call in nulls:
        assert call() != 0, name
        assert lib.kz_last_error().decode() == name + ": null argument"
    assert lib.kz_model_int8_taps_path(model._h, 8, INT8, buf, 4) != 0
    assert "buffer of at least" in lib.kz_last_error().decode()
    for args, phrase in (((1, 5, 1), "out of range (5 sites)"), ((1, 0, 0), "out of range (5 sites)"), ((1, -1, 1), "out of range (5 sites)"),
                         ((1, 4, 2), "out of range (5 sites)"), ((0, 0, 1), "batch 0 out of range"), ((9, 0, 1), "batch 9 out of range")):
        batch, first, count = args
        assert lib.kz_model_int8_taps(model._h, 0, 8, INT8, b, st, s, batch, first, count, image.ctypes.data, stream.ctypes.data) != 0
        msg = lib.kz_last_error().decode()
        assert msg.startswith("kz_model_int8_taps: ") and phrase in msg, msg
    assert "the batch size whose geometry is tapped" in msg
    assert lib.kz_model_int8_taps(model._h, 0, 8, INT8, b, st - 1, s, 1, 0, 1, image.ctypes.data, stream.ctypes.data) != 0
    assert "bits_stride too small" in lib.kz_last_error().decode()
    assert lib.kz_model_int8_error_profile(model._h, 0, 8, INT8, b, st, s, 9, out.ctypes.data) != 0
    assert lib.kz_last_error().decode().startswith("kz_model_int8_error_profile: batch 9 out of range")


@pytest.mark.parametrize("case", sweep_cases.CASES, ids=lambda c: c.id)
def test_taps_path_is_the_plans_tower_without_heads(case):
    """Every case of the three committed int8 path tables x its max_batch values: where the calibrated network has a plan the tap
    path is that plan's tower without "+heads", one of the two int8 kernels; where it has none the path is refused."""
    tables = {dtype: json.load(open(os.path.join(REPO, "tests", "golden", name))) for dtype, name in TABLES.items()}
    rows = {dtype: t["cases"][case.id] for dtype, t in tables.items()}
    model = res_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw)
    if rows[INT8][0] == "no calibration":
        assert all(set(r) == {"no calibration"} for r in rows.values())
        for dtype in TABLES:
            assert refusal(model.int8_taps_path, 8, dtype).startswith("kz_model_int8_taps_path: ")
        return
    quant = calibrated(model)
    for dtype, table in tables.items():
        for mb, entry in zip(table["max_batch"], rows[dtype]):
            assert refusal(model.int8_taps_path, mb, dtype).startswith("kz_model_int8_taps_path: ")  # (as loaded: not calibrated)
            if entry == "refused":
                msg = refusal(quant.int8_taps_path, mb, dtype)
                assert msg.startswith("kz_model_int8_taps_path: ") and f"does not run in dtype {dtype}" in msg, msg
                continue
            path = entry.split()[0]
            base = path[:-len("+heads")] if path.endswith("+heads") else path
            assert base in PATHS and quant.plan(mb, dtype)[0] == path
            assert quant.int8_taps_path(mb, dtype) == base, (case.id, dtype, mb)
    # dtype 5 taps what dtype 4 taps, dtype 8 what dtype 5 taps wherever dtype 5 has a plan
    for mb in tables[INT8]["max_batch"]:
        if quant.supports_dtype(INT8):
            assert quant.int8_taps_path(mb, INT8) == quant.int8_taps_path(mb, HEADS) == quant.int8_taps_path(mb, ANY) == "tower_resident_i8"


def test_the_tables_reach_both_kernels_and_the_heads():
    tables = {dtype: json.load(open(os.path.join(REPO, "tests", "golden", name))) for dtype, name in TABLES.items()}
    entries = {dtype: {e.split()[0] for row in t["cases"].values() for e in row} for dtype, t in tables.items()}
    assert "tower_resident_i8" in entries[INT8] and "tower_resident_i8+heads" in entries[HEADS]
    assert {"tower_resident_i8+heads", "board_conv_i8"} <= entries[ANY]


def test_the_three_older_entries_still_refuse_the_int8_dtypes():
    for game, channels, head in (("ataxx-7", 128, "ataxx_conv"), ("go-19", 128, "conv"), ("chess", 256, "attention")):
        quant = calibrated(res_model(game, 2, channels, head))
        bits, scalars = synth.random_boards(game, 2, seed=1)
        for dtype in (INT8, HEADS, ANY):
            want = OLD_MESSAGE % dtype
            assert refusal(quant.tower_taps_path, 64, dtype) == "kz_model_tower_taps_path: " + want
            assert refusal(quant.tower_taps, 0, 64, dtype, bits, scalars) == "kz_model_tower_taps: " + want
            assert refusal(quant.error_profile, 0, 64, dtype, bits, scalars) == "kz_model_error_profile: " + want


def test_the_tool_parses_and_prints_fake_records(tmp_path, capsys):
    path = tmp_path / "profile.json"
    out = tool.main(["--fake", "--synthetic", "go-19", "40", "256", "conv", "--dtype", "8", "--headroom", "1,2,4", "--calibrate-on", "64",
                     "--boards", "32", "--json", str(path)])
    captured = capsys.readouterr()
    assert json.loads(captured.out) == out == json.loads(path.read_text())
    assert out["dtype"] == 8 and out["calibrated_on"] == "64 other synthetic boards" and [c["headroom"] for c in out["columns"]] == [1.0, 2.0, 4.0]
    for col in out["columns"]:
        sites = col["sites"]
        assert [s["site"] for s in sites] == ["tower.0", "tower.1.mid", "tower.1", "tower.2.mid", "tower.3"]
        assert sites[1]["stream_rel_rms_err"] is None and sites[-1]["image_rel_rms_err"] is None and sites[-1]["at_clamp_share"] is None
        assert all(0 <= s["ref_beyond_share"] <= s["at_clamp_share"] <= 1 for s in sites[:-1])
        assert all(s["image_rel_rms_err"] > s["stream_rel_rms_err"] for s in sites[:-1:2])
    table = [ln for ln in captured.err.splitlines() if ln.startswith("# tower.")]
    assert len(table) == 5 and all(ln.count("%") == 6 for ln in table[:-1]) and "%" not in table[-1]
    head = [ln for ln in captured.err.splitlines() if "img rms/rms" in ln]
    assert len(head) == 1 and head[0].count("at clamp") == 3 and head[0].count("ref beyond") == 3
    assert "headroom 1 " in captured.err and "headroom 2 " in captured.err and "headroom 4 " in captured.err
    with pytest.raises(SystemExit):
        tool.main(["--fake", "--synthetic", "chess", "2", "256", "attention", "--dtype", "3"])
    with pytest.raises(AssertionError):
        tool.main(["--fake", "--model", "net.kzm", "--synthetic", "chess", "2", "256", "attention"])
    capsys.readouterr()
