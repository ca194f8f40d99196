"""kz_model_quantize_int8 / kz_model_int8_site_exponents and the int8 plan (include/kz_hip.h, "int8 calibration"), without a
GPU: every refusal by its message; a calibrated model is its source for every other dtype; the exponents are
ceil(log2(m / 127)), exact powers of two times 127 included; kz_model_supports_dtype(4) before and after calibration across
the sweep shapes; the int8 path table against tests/golden/path_table_int8.json."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O
from tests import sweep_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import gen_path_table  # noqa: E402

INT8 = capi.KZ_DTYPE_INT8
OTHER = (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16)


def res_model(game="chess", depth=2, channels=128, head="attention", **kw):
    return capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))


def refusal(fn, *args):
    with pytest.raises(capi.KzError) as e:
        fn(*args)
    return str(e.value)


def test_every_refusal_has_a_message_of_its_own():
    res = res_model()
    n = len(res.range_sites())
    ok = np.ones(n, np.float32)
    lib = capi.load()
    out = C.c_void_p()

    def raw(model, site_max, n_sites, outp):
        assert lib.kz_model_quantize_int8(model, site_max, n_sites, outp) != 0
        return lib.kz_last_error().decode()

    def with_entry(i, v):
        m = ok.copy()
        m[i] = v
        return refusal(res.quantize_int8, m)

    messages = {
        "null model": raw(None, ok.ctypes.data, n, C.byref(out)),
        "n_sites": refusal(res.quantize_int8, ok[:-1]),
        "entry": with_entry(0, 0.0),
        "attention": refusal(capi.Model(blob=O.load_blob("chess_att2x64")).quantize_int8, ok),
        "dense": refusal(capi.Model(blob=O.load_blob("sttt_dn1x64")).quantize_int8, ok),
        "no blocks": refusal(res_model(depth=0, channels=64).quantize_int8, ok[:1]),
        "calibrated": refusal(res.quantize_int8(ok).quantize_int8, ok),
    }
    assert raw(res._h, None, n, C.byref(out)) == messages["null model"] == raw(res._h, ok.ctypes.data, n, None)
    assert len(set(messages.values())) == len(messages), messages
    for what, needle in (("null model", "null argument"), ("n_sites", f"has {n} range sites"), ("entry", "site_max[0]"),
                         ("attention", "AttentionTower"), ("dense", "DenseNetwork"), ("no blocks", "without blocks"),
                         ("calibrated", "calibrated already")):
        assert needle in messages[what] and messages[what].startswith("kz_model_quantize_int8: "), (what, messages[what])
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert f"site_max[{n - 2}]" in with_entry(n - 2, bad)
    for anything in (0.0, -1.0, np.nan, np.inf):  # the last site is not quantised: its entry is accepted and ignored
        m = ok.copy()
        m[-1] = anything
        assert list(res.quantize_int8(m).int8_site_exponents()) == [capi_exp(1.0)] * (n - 1)
    # shift first, then calibrate; and the exponents are a calibrated model's
    assert "shift first, then calibrate" in refusal(res.quantize_int8(ok).stream_shift, 1)
    assert list(res.stream_shift(1).quantize_int8(ok).int8_site_exponents()) == [-6] * (n - 1)
    assert "not calibrated" in refusal(res.int8_site_exponents)


def capi_exp(m):
    return int(np.ceil(np.log2(np.float64(m) / 127.0)))


def test_site_exponents_are_ceil_log2_of_the_maximum_over_127():
    res = res_model(depth=3)
    n = len(res.range_sites())
    rng = np.random.default_rng(5)
    for trial in range(8):
        m = np.exp(rng.uniform(np.log(1e-3), np.log(6e4), size=n)).astype(np.float32)
        assert list(res.quantize_int8(m).int8_site_exponents()) == [capi_exp(v) for v in m[:-1]]
    for k in range(-12, 10):  # exact powers of two times 127, and their f32 neighbours
        m = np.full(n, 127.0 * 2.0 ** k, np.float32)
        assert list(res.quantize_int8(m).int8_site_exponents()) == [k] * (n - 1)
        assert list(res.quantize_int8(np.nextafter(m, np.float32(np.inf))).int8_site_exponents()) == [k + 1] * (n - 1)
        assert list(res.quantize_int8(np.nextafter(m, np.float32(0))).int8_site_exponents()) == [k] * (n - 1)


def test_a_calibrated_model_is_its_source_for_every_other_dtype():
    for game, depth, channels, head in (("chess", 2, 256, "attention"), ("ataxx-7", 2, 128, "ataxx_conv"), ("go-9", 1, 96, "conv"),
                                        ("go-19", 1, 64, "conv")):
        src = res_model(game, depth, channels, head)
        quant = src.quantize_int8(np.full(len(src.range_sites()), 3.0, np.float32))
        for f, _ in capi.ModelInfo._fields_:
            assert getattr(src.info, f) == getattr(quant.info, f), f
        for dtype in OTHER:
            assert src.supports_dtype(dtype) == quant.supports_dtype(dtype)
            for mb in (1, 8, 256, 2048):
                if src.supports_dtype(dtype):
                    assert src.plan(mb, dtype) == quant.plan(mb, dtype), (game, dtype, mb)
        assert quant.range_sites() == src.range_sites()
        assert not src.supports_dtype(INT8)
    # independent of the source: it outlives it
    src = res_model()
    quant = src.quantize_int8(np.ones(len(src.range_sites()), np.float32))
    src.close()
    assert quant.plan(64, INT8) == ("tower_resident_i8", 2)


def test_supports_int8_before_and_after_calibration_across_the_sweep_shapes():
    took = set()
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        assert not model.supports_dtype(INT8), case.id
        assert "dtype 4" in refusal(model.plan, 64, INT8) or "int8" in refusal(model.plan, 64, INT8)
        if "attention" in case.kw or case.head == "none" or case.depth < 1:
            refusal(model.quantize_int8, [1.0])
            continue
        quant = model.quantize_int8([1.0] * len(model.range_sites()))
        g = synth.game_spec(case.game)
        hw, c_in, cp = g["size"] ** 2, g["n_scalar"] + g["n_bool"], -(-case.channels // 64) * 64
        expect = (cp == 256 and hw <= 64 and c_in <= 128) or (cp == 128 and hw <= 96 and c_in <= 64)
        assert quant.supports_dtype(INT8) == expect, case.id
        if expect:
            took.add((cp, hw))
            assert quant.plan(256, INT8)[0] == "tower_resident_i8"
        else:
            msg = refusal(quant.plan, 256, INT8)
            assert "no kernel for this shape" in msg and "the model is calibrated" in msg, msg
            assert "calibration is missing" not in msg
    msg = refusal(res_model().plan, 64, INT8)
    assert "calibration is missing" in msg and "KZ_" not in msg
    # to a model that carries no calibration dtype 4 is first of all an unknown dtype; to a calibrated one it never is
    assert msg.startswith("kz_model_plan: unknown dtype 4 for a model that carries no int8 calibration")
    wide = res_model("chess", 2, 192, "attention")
    assert "unknown dtype" in refusal(wide.plan, 64, INT8)
    assert "unknown dtype" not in refusal(wide.quantize_int8([1.0] * len(wide.range_sites())).plan, 64, INT8)
    assert {(256, 64), (128, 64), (128, 81), (128, 49)} <= took


def test_int8_reads_none_of_the_switches(monkeypatch):
    """A 96-channel tower runs widened to 128 whatever the environment says, and the plan is the same under every switch."""
    model = res_model("go-9", 2, 96, "conv")
    quant = model.quantize_int8([1.0] * len(model.range_sites()))
    plain = quant.plan(64, INT8)
    assert plain[0] == "tower_resident_i8"
    for name in ("KZ_FORCE_GENERIC", "KZ_KEEP_ACTIVATIONS", "KZ_NO_FUSED_HEADS", "KZ_NO_RESIDENT_F16G", "KZ_NO_BOARD_CONV", "KZ_TOWER_NB"):
        monkeypatch.setenv(name, "1")
        assert quant.supports_dtype(INT8) and quant.plan(64, INT8) == plain, name
        monkeypatch.delenv(name)
    for channels in (64, 192):  # no multiple of 64 to widen to that has a kernel
        m = res_model("go-9", 2, channels, "conv")
        assert not m.quantize_int8([1.0] * len(m.range_sites())).supports_dtype(INT8)


def test_committed_int8_path_table_is_what_the_selector_chooses():
    committed = json.load(open(gen_path_table.OUT_INT8))
    fresh = json.loads(json.dumps(gen_path_table.build_int8()))
    assert committed == fresh, "regenerate with tools/gen_path_table.py --int8"
    assert any(row[0].startswith("tower_resident_i8") for row in fresh["cases"].values())
    assert set(fresh["uncalibrated"].values()) == {"refused"}
