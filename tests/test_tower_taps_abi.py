"""The tower taps' boundary without a GPU (include/kz_hip.h, "tower taps and error profile"): the three entries are exported and
bound, kz_site_error is 48 bytes, every model-level refusal is host logic in front of any HIP call (like kz_model_plan) with a
message of its own in the function's name, and kz_model_tower_taps_path is kz_model_plan's tower without "+heads" wherever
that is a one-launch ResTower — and refused everywhere else."""
import ctypes as C

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import sweep_cases

DTYPES = (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16)
ENTRIES = ("kz_model_tower_taps_path", "kz_model_tower_taps", "kz_model_error_profile")
ONE_LAUNCH = ("tower_resident_f16", "tower_resident_f16g", "tower_resident_bf16g", "tower_resident_split16", "tower_resident_f32")


def test_the_three_entries_are_exported_and_bound():
    lib = capi.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name


def test_site_error_is_48_bytes():
    assert C.sizeof(capi.SiteError) == 48
    assert capi.SITE_ERROR_DTYPE.itemsize == 48
    assert [n for n, _ in capi.SiteError._fields_] == list(capi.SITE_ERROR_DTYPE.names) == [
        "max_abs_err", "sum_sq_err", "sum_sq_ref", "max_abs_ref", "count", "nonfinite"]


def _calls(model, max_batch, dtype):
    """The three entries on `model` with well-formed dummy arguments: (name, callable) — a refusal raises KzError."""
    bits = np.zeros((1, max(model.info.bits_bytes, 1)), np.uint8)
    scalars = np.zeros((1, max(model.info.input_scalar_channels, 1)), np.float32)
    return [("kz_model_tower_taps_path", lambda: model.tower_taps_path(max_batch, dtype)),
            ("kz_model_tower_taps", lambda: model.tower_taps(0, max_batch, dtype, bits, scalars, 0, 1, out=np.zeros(1 << 16, np.float32))),
            ("kz_model_error_profile", lambda: model.error_profile(0, max_batch, dtype, bits, scalars))]


REFUSALS = {
    # what is refused: (model, max_batch, dtype, a phrase of the message)
    "attention_tower": (lambda: synth.random_model("chess", 1, 64, "attention", seed=1, attention=(4, 16, 16, 96)), 8, capi.KZ_DTYPE_F16, "AttentionTower"),
    "dense_network": (lambda: synth.random_model("sttt", 1, 64, "none", seed=1, dense_network=False), 8, capi.KZ_DTYPE_F16, "DenseNetwork"),
    "no_blocks": (lambda: synth.random_model("chess", 0, 128, "attention", seed=1), 8, capi.KZ_DTYPE_F16, "without blocks"),
    "per_layer": (lambda: synth.random_model("go-19", 1, 64, "conv", seed=1), 8, capi.KZ_DTYPE_F16, "KZ_KEEP_ACTIVATIONS"),
    "dtype_not_supported": (lambda: synth.random_model("go-19", 1, 64, "conv", seed=1), 8, capi.KZ_DTYPE_BF16, "does not run in dtype 3"),
    "unknown_dtype": (lambda: synth.random_model("chess", 1, 128, "attention", seed=1), 8, 7, "unknown dtype 7"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_model_level_refusals_need_no_gpu(case):
    blob, max_batch, dtype, phrase = REFUSALS[case]
    model = capi.Model(blob=blob())
    for name, call in _calls(model, max_batch, dtype):
        with pytest.raises(capi.KzError) as e:
            call()
        assert str(e.value).startswith(name + ": ") and phrase in str(e.value), (name, str(e.value))


def test_every_refusal_has_a_message_of_its_own():
    messages = set()
    for case, (blob, max_batch, dtype, _) in REFUSALS.items():
        with pytest.raises(capi.KzError) as e:
            capi.Model(blob=blob()).tower_taps_path(max_batch, dtype)
        messages.add(str(e.value))
    assert len(messages) == len(REFUSALS)


def test_null_arguments_fail_with_a_message():
    lib = capi.load()
    model = capi.Model(blob=synth.random_model("chess", 1, 128, "attention", seed=1))
    bits = np.zeros((1, model.info.bits_bytes), np.uint8)
    scalars = np.zeros((1, model.info.input_scalar_channels), np.float32)
    out = np.zeros(1 << 16, np.float32)
    buf = C.create_string_buffer(64)
    F16 = capi.KZ_DTYPE_F16
    nulls = [
        ("kz_model_tower_taps_path", lambda: lib.kz_model_tower_taps_path(None, 8, F16, buf, len(buf))),
        ("kz_model_tower_taps", lambda: lib.kz_model_tower_taps(None, 0, 8, F16, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 1, 0, 1, out.ctypes.data)),
        ("kz_model_tower_taps", lambda: lib.kz_model_tower_taps(model._h, 0, 8, F16, None, bits.shape[1], scalars.ctypes.data, 1, 0, 1, out.ctypes.data)),
        ("kz_model_tower_taps", lambda: lib.kz_model_tower_taps(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1], None, 1, 0, 1, out.ctypes.data)),
        ("kz_model_tower_taps", lambda: lib.kz_model_tower_taps(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 1, 0, 1, None)),
        ("kz_model_error_profile", lambda: lib.kz_model_error_profile(None, 0, 8, F16, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 1, out.ctypes.data)),
        ("kz_model_error_profile", lambda: lib.kz_model_error_profile(model._h, 0, 8, F16, None, bits.shape[1], scalars.ctypes.data, 1, out.ctypes.data)),
        ("kz_model_error_profile", lambda: lib.kz_model_error_profile(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1], None, 1, out.ctypes.data)),
        ("kz_model_error_profile", lambda: lib.kz_model_error_profile(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 1, None)),
    ]
    for name, call in nulls:
        assert call() != 0, name
        assert lib.kz_last_error().decode() == name + ": null argument"
    # a buffer too small for the path's name is told how large it has to be
    assert lib.kz_model_tower_taps_path(model._h, 8, F16, buf, 4) != 0
    assert "buffer of at least" in lib.kz_last_error().decode()
    # and the argument checks of the two evaluating entries come before any HIP call as well
    for name, args, phrase in (("sites", (1, 3, 1), "out of range (3 sites)"), ("sites", (1, 0, 0), "out of range (3 sites)"), ("sites", (1, -1, 1), "out of range (3 sites)"),
                               ("batch", (0, 0, 1), "batch 0 out of range"), ("batch", (9, 0, 1), "batch 9 out of range")):
        batch, first, count = args
        assert lib.kz_model_tower_taps(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, batch, first, count, out.ctypes.data) != 0
        assert phrase in lib.kz_last_error().decode(), (name, lib.kz_last_error().decode())
    assert lib.kz_model_tower_taps(model._h, 0, 8, F16, bits.ctypes.data, bits.shape[1] - 1, scalars.ctypes.data, 1, 0, 1, out.ctypes.data) != 0
    assert "bits_stride too small" in lib.kz_last_error().decode()
    assert lib.kz_model_error_profile(model._h, 0, 8, capi.KZ_DTYPE_F32, bits.ctypes.data, bits.shape[1], scalars.ctypes.data, 1, out.ctypes.data) != 0
    assert "compares nothing" in lib.kz_last_error().decode()


@pytest.mark.parametrize("case", sweep_cases.CASES, ids=lambda c: c.id)
def test_taps_path_is_the_plans_tower_without_heads(case):
    """Every sweep case x four dtypes x max_batch 1 / 8 / 256 / 2048: where kz_model_plan names a one-launch ResTower the tap path
    is that name without "+heads"; everywhere else — a refused dtype, a per-layer plan, another kind of network — it is refused."""
    model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
    res_tower = "attention" not in case.kw and "dense_network" not in case.kw
    tapped = 0
    for dtype in DTYPES:
        for max_batch in (1, 8, 256, 2048):
            try:
                path = model.plan(max_batch, dtype)[0]
            except capi.KzError:
                path = None
            base = path[:-len("+heads")] if path and path.endswith("+heads") else path
            if res_tower and case.depth >= 1 and base in ONE_LAUNCH:
                assert model.tower_taps_path(max_batch, dtype) == base, (dtype, max_batch)
                tapped += 1
            else:
                with pytest.raises(capi.KzError) as e:
                    model.tower_taps_path(max_batch, dtype)
                assert str(e.value).startswith("kz_model_tower_taps_path: "), str(e.value)
    if not res_tower:
        assert tapped == 0
