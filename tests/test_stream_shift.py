"""kz_model_stream_shift and the range profile's site list, without a GPU: the shifted model is planned like its source, every
refusal has a message of its own, the sites are the tensors an f16 / split16 kernel stores, and the binding's shift_for follows
the rule of include/kz_hip.h: k = max(0, ceil(log2(m / 65504)) + headroom_bits)."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import oracle_lib as O

DTYPES = (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16)
NETS = [("ataxx-7", 2, 128, "ataxx_conv"), ("chess", 2, 256, "attention"), ("go-19", 2, 64, "conv")]


def plan_or_refusal(model, max_batch, dtype):
    try:
        return model.plan(max_batch, dtype)
    except capi.KzError as e:
        return "refused", str(e)


@pytest.mark.parametrize("game,depth,channels,head", NETS, ids=[f"{n[0]}-{n[1]}x{n[2]}" for n in NETS])
def test_the_shifted_model_is_planned_like_its_source(game, depth, channels, head):
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=5))
    refused = 0
    for k in (12, -12, 0, 3):
        shifted = model.stream_shift(k)
        for field, _ in capi.ModelInfo._fields_:
            assert getattr(shifted.info, field) == getattr(model.info, field), field
        for dtype in DTYPES:
            assert shifted.supports_dtype(dtype) == model.supports_dtype(dtype)
            for max_batch in (1, 8, 256, 2048):
                want = plan_or_refusal(model, max_batch, dtype)
                assert plan_or_refusal(shifted, max_batch, dtype) == want, (k, dtype, max_batch)
                refused += want[0] == "refused"
    # (Go 19x19 has no bf16 kernel: the refusal is the source's too; the other two networks run in all four)
    assert (refused > 0) == (game == "go-19")


def test_a_shifted_model_outlives_its_source():
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 16, "ataxx_conv", seed=1))
    shifted = model.stream_shift(4)
    model.close()
    assert shifted.plan(8, capi.KZ_DTYPE_F32)[0] == "conv_igemm_f32"
    assert shifted.stream_shift(-4).info.tower_depth == 2


def refusal(fn, *args):
    with pytest.raises(capi.KzError) as e:
        fn(*args)
    return str(e.value)


def f32_range_refusal(model):
    """Shifts by 2^-24 again and again: a weight of the stem leaves f32's normal range (2^-126) within six steps."""
    for _ in range(6):
        try:
            model = model.stream_shift(24)
        except capi.KzError as e:
            return str(e)
    raise AssertionError("six shifts by 2^-24 were accepted")


def test_every_refusal_has_a_message_of_its_own():
    res = capi.Model(blob=synth.random_model("ataxx-7", 2, 16, "ataxx_conv", seed=1))
    attention = capi.Model(blob=O.load_blob("chess_att2x64"))
    dense = capi.Model(blob=O.load_blob("sttt_dn1x64"))
    stem_only = capi.Model(blob=synth.random_model("chess", 0, 64, "attention", seed=1))
    messages = {
        "attention": refusal(attention.stream_shift, 1),
        "dense": refusal(dense.stream_shift, 1),
        "no blocks": refusal(stem_only.stream_shift, 1),
        "k too large": refusal(res.stream_shift, 25),
        "f32 range": f32_range_refusal(res),
    }
    assert refusal(res.stream_shift, -25) == messages["k too large"].replace("k = 25", "k = -25")
    assert len(set(messages.values())) == len(messages), messages
    for what, needle in (("attention", "AttentionTower"), ("dense", "DenseNetwork"), ("no blocks", "without blocks"),
                         ("k too large", "[-24, 24]"), ("f32 range", "normal range")):
        assert messages[what].startswith("kz_model_stream_shift: ") and needle in messages[what], messages[what]
    # the library's strings name no KZ_ identifier here (tests/test_abi.py compares them with the documented list)
    assert not any("KZ_" in m for m in messages.values())
    # the limits themselves are accepted
    assert res.stream_shift(24).info.tower_depth == 2 and res.stream_shift(-24).info.tower_depth == 2
    # the sites: the same three kinds of network are refused, each in its own words
    site_messages = {refusal(m.range_sites) for m in (attention, dense, stem_only)}
    assert len(site_messages) == 2 and all(m.startswith("kz_model_range_sites: ") for m in site_messages)


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_site_count_and_names(depth):
    model = capi.Model(blob=synth.random_model("ataxx-7", depth, 16, "ataxx_conv", seed=1))
    want = ["tower.0"]
    for i in range(1, depth + 1):
        want += [f"tower.{i}.mid", f"tower.{i}" if i < depth else f"tower.{depth + 1}"]
    assert len(want) == 2 * depth + 1
    assert model.range_sites() == want
    assert model.stream_shift(7).range_sites() == want
    n = capi.C.c_int()
    capi.check(capi.load().kz_model_range_sites(model._h, capi.C.byref(n)))
    assert n.value == 2 * depth + 1
    buf = capi.C.create_string_buffer(32)
    for site in (-1, 2 * depth + 1):
        assert capi.load().kz_model_range_site_name(model._h, site, buf, len(buf)) != 0
        assert "out of range" in capi.load().kz_last_error().decode()
    assert capi.load().kz_model_range_site_name(model._h, 1, buf, 4) != 0  # "tower.1.mid" does not fit
    assert "buffer" in capi.load().kz_last_error().decode()


def test_the_profile_checks_its_arguments_before_it_touches_a_gpu():
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 16, "ataxx_conv", seed=1))
    bits, scalars = synth.random_boards("ataxx-7", 3, seed=1)
    with pytest.raises(capi.KzError, match="bits_stride too small"):
        model.range_profile(0, bits[:, :-1], scalars)
    with pytest.raises(capi.KzError, match="batch must be positive"):
        model.range_profile(0, bits[:0], scalars[:0])
    with pytest.raises(capi.KzError, match="AttentionTower|ResTower"):
        capi.Model(blob=O.load_blob("chess_att2x64")).range_profile(0, bits, scalars)


def test_shift_for_follows_the_rule():
    table = [
        # (max |x|, headroom bits, k)
        (65504.0, 0, 0), (65504.0, 2, 2), (65504.0, 5, 5),          # the largest f16: headroom only
        (65505.0, 0, 1), (65505.0, 2, 3),                           # one past it: one binade down
        (1.0, 0, 0), (1.0, 2, 0), (0.0, 0, 0), (0.0, 2, 0), (100.0, 3, 0),       # in range with room to spare: never negative
        (2 * 65504.0, 0, 1), (2 * 65504.0 + 1, 0, 2), (4 * 65504.0, 2, 4),
        (1.0e6, 0, 4), (1.0e6, 2, 6),                               # 1e6 / 65504 = 15.3
        (32752.0, 2, 1), (32753.0, 2, 2), (16376.0, 2, 0),          # the headroom is taken below the limit as well
        (float(np.float32(65504.0 * 4096)), 2, 14),
    ]
    for max_abs, headroom, k in table:
        assert capi.shift_for(max_abs, headroom) == k, (max_abs, headroom)
        want = max(0, int(np.ceil(np.log2(max_abs / 65504.0))) + headroom) if max_abs > 0 else 0
        assert k == want, (max_abs, headroom, want)
    assert capi.shift_for(65505.0) == 3  # the tools' default: two bits
    for bad in (float("inf"), float("nan"), -1.0):
        with pytest.raises(capi.KzError):
            capi.shift_for(bad, 0)
