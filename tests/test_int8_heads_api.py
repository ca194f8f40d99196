"""KZ_DTYPE_INT8_HEADS (dtype 5) without a GPU: the plan is "tower_resident_i8+heads", one launch, exactly where the int8 launch
can carry the conv policy heads and the scalar head, and dtype 4's plan everywhere else.

The rule is restated here in Python (`fused`), from include/kz_hip.h and DESIGN.md 6.2.2, and held against kz_model_plan over
every sweep case and every network of tests/int8_nets.py at four batch sizes:
  conv or ataxx_conv policy head; the tile count of the (widened) channels and the board — 64 rows at 256 channels, at 128
  channels 112 for a board of at most 56 squares, else 64, else 96 —; at most four whole boards in those rows; at most 32
  policy planes, at most 32 scalar-head channels (the extra-move filter counted), at most 256 hidden units; and the tail's
  floats — the scalar head's activations, the extra-move plane, the hidden layer, the last Linear's weights, the partial sums —
  within min(16 KB, 160 KB - the launch's own LDS).
Then the refusals (dtype 4's, saying "dtype 5"), the switches (none is read), the taps and the error profile (refused), the
library's strings, and the committed path table of dtype 5 beside the unchanged one of dtype 4."""
import json
import os
import subprocess
import sys

import pytest

from kzero_amd import capi, synth
from tests import int8_nets
from tests import sweep_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import gen_path_table  # noqa: E402

INT8 = capi.KZ_DTYPE_INT8
FUSED = ("tower_resident_i8+heads", 1)
BATCHES = (1, 8, 256, 2048)
SWITCHES = ("KZ_FORCE_GENERIC", "KZ_KEEP_ACTIVATIONS", "KZ_NO_FUSED_HEADS", "KZ_NO_RESIDENT_F16G", "KZ_NO_BOARD_CONV", "KZ_TOWER_NB")


def res_model(game="chess", depth=2, channels=128, head="attention", **kw):
    return capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))


def calibrated(model):
    return model.quantize_int8([1.0] * len(model.range_sites()))


def refusal(fn, *args):
    with pytest.raises(capi.KzError) as e:
        fn(*args)
    return str(e.value)


def own_lds_bytes(channels, nt):
    """The int8 launch's own LDS: the f16 stream image (rows of 2 C + 16 bytes) rounded to 256, then two planes of
    [X8][Y8][16 zero rows] with rows of C / 2 + 16 bytes, each rounded to 256."""
    rows, rs = nt * 16, channels // 2 + 16
    q_off = -(-rows * (2 * channels + 16) // 256) * 256
    plane = -(-(2 * rows * rs + 16 * rs) // 256) * 256
    return q_off + 2 * plane


def fused(game, channels, head, kw):
    """(the int8 launch carries the heads, boards per workgroup then), from the shape alone."""
    g = synth.game_spec(game)
    hw = g["size"] ** 2
    cp = -(-channels // 64) * 64
    if head not in ("conv", "ataxx_conv"):
        return False, 0
    if cp == 256:
        nt = 4 if hw <= 64 else 0
    elif cp == 128:
        nt = 7 if 2 * hw <= 112 else 4 if hw <= 64 else 6 if hw <= 96 else 0
    else:
        nt = 0
    if not nt:
        return False, 0
    nb = nt * 16 // hw
    hc, hs = kw.get("scalar_hidden_channels", 4), kw.get("scalar_hidden_size", 32)
    pc, extra = (17, 0) if head == "ataxx_conv" else (1, 1)
    if nb > 4 or pc > 32 or hc + (1 if extra else 0) > 32 or hs > 256:
        return False, nb
    nseg = 256 // hs
    floats = nb * hc * hw + nb * hw + nb * hs + 5 * hs + nseg * nb * hs
    return floats * 4 <= min(16 * 1024, 160 * 1024 - own_lds_bytes(cp, nt)), nb


def test_the_constant_and_the_conv_policy_networks_plan_one_launch():
    assert capi.KZ_DTYPE_INT8_HEADS == 5
    for game, channels, head in (("ataxx-7", 128, "ataxx_conv"), ("go-9", 128, "conv"), ("ataxx-7", 256, "ataxx_conv")):
        quant = calibrated(res_model(game, 2, channels, head))
        for mb in (1, 64, 256, 2048):
            assert quant.plan(mb, 5) == FUSED, (game, channels, mb)
            assert quant.plan(mb, INT8)[0] == "tower_resident_i8" and quant.plan(mb, INT8)[1] > 1


def check_plan(name, model, game, channels, head, kw):
    assert model.supports_dtype(5) == model.supports_dtype(INT8) is False, name  # (as loaded: no calibration)
    try:
        quant = calibrated(model)
    except capi.KzError:
        return None
    assert quant.supports_dtype(5) == quant.supports_dtype(INT8), name
    if not quant.supports_dtype(INT8):
        assert "dtype 5" in refusal(quant.plan, 64, 5)
        return None
    want, nb = fused(game, channels, head, kw)
    for mb in BATCHES:
        if want:
            assert quant.plan(mb, 5) == FUSED, (name, mb)
        else:
            assert quant.plan(mb, 5) == quant.plan(mb, INT8), (name, mb)
            assert "+heads" not in quant.plan(mb, 5)[0]
    return want, nb, quant


def test_heads_inside_exactly_where_the_rule_says_across_the_sweep_shapes():
    took = 0
    for case in sweep_cases.CASES:
        model = capi.Model(blob=synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw))
        got = check_plan(case.id, model, case.game, case.channels, case.head, case.kw)
        took += bool(got and got[0])
    assert took >= 5  # Ataxx 5 .. 8 at 128 / 256 channels and Go 9x9 128 with both scalar heads are in the sweep


def test_heads_inside_exactly_where_the_rule_says_across_the_int8_networks():
    expect = {"ataxx7_2x128": 2, "go9_3x128": 1, "ataxx5_2x128": 4, "ataxx6_2x128": 3, "ataxx4_2x256": 4, "ataxx5_2x256": 2,
              "ataxx6_2x256": 1, "ataxx7_2x256": 1, "ataxx7_2x96": 2}
    not_fused = {"ataxx4_2x128": 7, "ataxx2_2x128": 28, "ataxx2_2x256": 16}
    for name, (game, depth, channels, head, kw) in int8_nets.NETS.items():
        blob = synth.random_model(game, depth, channels, head, seed=1, **kw)
        got = check_plan(name, capi.Model(blob=blob), game, channels, head, kw)
        assert got is not None, name  # every network of that table runs in int8
        want, nb, quant = got
        if name in expect:
            assert want and nb == expect[name], (name, want, nb)
        else:
            assert not want, name
        if name in not_fused:
            assert nb == not_fused[name], (name, nb)  # (the shape has a conv head: the boards per workgroup keep it outside)
        if name == "ataxx7_2x96":  # widened to 128, heads included — as the f16 plan of the same blob widens them
            assert ("+heads" in quant.plan(64, 5)[0]) == ("+heads" in capi.Model(blob=blob).plan(64, capi.KZ_DTYPE_F16)[0])
    assert set(expect) | set(not_fused) <= set(int8_nets.NETS)
    for name in ("ttt_2x128_dense", "arimaa_2x96", "chess_2x256_att", "chess_2x128_att", "chess_2x200_att"):
        assert name in int8_nets.NETS and name not in expect


def test_refusals_say_dtype_5_and_other_values_stay_unknown():
    for model in (res_model(), res_model("ataxx-7", 2, 128, "ataxx_conv"), res_model("go-19", 1, 64, "conv"),
                  res_model("chess", 2, 192, "attention")):
        msg = refusal(model.plan, 64, 5)
        assert msg.startswith("kz_model_plan: unknown dtype 5 for a model that carries no int8 calibration"), msg
        assert "KZ_" not in msg and "dtype 4" not in msg
        assert msg.replace("dtype 5", "dtype 4") == refusal(model.plan, 64, INT8)  # the rest of dtype 4's message follows
    wide = calibrated(res_model("chess", 2, 192, "attention"))
    msg = refusal(wide.plan, 64, 5)
    assert "unknown dtype" not in msg and "(dtype 5) has no kernel for this shape" in msg and "the model is calibrated" in msg
    quant = calibrated(res_model("ataxx-7", 2, 128, "ataxx_conv"))
    for dtype in (6, 17):
        assert refusal(quant.plan, 64, dtype) == "kz_model_plan: unknown dtype"
        assert not quant.supports_dtype(dtype)


def test_dtype_5_reads_none_of_the_switches(monkeypatch):
    for game, channels, head in (("ataxx-7", 128, "ataxx_conv"), ("go-9", 96, "conv"), ("chess", 256, "attention")):
        quant = calibrated(res_model(game, 2, channels, head))
        plain = [quant.plan(mb, 5) for mb in BATCHES]
        assert ("+heads" in plain[0][0]) == (head != "attention")
        for name in SWITCHES:
            monkeypatch.setenv(name, "1")
            assert quant.supports_dtype(5) and [quant.plan(mb, 5) for mb in BATCHES] == plain, name
            monkeypatch.delenv(name)


def test_taps_and_the_error_profile_refuse_dtype_5():
    quant = calibrated(res_model("ataxx-7", 2, 128, "ataxx_conv"))
    bits, scalars = synth.random_boards("ataxx-7", 2, seed=1)
    four = refusal(quant.tower_taps_path, 64, INT8)
    five = refusal(quant.tower_taps_path, 64, 5)
    assert "no tap instance" in five and "dtype 5" in five and five.replace("dtype 5", "dtype 4") == four
    assert "no tap instance" in refusal(quant.tower_taps, 0, 64, 5, bits, scalars)
    assert "no tap instance" in refusal(quant.error_profile, 0, 64, 5, bits, scalars)


def test_the_library_names_the_path_and_not_the_constant():
    out = subprocess.run(["strings", "-n", "4", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "tower_resident_i8+heads" in out
    assert "KZ_DTYPE_INT8_HEADS" not in out and "KZ_DTYPE_INT8" not in out


def test_committed_path_tables_are_what_the_selector_chooses():
    committed = json.load(open(gen_path_table.OUT_INT8_HEADS))
    fresh = json.loads(json.dumps(gen_path_table.build_int8_heads()))
    assert committed == fresh, "regenerate with tools/gen_path_table.py --int8-heads"
    four = json.loads(json.dumps(gen_path_table.build_int8()))
    assert four == json.load(open(gen_path_table.OUT_INT8)), "dtype 4's table must not change"
    assert set(fresh["cases"]) == set(four["cases"]) and fresh["max_batch"] == four["max_batch"]
    assert set(fresh["uncalibrated"].values()) == {"refused"}
    n_fused = 0
    for case, row in fresh["cases"].items():
        for a, b in zip(row, four["cases"][case]):
            assert a == b or (a == "tower_resident_i8+heads 1" and b.startswith("tower_resident_i8 ")), (case, a, b)
            n_fused += a != b
    assert n_fused >= 20
