"""The device-weights cache (kzero_amd/csrc/kz_device_weights.hpp: WeightsKey) against mis-sharing: two engines of one model and
one dtype whose plans differ, both alive in one process, each return — bit for bit — what an engine of that plan returns when it
is created alone, in either creation order; and a second engine of an equal key returns the bits of the first.

Engines of one model share packed weight streams wherever their keys are equal, so a key that leaves out something the packing
reads hands the second engine the first one's stream.  tests/test_gpu_range_profile_fast.py section 8 holds the one sharing that
is wanted (the exact-f32 stream with or without heads); this file holds the pairs that must not share, or may share only what is
the same: the pairs are rows of the committed tests/golden/path_table.json ("switches") — switch sets and max_batch values that
change the path name for the same network and dtype — on its depth-1 sweep cases, the smallest networks that reach these paths,
with 5 boards:

  conv_heads   Go 9x9 1x96, f16: the conv heads inside the one-launch tower against separate head launches
  per_layer    chess 1x256 (47 planes), f16: the one-launch tower with its heads against the per-layer implicit GEMM
  att_heads    the same network, f16: the attention heads inside the tower launch against the one-launch kz_att_heads behind it
  att_three    the same network, split arithmetic: the attention heads inside the launch against the three separate launches
  f32_generic  the same network, exact f32: the one-launch tower against the per-layer implicit GEMM
  max_batch    Go 19x19 1x192, f16, no switch: the implicit GEMM at max_batch 8 against the board-tile kernel at 256

The environment switches are set around engine creation only (the selector reads them there)."""
import json
import os

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import sweep_cases

pytestmark = pytest.mark.gpu

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_table.json")))["switches"]
INDEX_CHARS = "".join(chr(c) for c in range(0x21, 0x7f) if chr(c) not in "\\\"")  # (tools/gen_path_table.py)
DTYPES = {"f32": capi.KZ_DTYPE_F32, "f16": capi.KZ_DTYPE_F16, "f32split16": capi.KZ_DTYPE_F32_SPLIT16}
SWITCHES = sorted({k for ks in TABLE["sets"] for k in ks})
BOARDS = 5

CHESS, GO9, GO19 = "chess-hist-2_1x256_attention", "go-9_1x96_conv", "go-19_1x192_conv"
# id: (sweep case, dtype, (max_batch, switch set) of the one engine, of the other)
PAIRS = {
    "conv_heads": (GO9, "f16", (8, ()), (8, ("KZ_NO_FUSED_HEADS",))),
    "per_layer": (CHESS, "f16", (8, ()), (8, ("KZ_FORCE_GENERIC",))),
    "att_heads": (CHESS, "f16", (8, ()), (8, ("KZ_NO_FUSED_HEADS",))),
    "att_three": (CHESS, "f32split16", (8, ()), (8, ("KZ_NO_FUSED_HEADS",))),
    "f32_generic": (CHESS, "f32", (8, ()), (8, ("KZ_FORCE_GENERIC",))),
    "max_batch": (GO19, "f16", (8, ()), (256, ())),
}


def table_entry(case_id, dtype, max_batch, switches):
    """The committed table's "path launches" for this engine."""
    i = (TABLE["dtypes"].index(dtype) * len(TABLE["max_batch"]) + TABLE["max_batch"].index(max_batch)) * len(TABLE["sets"]) + \
        TABLE["sets"].index(list(switches))
    return TABLE["values"][INDEX_CHARS.index(TABLE["cases"][case_id][i])]


class Net:
    """A sweep case's network as the path table draws it, 5 boards, and per plan the outputs of an engine created alone — on a
    model handle of its own, so that nothing is there to share.  Computed once per module and left unchanged."""
    _cache = {}

    def __init__(self, case_id):
        case = next(c for c in sweep_cases.CASES if c.id == case_id)
        self.id = case_id
        self.blob = synth.random_model(case.game, case.depth, case.channels, case.head, seed=11, **case.kw)
        self.bits, self.scalars_in = synth.random_boards(case.game, BOARDS, seed=4)
        self.alone = {}

    @classmethod
    def get(cls, case_id):
        if case_id not in cls._cache:
            cls._cache[case_id] = cls(case_id)
        return cls._cache[case_id]

    def create(self, monkeypatch, model, dtype, max_batch, switches):
        with monkeypatch.context() as mp:
            for k in SWITCHES:
                mp.delenv(k, raising=False)
            for k in switches:
                mp.setenv(k, "1")
            eng = capi.Engine(model, 0, max_batch, DTYPES[dtype])
        assert eng.tower_path == table_entry(self.id, dtype, max_batch, switches).split()[0], (eng.tower_path, dtype, max_batch, switches)
        return eng

    def run(self, eng):
        s, p = eng.eval_packed(self.bits, self.scalars_in)
        assert np.isfinite(s).all() and np.isfinite(p).all()
        return s.copy(), p.copy()

    def expect(self, monkeypatch, dtype, max_batch, switches):
        key = (dtype, max_batch, switches)
        if key not in self.alone:
            eng = self.create(monkeypatch, capi.Model(blob=self.blob), dtype, max_batch, switches)
            out = self.run(eng)
            eng.close()
            for a in out:
                a.setflags(write=False)
            self.alone[key] = out
        return self.alone[key]


def same_bits(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert capi.device_count() >= 1


def test_the_pairs_are_rows_of_the_path_table_that_differ():
    for name, (case_id, dtype, one, other) in PAIRS.items():
        a, b = table_entry(case_id, dtype, *one), table_entry(case_id, dtype, *other)
        assert a != b and "refused" not in (a, b), (name, a, b)
        assert a.split()[0] != b.split()[0], (name, a, b)  # (the path name, not only the launch count)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_engines_of_different_plans_return_what_each_returns_alone(monkeypatch, name, order):
    case_id, dtype, one, other = PAIRS[name]
    net = Net.get(case_id)
    want = [net.expect(monkeypatch, dtype, *plan) for plan in (one, other)]
    # (the two plans do compute different bits here, or the pair could not tell a shared stream from its own)
    print(f"[weights sharing] {name}: {table_entry(case_id, dtype, *one)} | {table_entry(case_id, dtype, *other)}; "
          f"max |d policy| between the plans {np.abs(want[0][1] - want[1][1]).max():.3e}")
    plans = [(one, want[0]), (other, want[1])]
    if order == "reverse":
        plans.reverse()
    model = capi.Model(blob=net.blob)
    engines = [net.create(monkeypatch, model, dtype, *plan) for plan, _ in plans]  # both alive from here on
    for _ in range(2):  # (alternating: neither engine's launches disturb the other's buffers)
        for eng, (plan, expected) in zip(engines, plans):
            assert same_bits(net.run(eng), expected), (name, order, plan)
    # the first engine gone, the second one's stream stays; and an engine of the first plan created now packs its own again
    engines[0].close()
    assert same_bits(net.run(engines[1]), plans[1][1])
    again = net.create(monkeypatch, model, dtype, *plans[0][0])
    assert same_bits(net.run(again), plans[0][1]) and same_bits(net.run(engines[1]), plans[1][1])


@pytest.mark.parametrize("name", list(PAIRS))
def test_a_second_engine_of_an_equal_key_returns_the_bits_of_the_first(monkeypatch, name):
    case_id, dtype, one, _ = PAIRS[name]
    net = Net.get(case_id)
    want = net.expect(monkeypatch, dtype, *one)
    model = capi.Model(blob=net.blob)
    first = net.create(monkeypatch, model, dtype, *one)
    second = net.create(monkeypatch, model, dtype, *one)
    assert same_bits(net.run(first), want) and same_bits(net.run(second), want)
    first.close()  # (the shared stream lives on with the second engine)
    assert same_bits(net.run(second), want)
